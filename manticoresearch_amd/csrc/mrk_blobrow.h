// mrk_blobrow.h -- the load-time walk of the attribute rows' blob rows (mrk_segment_set_blobs).  Plain C++, no HIP: the library calls it
// before a byte of the pool reaches the device, and tests/cpp/filter_edges.cpp runs it on the CPU under AddressSanitizer.
#pragma once
#include <stdint.h>
#include <stdio.h>

namespace mrk {

// Every row's blob row (attribute.cpp:495-513: length-size byte, n_blob cumulative lengths, data) lies inside pool[0, len): the offset
// (the row's second attribute, sphGetBlobRowOffset), the type byte (BLOB_ROW_LEN_BYTE / _WORD / _DWORD), the header, and lengths that
// never descend and end inside the pool.  What row_passes_filters (mrk_dev.h) later dereferences without a check was checked here.
// -> true; or false with the reason in why[why_len].  Reads pool[0, len) and rows[0, n_rows * stride) only.
inline bool blob_rows_inside_pool(const uint8_t* pool, uint64_t len, uint32_t n_blob, const uint32_t* rows, uint32_t stride, uint64_t n_rows, char* why,
                                  size_t why_len) {
  for (uint64_t r = 0; r < n_rows; ++r) {
    const uint32_t* row = rows + r * stride;
    const uint64_t off = (uint64_t)row[2] | ((uint64_t)row[3] << 32);
    if (off >= len) {
      snprintf(why, why_len, "row %llu: blob offset %llu past the pool (%llu bytes)", (unsigned long long)r, (unsigned long long)off, (unsigned long long)len);
      return false;
    }
    const uint8_t* br = pool + off;
    if (br[0] > 2) {
      snprintf(why, why_len, "row %llu: blob row type %u", (unsigned long long)r, br[0]);
      return false;
    }
    const uint32_t sz = br[0] == 0 ? 1u : br[0] == 1 ? 2u : 4u;
    const uint64_t head = 1ull + (uint64_t)n_blob * sz;
    if (len - off < head) {
      snprintf(why, why_len, "row %llu: blob row header past the pool", (unsigned long long)r);
      return false;
    }
    uint64_t prev = 0;
    for (uint32_t a = 0; a < n_blob; ++a) {
      uint64_t l = 0;
      for (uint32_t i = 0; i < sz; ++i) l |= (uint64_t)br[1 + a * sz + i] << (8 * i);
      if (l < prev || l > len - off - head) {
        snprintf(why, why_len, "row %llu: blob attribute %u runs past the pool", (unsigned long long)r, a);
        return false;
      }
      prev = l;
    }
  }
  return true;
}

} // namespace mrk
