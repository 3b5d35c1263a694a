// filter_edges.cpp -- the device's filter functions and the load-time blob-row walk on the CPU, under AddressSanitizer + UBSan.
//   1. mrk::blob_rows_inside_pool (csrc/mrk_blobrow.h, what mrk_segment_set_blobs calls) accepts the crafted rows and pool;
//   2. mrk::row_passes_filters and mrk::weight_passes_filters (csrc/mrk_dev.h, the very functions scan_pk_kernel and rank_kernel call,
//      compiled for the host) answer every (case, row) as the Python model of the reference does (tests/filter_edges_common.py).
//      Rows and pool live in heap blocks of their EXACT size: the library's spare bytes behind its device copies are no part of what
//      is checked here, so a read past a row's last dword or past the pool's last byte is a sanitizer report;
//   3. the walk refuses damaged pools: an offset on the pool's last byte, a header that runs past the end, a two-byte length one
//      past the end (and accepts the same length one smaller), a descending cumulative length, type byte 3.
// Input: the file tests/test_filter_edges_cpu.py writes (layout: read_input below).  No GPU, no libmrk.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include <hip/hip_runtime.h> // (the function qualifiers of mrk_dev.h; no HIP call is made)

#include "../../manticoresearch_amd/csrc/mrk_blobrow.h"
#include "../../manticoresearch_amd/csrc/mrk_dev.h"

static_assert(sizeof(mrk::DevFilter) == 104, "the Python side packs DevFilter as 6 x u32, 2 x i64, 8 x i64");

struct Case {
  uint32_t n_f, n_wf;
  mrk::DevFilter f[MRK_MAX_FILTERS], wf[MRK_MAX_FILTERS];
  std::vector<int32_t> weight;
  std::vector<uint8_t> want;
};

static void need(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s\n", what);
    exit(2);
  }
}

static void get(FILE* fp, void* dst, size_t n) { need(n == 0 || fread(dst, 1, n, fp) == n, "short input file"); }

// a walk that must refuse, for the stated reason
static int refuses(const char* name, const uint8_t* pool, uint64_t len, const uint32_t* row, const char* reason) {
  char why[160] = "";
  uint8_t* exact = (uint8_t*)malloc((size_t)len); // exact size: the walk itself must not read past the pool either
  memcpy(exact, pool, (size_t)len);
  const bool ok = mrk::blob_rows_inside_pool(exact, len, 3, row, 4, 1, why, sizeof why);
  free(exact);
  if (ok || !strstr(why, reason)) {
    printf("WALK %s: %s (%s)\n", name, ok ? "accepted" : "refused for another reason", why);
    return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  need(argc == 2, "usage: filter_edges INPUT");
  FILE* fp = fopen(argv[1], "rb");
  need(fp != nullptr, "cannot open the input file");
  // u64 header: magic, stride (dwords), rows, pool bytes, blob attributes per row, cases; then the rows, the pool, and per case
  // u32 n_filters, u32 n_weight_filters, DevFilter[2] filters, DevFilter[2] weight filters, i32 weight[rows], u8 expected[rows]
  uint64_t h[6];
  get(fp, h, sizeof h);
  need(h[0] == 0x47444546ull, "bad magic");
  const uint32_t stride = (uint32_t)h[1], n_blob = (uint32_t)h[4];
  const uint64_t n_rows = h[2], pool_len = h[3], n_cases = h[5];
  uint32_t* rows = (uint32_t*)malloc((size_t)n_rows * stride * 4);
  uint8_t* pool = (uint8_t*)malloc((size_t)pool_len);
  get(fp, rows, (size_t)n_rows * stride * 4);
  get(fp, pool, (size_t)pool_len);
  std::vector<Case> cases((size_t)n_cases);
  for (Case& c : cases) {
    get(fp, &c.n_f, 4);
    get(fp, &c.n_wf, 4);
    need(c.n_f <= MRK_MAX_FILTERS && c.n_wf <= MRK_MAX_FILTERS, "too many filters in a case");
    get(fp, c.f, sizeof c.f);
    get(fp, c.wf, sizeof c.wf);
    c.weight.resize((size_t)n_rows);
    c.want.resize((size_t)n_rows);
    get(fp, c.weight.data(), (size_t)n_rows * 4);
    get(fp, c.want.data(), (size_t)n_rows);
  }
  fclose(fp);

  int bad = 0;
  char why[160] = "";
  if (!mrk::blob_rows_inside_pool(pool, pool_len, n_blob, rows, stride, n_rows, why, sizeof why)) {
    printf("WALK crafted pool refused: %s\n", why);
    bad++;
  }
  mrk::DevSegment seg;
  memset(&seg, 0, sizeof seg);
  seg.attrs = rows, seg.attr_stride = stride, seg.blobs = pool;
  uint64_t checked = 0;
  if (!bad) // (never evaluate over a pool the walk refused)
    for (size_t ci = 0; ci < cases.size(); ++ci) {
      const Case& c = cases[ci];
      uint64_t n_bad = 0, first = 0;
      for (uint64_t r = 0; r < n_rows; ++r, ++checked) {
        const bool got = mrk::row_passes_filters(seg, c.f, c.n_f, (uint32_t)r) && mrk::weight_passes_filters(c.wf, c.n_wf, c.weight[r]);
        if (got != (c.want[r] != 0) && !n_bad++) first = r;
      }
      if (n_bad) {
        printf("MISMATCH case %zu rows %llu first %llu\n", ci, (unsigned long long)n_bad, (unsigned long long)first);
        bad++;
      }
    }

  // damaged pools: one row (stride 4), three blob attributes, a 64-byte pool
  {
    uint8_t p[64];
    memset(p, 0, sizeof p);
    uint32_t row[4] = {1, 0, 0, 0};
    row[2] = 63; // the type byte is the pool's last byte: no room for the lengths
    bad += refuses("offset on the last byte", p, 64, row, "header past the pool");
    row[2] = 64;
    bad += refuses("offset at the end", p, 64, row, "past the pool");
    row[2] = 61; // type 0: 1 + 3 bytes of header from 61
    bad += refuses("header past the end", p, 64, row, "header past the pool");
    // a two-byte-length row at 40: header 1 + 6 bytes, 17 data bytes left
    row[2] = 40;
    p[40] = 1;
    p[41] = 4, p[43] = 9, p[45] = 17;
    {
      char w[160] = "";
      if (!mrk::blob_rows_inside_pool(p, 64, 3, row, 4, 1, w, sizeof w)) {
        printf("WALK a row that ends on the pool's last byte was refused: %s\n", w);
        bad++;
      }
    }
    p[45] = 18;
    bad += refuses("two-byte length one past the end", p, 64, row, "blob attribute 2 runs past the pool");
    p[45] = 17, p[46] = 1; // 17 + 256: the high byte counts
    bad += refuses("two-byte length, high byte", p, 64, row, "blob attribute 2 runs past the pool");
    p[46] = 0, p[41] = 9, p[43] = 4;
    bad += refuses("descending cumulative length", p, 64, row, "blob attribute 1 runs past the pool");
    p[41] = 4, p[43] = 9, p[40] = 3;
    bad += refuses("type byte 3", p, 64, row, "blob row type 3");
  }
  free(rows);
  free(pool);
  printf("checked %llu\n", (unsigned long long)checked);
  if (bad) return 1;
  printf("ok\n");
  return 0;
}
