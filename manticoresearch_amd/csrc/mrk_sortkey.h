// mrk_sortkey.h -- the order-preserving 32-bit map of a sorter's primary attribute (mrk_query.sort), one definition for the
// planner, the kernels and the CPU unit test.  "Larger mapped key = better" always holds: unsigned integers as they are,
// floats by the usual sign flip with -0.0 folded onto +0.0 (SPH_KEYPART_FLOAT compares floats: the two zeros are equal and
// the comparison falls through to the next key part), ascending orders complemented.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRK_HD __host__ __device__
#else
#define MRK_HD
#endif

namespace mrk {

constexpr uint32_t SORT_FLOAT = 1, SORT_DESC = 2; // DevQuery::sort_flags

// the attribute's bits out of its dword (sphGetRowAttr, sphinx.h:993-1014, for locators of <= 32 bits)
MRK_HD inline uint32_t sort_extract(uint32_t dword, uint32_t shift, uint32_t bits) { return bits >= 32u ? dword : (dword >> shift) & ((1u << bits) - 1u); }

MRK_HD inline bool sort_is_nan(uint32_t v) { return (v & 0x7FFFFFFFu) > 0x7F800000u; }

MRK_HD inline uint32_t sort_map_key(uint32_t v, uint32_t flags) {
  uint32_t m = v;
  if (flags & SORT_FLOAT) {
    if ((v << 1) == 0u) v = 0u; // -0.0 == +0.0
    m = (v & 0x80000000u) ? ~v : (v | 0x80000000u);
  }
  return (flags & SORT_DESC) ? m : ~m;
}

// The sort spec word of a wide exchange row (MRK_SROW_WORDS, include/mrk.h): everything that decides whether two shards' mapped
// keys and tie rules compare, and nothing of where a segment stores the column.  0 = a relevance query.
//   bit 0 sorted | bit 1 float | bit 2 desc | bits 4-5 then_weight | bits 8-13 bit_count
constexpr uint64_t SPEC_SORTED = 1, SPEC_FLOAT = 2, SPEC_DESC = 4;
MRK_HD inline uint64_t sort_spec_word(uint32_t flags, uint32_t tie, uint32_t bits) {
  return SPEC_SORTED | ((flags & SORT_FLOAT) ? SPEC_FLOAT : 0u) | ((flags & SORT_DESC) ? SPEC_DESC : 0u) | ((uint64_t)(tie & 3u) << 4) | ((uint64_t)(bits & 63u) << 8);
}
MRK_HD inline uint32_t sort_spec_tie(uint64_t spec) { return spec ? (uint32_t)(spec >> 4) & 3u : 1u; } // relevance = weight desc

// the inverse of sort_map_key under a spec word: the attribute's raw value (a float's -0.0 was folded onto +0.0 and reads +0.0)
MRK_HD inline uint32_t sort_unmap_key(uint64_t spec, uint32_t mapped) {
  const uint32_t m = (spec & SPEC_DESC) ? mapped : ~mapped;
  if (!(spec & SPEC_FLOAT)) return m;
  return (m & 0x80000000u) ? (m ^ 0x80000000u) : ~m;
}

// pruning bin of a mapped key: monotone non-decreasing in it; lo / shift come from the column's range (mrk_plan.cpp)
MRK_HD inline uint32_t sort_bin(uint32_t lo, uint32_t shift, uint32_t mapped) {
  if (mapped < lo) return 0u;
  const uint32_t b = (mapped - lo) >> shift;
  return b < 1023u ? b : 1023u;
}

// A candidate of a sorted query is 128 bits, compared as (hi, lo), larger = better:
//   hi = mapped key << 32 | the weight as the tie rule orders it (0 where the weight is no part of the order)
//   lo = ~global rowid << 32 | the true weight
MRK_HD inline uint32_t sort_weight_part(uint32_t tie, int32_t weight) {
  const uint32_t w = (uint32_t)weight ^ 0x80000000u;
  return tie == 1u ? w : tie == 2u ? ~w : 0u;
}

#undef MRK_HD
} // namespace mrk
