// sort_unmap.cpp -- the sort key map and its inverse (csrc/mrk_sortkey.h: sort_map_key, sort_spec_word, sort_unmap_key), host only,
// under AddressSanitizer + UBSan: for integer and float kinds, both directions, bit counts 1 / 5 / 31 / 32, over edge values and
// 10^5 random ones, unmap(spec, map(v)) == v -- except that a float's -0.0 comes back as +0.0 -- and the map stays monotone.
// Built and run by tests/test_sort_merge_cpu.py; no GPU, no libmrk.so.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_sortkey.h"

static int g_bad = 0;
#define CHECK(c, ...)                             \
  do {                                            \
    if (!(c)) {                                   \
      if (g_bad < 20) {                           \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                      \
        printf("\n");                             \
      }                                           \
      ++g_bad;                                    \
    }                                             \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { // xorshift64*
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 32);
}

static float as_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

int main() {
  using namespace mrk;
  uint64_t checked = 0;
  const uint32_t bit_counts[] = {1, 5, 31, 32};
  for (int kind = 0; kind < 2; ++kind)
    for (int desc = 0; desc < 2; ++desc)
      for (uint32_t tie = 0; tie < 3; ++tie)
        for (uint32_t bits : bit_counts) {
          if (kind == 1 && bits != 32) continue; // a float attribute is 32 bits wide
          const uint32_t flags = (kind ? SORT_FLOAT : 0u) | (desc ? SORT_DESC : 0u);
          const uint64_t spec = sort_spec_word(flags, tie, bits);
          CHECK(spec != 0 && (spec & SPEC_SORTED), "spec word of a sorted query is never the relevance word");
          CHECK(sort_spec_tie(spec) == tie && ((spec >> 8) & 63u) == bits && !!(spec & SPEC_FLOAT) == !!kind && !!(spec & SPEC_DESC) == !!desc,
                "spec fields kind %d desc %d tie %u bits %u", kind, desc, tie, bits);
          const uint32_t mask = bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1u;
          std::vector<uint32_t> vals = {0u,          mask,        1u & mask,   mask >> 1,   (mask >> 1) + 1u, // 0, all ones, the middle
                                        0x80000000u & mask, 0x00000001u, 0x80000001u & mask, 0x007FFFFFu & mask, 0x807FFFFFu & mask, // both zeros, denormals
                                        0x7F800000u & mask, 0xFF800000u & mask, 0x7F7FFFFFu & mask, 0xFF7FFFFFu & mask,              // infinities, max finite
                                        0x00800000u & mask, 0x80800000u & mask, 0x3F800000u & mask, 0xBF800000u & mask};
          for (int i = 0; i < 100000; ++i) vals.push_back(rnd() & mask);
          uint32_t prev_v = 0, prev_m = 0;
          bool have_prev = false;
          for (uint32_t v : vals) {
            if (kind == 1 && sort_is_nan(v)) continue; // a column with a NaN is declined by the planner: no order to keep
            const uint32_t m = sort_map_key(v, flags);
            const uint32_t back = sort_unmap_key(spec, m);
            const uint32_t want = (kind == 1 && v == 0x80000000u) ? 0u : v; // -0.0 reads +0.0
            CHECK(back == want, "kind %d desc %d bits %u: v %08x -> m %08x -> %08x", kind, desc, bits, v, m, back);
            if (have_prev) { // monotone: "better" (larger mapped key) = larger value under desc, smaller under asc; equal values map equal
              int cmp;
              if (kind == 1) {
                const float a = as_float(prev_v), b = as_float(v);
                cmp = a < b ? -1 : a > b ? 1 : 0;
              } else
                cmp = prev_v < v ? -1 : prev_v > v ? 1 : 0;
              if (!desc) cmp = -cmp;
              const int mc = prev_m < m ? -1 : prev_m > m ? 1 : 0;
              CHECK(cmp == mc, "kind %d desc %d bits %u: order of %08x / %08x is %d, of the mapped keys %d", kind, desc, bits, prev_v, v, cmp, mc);
            }
            prev_v = v, prev_m = m, have_prev = true;
            ++checked;
          }
        }
  CHECK(sort_spec_tie(0) == 1u, "a relevance row orders by weight descending");
  if (g_bad) {
    printf("%d failures\n", g_bad);
    return 1;
  }
  printf("ok unmap %llu values\n", (unsigned long long)checked);
  return 0;
}
