// order_unmap.cpp -- the 64-bit order key map and its inverse under a spec word (csrc/mrk_sortkey.h: order_map_i64, order_map_part,
// order_spec_word, order_unmap_key), host only, under AddressSanitizer + UBSan.  INT64 in both directions over INT64_MIN, -1, 0, 1,
// INT64_MAX and random values; every pair of <= 32-bit kinds (integer, float, bit-fields of 1 / 5 / 31 bits) and directions; a sort
// spec (one part, key in the high dword).  unmap(spec, map(v)) == v, except that a float's -0.0 reads +0.0; the map stays monotone
// in the order the spec states; spec words that differ in what they state differ.
// Built and run by tests/test_order_merge_cpu.py; no GPU, no libmrk.so.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
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
static uint64_t rnd64() { // xorshift64*
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return g_rng * 0x2545F4914F6CDD1Dull;
}

static float as_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// -1 / 0 / 1: how raw values a, b of one part compare in the part's own order (ascending)
static int cmp_part(uint32_t a, uint32_t b, bool is_float) {
  if (is_float) {
    const float x = as_float(a), y = as_float(b);
    return x < y ? -1 : x > y ? 1 : 0;
  }
  return a < b ? -1 : a > b ? 1 : 0;
}

struct Kind {
  bool is_float;
  uint32_t bits;
};

int main() {
  using namespace mrk;
  uint64_t checked = 0;
  std::set<uint64_t> specs;
  // ---- one signed 64-bit attribute
  for (int desc = 0; desc < 2; ++desc)
    for (uint32_t tie = 0; tie < 3; ++tie) {
      const uint32_t f = desc ? SORT_DESC : 0u;
      const uint64_t spec = order_spec_word(SORT_ON_ORDER, f | SORT_SIGNED | SORT_WIDE, 32, f, 32, tie);
      specs.insert(spec);
      CHECK((spec & OSPEC_ORDERED) && (spec & OSPEC_WIDE) && (spec & OSPEC_INT64) && order_spec_tie(spec) == tie, "INT64 spec fields desc %d tie %u", desc, tie);
      std::vector<int64_t> vals = {INT64_MIN, -1, 0, 1, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1, (int64_t)0xFFFFFFFFll, (int64_t)0x100000000ll, -(int64_t)0x100000000ll};
      for (int i = 0; i < 100000; ++i) vals.push_back((int64_t)rnd64());
      int64_t pv = 0;
      uint64_t pm = 0;
      bool have = false;
      for (int64_t v : vals) {
        const uint64_t m = order_map_i64(v, desc != 0);
        // the same key from the two dwords, as the kernels build it
        const uint64_t m2 = order_key(order_map_part((uint32_t)((uint64_t)v >> 32), f | SORT_SIGNED), order_map_part((uint32_t)(uint64_t)v, f));
        CHECK(m == m2, "INT64 %lld: map %016llx, from its dwords %016llx", (long long)v, (unsigned long long)m, (unsigned long long)m2);
        CHECK((int64_t)order_unmap_key(spec, m) == v, "INT64 desc %d: %lld -> %016llx -> %lld", desc, (long long)v, (unsigned long long)m, (long long)(int64_t)order_unmap_key(spec, m));
        if (have) {
          int c = pv < v ? -1 : pv > v ? 1 : 0;
          if (!desc) c = -c;
          const int mc = pm < m ? -1 : pm > m ? 1 : 0;
          CHECK(c == mc, "INT64 desc %d: order of %lld / %lld is %d, of the mapped keys %d", desc, (long long)pv, (long long)v, c, mc);
        }
        pv = v, pm = m, have = true;
        ++checked;
      }
    }
  // ---- two parts of <= 32 bits, every pair of kinds and directions
  const Kind kinds[] = {{false, 32}, {true, 32}, {false, 1}, {false, 5}, {false, 31}};
  const uint32_t edge[] = {0u, 1u, 0x80000000u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0x7F800000u, 0xFF800000u, 0x00000001u, 0x80000001u, 0x3F800000u, 0xBF800000u};
  for (const Kind& A : kinds)
    for (const Kind& B : kinds)
      for (int da = 0; da < 2; ++da)
        for (int db = 0; db < 2; ++db) {
          const uint32_t fa = (A.is_float ? SORT_FLOAT : 0u) | (da ? SORT_DESC : 0u), fb = (B.is_float ? SORT_FLOAT : 0u) | (db ? SORT_DESC : 0u);
          const uint32_t tie = (uint32_t)(da + 2 * db) % 3u;
          const uint64_t spec = order_spec_word(SORT_ON_ORDER, fa | SORT_WIDE, A.bits, fb, B.bits, tie);
          specs.insert(spec);
          CHECK((spec & OSPEC_WIDE) && !(spec & OSPEC_INT64) && order_spec_tie(spec) == tie && order_spec_flags(spec, 0) == fa && order_spec_flags(spec, 1) == fb,
                "pair spec fields");
          const uint32_t ma = A.bits >= 32 ? 0xFFFFFFFFu : (1u << A.bits) - 1u, mb = B.bits >= 32 ? 0xFFFFFFFFu : (1u << B.bits) - 1u;
          uint32_t pa = 0, pb = 0;
          uint64_t pm = 0;
          bool have = false;
          for (int i = 0; i < 4000; ++i) {
            const uint64_t r = rnd64();
            // (few distinct first values, so that the second part decides often)
            uint32_t a = i < 121 ? edge[i / 11] : (i & 1) ? (uint32_t)(r >> 32) : edge[(r >> 40) % 11], b = i < 121 ? edge[i % 11] : (uint32_t)r;
            a &= ma, b &= mb;
            if ((A.is_float && sort_is_nan(a)) || (B.is_float && sort_is_nan(b))) continue;
            const uint64_t m = order_key(order_map_part(a, fa), order_map_part(b, fb));
            const uint64_t back = order_unmap_key(spec, m);
            const uint32_t wa = A.is_float && a == 0x80000000u ? 0u : a, wb = B.is_float && b == 0x80000000u ? 0u : b; // -0.0 reads +0.0
            CHECK(back == (((uint64_t)wa << 32) | wb), "pair: %08x %08x -> %016llx -> %016llx", a, b, (unsigned long long)m, (unsigned long long)back);
            if (have) {
              int c = cmp_part(pa, a, A.is_float);
              if (!da) c = -c;
              if (c == 0) {
                c = cmp_part(pb, b, B.is_float);
                if (!db) c = -c;
              }
              const int mc = pm < m ? -1 : pm > m ? 1 : 0;
              CHECK(c == mc, "pair: order of (%08x %08x) / (%08x %08x) is %d, of the mapped keys %d", pa, pb, a, b, c, mc);
            }
            pa = a, pb = b, pm = m, have = true;
            ++checked;
          }
        }
  // ---- a sort travels with its 32-bit key in the high dword
  for (const Kind& A : kinds)
    for (int da = 0; da < 2; ++da) {
      const uint32_t fa = (A.is_float ? SORT_FLOAT : 0u) | (da ? SORT_DESC : 0u);
      const uint64_t spec = order_spec_word(SORT_ON_ATTR, fa, A.bits, 0xFFFFFFFFu, 0xFFFFFFFFu, 1); // (the second part's words are not read)
      specs.insert(spec);
      CHECK((spec & OSPEC_ORDERED) && !(spec & OSPEC_WIDE) && (spec >> 24) == 0, "sort spec");
      const uint32_t ma = A.bits >= 32 ? 0xFFFFFFFFu : (1u << A.bits) - 1u;
      for (uint32_t e : edge) {
        const uint32_t a = e & ma;
        if (A.is_float && sort_is_nan(a)) continue;
        const uint64_t m = (uint64_t)sort_map_key(a, fa) << 32;
        const uint32_t wa = A.is_float && a == 0x80000000u ? 0u : a;
        CHECK(order_unmap_key(spec, m) == (uint64_t)wa << 32, "sort: %08x", a);
        CHECK((uint32_t)(order_unmap_key(spec, m) >> 32) == sort_unmap_key(sort_spec_word(fa, 1, A.bits), (uint32_t)(m >> 32)), "sort: the wide rows' inverse agrees");
        ++checked;
      }
    }
  CHECK(specs.size() == 6 + 5 * 5 * 4 + 5 * 2, "spec words that state different orders differ: %zu distinct", specs.size());
  CHECK(order_spec_word(0, 3, 32, 3, 32, 2) == 0 && order_spec_tie(0) == 1u && order_unmap_key(0, 12345) == 0, "a relevance row: spec 0, weight descending");
  if (g_bad) {
    printf("%d failures\n", g_bad);
    return 1;
  }
  printf("ok order unmap %llu values\n", (unsigned long long)checked);
  return 0;
}
