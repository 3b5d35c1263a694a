// weight_first_spec.cpp -- the order spec word of a weight-first order (csrc/mrk_sortkey.h: order_spec_word_wfirst, OSPEC_WFIRST) and
// order_unmap_key under it, host only, under AddressSanitizer + UBSan.  Every accepted shape of parts -- none (weight ASC alone), one
// part of <= 32 bits, two parts, one INT64 -- under both directions of the weight, built from the words the planner puts into a
// weight-first DevQuery.  Checked here: bit 3 is set exactly for weight-first; bits 4-5 hold the weight's direction; every other field
// equals the same parts' attribute-first spec; unmap under the weight-first spec equals unmap under that spec, and inverts the map;
// a spec without parts unmaps to 0.  Every spec is also printed, one line per shape, for tests/test_weight_first_merge_cpu.py to hold
// against dist.order_spec_word:
//   S <weight_first> <then_weight> <n_parts> <int64> <float0> <bits0> <desc0> <float1> <bits1> <desc1> <spec, hex>
// Built and run by tests/test_weight_first_merge_cpu.py; no GPU, no libmrk.so.
#include <stdint.h>
#include <stdio.h>

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

struct Kind {
  bool is_float;
  uint32_t bits;
};

static uint32_t part_flags(const Kind& k, int desc) { return (k.is_float ? mrk::SORT_FLOAT : 0u) | (desc ? mrk::SORT_DESC : 0u); }

static void line(uint32_t wf, uint32_t tw, int n_parts, int i64, const Kind& a, int da, const Kind& b, int db, uint64_t spec) {
  printf("S %u %u %d %d %d %u %d %d %u %d %016llx\n", wf, tw, n_parts, i64, (int)a.is_float, a.bits, da, (int)b.is_float, b.bits, db, (unsigned long long)spec);
}

int main() {
  using namespace mrk;
  const Kind kinds[] = {{false, 32}, {true, 32}, {false, 1}, {false, 5}, {false, 31}};
  const Kind none{false, 0}, dw{false, 32};
  const uint64_t rest = ~(OSPEC_WFIRST | (3ull << 4)); // everything but bit 3 and bits 4-5
  uint64_t checked = 0;
  // the attribute-first specs, as they were: printed for the Python side, bit 3 clear
  for (uint32_t tw = 0; tw < 3; ++tw) {
    for (const Kind& A : kinds)
      for (int da = 0; da < 2; ++da) {
        const uint64_t s1 = order_spec_word(SORT_ON_ATTR, part_flags(A, da), A.bits, 0, 0, tw);
        CHECK(!(s1 & OSPEC_WFIRST), "a sort spec has bit 3 clear");
        line(0, tw, 1, 0, A, da, none, 0, s1);
        for (const Kind& B : kinds)
          for (int db = 0; db < 2; ++db) {
            const uint64_t s2 = order_spec_word(SORT_ON_ORDER, part_flags(A, da) | SORT_WIDE, A.bits, part_flags(B, db), B.bits, tw);
            CHECK(!(s2 & OSPEC_WFIRST), "a two-part spec has bit 3 clear");
            line(0, tw, 2, 0, A, da, B, db, s2);
          }
      }
    for (int d = 0; d < 2; ++d) {
      const uint32_t f = d ? SORT_DESC : 0u;
      const uint64_t s = order_spec_word(SORT_ON_ORDER, f | SORT_SIGNED | SORT_WIDE, 32, f, 32, tw);
      CHECK(!(s & OSPEC_WFIRST), "an INT64 spec has bit 3 clear");
      line(0, tw, 1, 1, dw, d, dw, d, s);
    }
  }
  for (uint32_t wf = 1; wf <= 2; ++wf) {
    // ---- one part of <= 32 bits: the planner's sort_flags = SORT_WFIRST | the part's; ord_* are not read
    for (const Kind& A : kinds)
      for (int da = 0; da < 2; ++da) {
        const uint32_t fa = part_flags(A, da);
        const uint64_t spec = order_spec_word_wfirst(SORT_WFIRST | fa, A.bits, 0xFFFFFFFFu, 0xFFFFFFFFu, wf, 1);
        const uint64_t plain = order_spec_word(SORT_ON_ATTR, fa, A.bits, 0, 0, wf);
        CHECK((spec & OSPEC_WFIRST) && order_spec_wfirst_valid(spec) && ((spec >> 4) & 3u) == wf, "one part: bit 3 and the direction");
        CHECK((spec & rest) == (plain & rest) && !(spec & OSPEC_WIDE) && (spec >> 24) == 0, "one part: the fields of the same parts' sort spec");
        line(wf, 0, 1, 0, A, da, none, 0, spec);
        const uint32_t ma = A.bits >= 32 ? 0xFFFFFFFFu : (1u << A.bits) - 1u;
        for (int i = 0; i < 2000; ++i) {
          const uint32_t a = (uint32_t)rnd64() & ma;
          if (A.is_float && sort_is_nan(a)) continue;
          const uint64_t m = order_key(order_map_part(a, fa), 0u);
          const uint32_t wa = A.is_float && a == 0x80000000u ? 0u : a; // -0.0 reads +0.0
          CHECK(order_unmap_key(spec, m) == (uint64_t)wa << 32 && order_unmap_key(spec, m) == order_unmap_key(plain, m), "one part: %08x", a);
          ++checked;
        }
        // ---- two parts
        for (const Kind& B : kinds)
          for (int db = 0; db < 2; ++db) {
            const uint32_t fb = part_flags(B, db);
            const uint64_t spec2 = order_spec_word_wfirst(SORT_WFIRST | fa, A.bits, fb, B.bits, wf, 2);
            const uint64_t plain2 = order_spec_word(SORT_ON_ORDER, fa | SORT_WIDE, A.bits, fb, B.bits, wf);
            CHECK((spec2 & OSPEC_WFIRST) && ((spec2 >> 4) & 3u) == wf && (spec2 & rest) == (plain2 & rest) && (spec2 & OSPEC_WIDE) && !(spec2 & OSPEC_INT64), "two parts: fields");
            CHECK(order_spec_flags(spec2, 0) == fa && order_spec_flags(spec2, 1) == fb, "two parts: the parts' flags");
            line(wf, 0, 2, 0, A, da, B, db, spec2);
            const uint32_t mb = B.bits >= 32 ? 0xFFFFFFFFu : (1u << B.bits) - 1u;
            for (int i = 0; i < 200; ++i) {
              const uint64_t r = rnd64();
              const uint32_t a = (uint32_t)(r >> 32) & ma, b = (uint32_t)r & mb;
              if ((A.is_float && sort_is_nan(a)) || (B.is_float && sort_is_nan(b))) continue;
              const uint64_t m = order_key(order_map_part(a, fa), order_map_part(b, fb));
              const uint32_t wa = A.is_float && a == 0x80000000u ? 0u : a, wb = B.is_float && b == 0x80000000u ? 0u : b;
              CHECK(order_unmap_key(spec2, m) == (((uint64_t)wa << 32) | wb) && order_unmap_key(spec2, m) == order_unmap_key(plain2, m), "two parts: %08x %08x", a, b);
              ++checked;
            }
          }
      }
    // ---- one INT64: high dword signed in sort_*, low dword plain in ord_*, two dwords
    for (int d = 0; d < 2; ++d) {
      const uint32_t f = d ? SORT_DESC : 0u;
      const uint64_t spec = order_spec_word_wfirst(SORT_WFIRST | f | SORT_SIGNED, 32, f, 32, wf, 2);
      const uint64_t plain = order_spec_word(SORT_ON_ORDER, f | SORT_SIGNED | SORT_WIDE, 32, f, 32, wf);
      CHECK((spec & OSPEC_WFIRST) && ((spec >> 4) & 3u) == wf && (spec & rest) == (plain & rest) && (spec & OSPEC_WIDE) && (spec & OSPEC_INT64), "INT64: fields");
      line(wf, 0, 1, 1, dw, d, dw, d, spec);
      const int64_t edge[] = {INT64_MIN, -1, 0, 1, INT64_MAX};
      for (int i = 0; i < 5000; ++i) {
        const int64_t v = i < 5 ? edge[i] : (int64_t)rnd64();
        const uint64_t m = order_map_i64(v, d != 0);
        CHECK((int64_t)order_unmap_key(spec, m) == v && order_unmap_key(spec, m) == order_unmap_key(plain, m), "INT64 desc %d: %lld", d, (long long)v);
        ++checked;
      }
    }
    // ---- no parts: both part fields zero whatever the part words hold; unmaps to 0.  (The planner accepts it under weight ASC only; the
    // word itself is built for either direction.)
    const uint64_t spec0 = order_spec_word_wfirst(SORT_WFIRST, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, wf, 0);
    CHECK(spec0 == (OSPEC_ORDERED | OSPEC_WFIRST | ((uint64_t)wf << 4)), "no parts: %016llx", (unsigned long long)spec0);
    CHECK(order_unmap_key(spec0, 0) == 0 && order_unmap_key(spec0, rnd64()) == 0, "no parts unmap to 0");
    if (wf == 2) line(wf, 0, 0, 0, none, 0, none, 0, spec0);
  }
  // directions that are none
  CHECK(!order_spec_wfirst_valid(OSPEC_ORDERED | OSPEC_WFIRST) && !order_spec_wfirst_valid(OSPEC_ORDERED | OSPEC_WFIRST | (3ull << 4)), "direction 0 / 3 is no spec");
  if (g_bad) {
    printf("%d failures\n", g_bad);
    return 1;
  }
  printf("ok weight-first spec %llu values\n", (unsigned long long)checked);
  return 0;
}
