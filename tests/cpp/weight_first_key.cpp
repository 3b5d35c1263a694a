// weight_first_key.cpp -- the weight-first candidate layout of csrc/mrk_sortkey.h (the weight in front of an order: mrk_order::then_weight = MRK_ORDER_WEIGHT_FIRST_*) on the host, under
// AddressSanitizer + UBSan: (hi, lo) compared as 128 bits against a comparator written from the order's definition (MatchGeneric2_fn /
// 3_fn with SPH_KEYPART_WEIGHT as key part 0: weight, the parts in their order and directions, rowid ascending), the inverse maps, and
// the weight's pruning bin.  Built and run by tests/test_weight_first_cpu.py; no GPU, no libmrk.so.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_sortkey.h"

static int g_bad = 0;
#define CHECK(c, ...)                               \
  do {                                              \
    if (!(c)) {                                     \
      if (g_bad < 50) {                             \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                        \
        printf("\n");                               \
      }                                             \
      ++g_bad;                                      \
    }                                               \
  } while (0)

static uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static float bitsf(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}

struct Row {
  uint32_t v0, v1; // the parts' raw values (a 64-bit attribute: high, low dword)
  int32_t w;
  uint32_t rowid;
  uint64_t hi, lo;
};
struct Spec {
  uint32_t wf;     // 1 = weight DESC, 2 = weight ASC
  int shape;       // 0 = no parts, 1 = one part of <= 32 bits, 2 = two parts, 3 = one INT64
  uint32_t f0, f1; // SORT_FLOAT | SORT_DESC per part
};
static int cmp_part(uint32_t a, uint32_t b, uint32_t fl) { // < 0: a is BETTER
  int c;
  if (fl & mrk::SORT_FLOAT) {
    const float x = bitsf(a), y = bitsf(b);
    c = x < y ? -1 : x > y ? 1 : 0;
  } else
    c = a < b ? -1 : a > b ? 1 : 0;
  return (fl & mrk::SORT_DESC) ? -c : c;
}
static bool better(const Row& a, const Row& b, const Spec& s) {
  if (a.w != b.w) return s.wf == 1 ? a.w > b.w : a.w < b.w;
  int c = 0;
  if (s.shape == 3) {
    const int64_t x = (int64_t)(((uint64_t)a.v0 << 32) | a.v1), y = (int64_t)(((uint64_t)b.v0 << 32) | b.v1);
    c = x < y ? -1 : x > y ? 1 : 0;
    if (s.f0 & mrk::SORT_DESC) c = -c;
  } else {
    if (s.shape >= 1) c = cmp_part(a.v0, b.v0, s.f0);
    if (!c && s.shape == 2) c = cmp_part(a.v1, b.v1, s.f1);
  }
  if (c) return c < 0;
  return a.rowid < b.rowid;
}
static uint32_t pick_int(uint64_t r) {
  static const uint32_t v[] = {0u, 1u, 7u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  return v[r % 7];
}
static float pick_float(uint64_t r) {
  static const float v[] = {-INFINITY, -2.5f, -0.0f, 0.0f, 1.0e-40f, 0.5f, 2.5f, INFINITY};
  return v[r % 8];
}
static int32_t pick_weight(uint64_t r) {
  static const int32_t v[] = {INT32_MIN, INT32_MIN + 1, -100000, -1, 0, 1, 1427, 2414, 3442, INT32_MAX - 1, INT32_MAX};
  return v[r % 11];
}
static int64_t pick_i64(uint64_t r) {
  static const int64_t v[] = {INT64_MIN, INT64_MIN + 1, -0x100000000ll, -1, 0, 1, 0xFFFFFFFFll, 0x100000000ll, INT64_MAX};
  return v[r % 9];
}

int main() {
  using namespace mrk;
  const int N = 3000;
  int variants = 0;
  for (uint32_t wf = 1; wf <= 2; ++wf)
    for (int shape = 0; shape <= 3; ++shape)
      for (int dirs = 0; dirs < 4; ++dirs)
        for (int fl = 0; fl < 3; ++fl) { // which part is a float: none, the first, the second
          if (shape == 0 && (dirs || fl)) continue;
          if ((shape == 1 || shape == 3) && (dirs > 1 || fl == 2)) continue;
          if (shape == 3 && fl) continue;
          Spec s{wf, shape, (dirs & 1) ? SORT_DESC : 0u, (dirs & 2) ? SORT_DESC : 0u};
          if (fl == 1) s.f0 |= SORT_FLOAT;
          if (fl == 2) s.f1 |= SORT_FLOAT;
          ++variants;
          const uint32_t np = shape == 3 ? 2u : (uint32_t)shape;
          const OrderPart p0{0u, 0u, 32u, s.f0 | (shape == 3 ? SORT_SIGNED : 0u)}, p1{1u, 0u, 32u, shape == 3 ? s.f0 : s.f1};
          std::vector<Row> rows((size_t)N);
          for (int i = 0; i < N; ++i) {
            Row& r = rows[(size_t)i];
            if (shape == 3) {
              const int64_t v = pick_i64(rnd());
              r.v0 = (uint32_t)((uint64_t)v >> 32), r.v1 = (uint32_t)(uint64_t)v;
            } else {
              r.v0 = (s.f0 & SORT_FLOAT) ? fbits(pick_float(rnd())) : pick_int(rnd());
              r.v1 = (s.f1 & SORT_FLOAT) ? fbits(pick_float(rnd())) : pick_int(rnd());
            }
            r.w = pick_weight(rnd());
            r.rowid = i % 5 == 0 ? 0xFFFFFFFFu - (uint32_t)i : (uint32_t)i * 3u + 5u;
            const uint32_t row[2] = {r.v0, r.v1};
            const uint64_t pk = wfirst_row_key(np ? row : nullptr, np, p0, p1);
            r.hi = wfirst_hi(wf, r.w, pk), r.lo = wfirst_lo(pk, r.rowid);
            // the inverse maps: weight, rowid, the raw parts (a float's -0.0 reads +0.0)
            CHECK(wfirst_weight(wf, r.hi) == r.w && wfirst_rowid(r.lo) == r.rowid, "weight / rowid round trip: w %d rowid %u", r.w, r.rowid);
            CHECK(wfirst_parts_key(r.hi, r.lo) == pk, "parts key out of (hi, lo)");
            if (shape == 3) {
              const int64_t v = (int64_t)(((uint64_t)r.v0 << 32) | r.v1);
              CHECK(pk == order_map_i64(v, (s.f0 & SORT_DESC) != 0) && order_unmap_i64(pk, (s.f0 & SORT_DESC) != 0) == v, "a 64-bit part is its mapped key");
            } else {
              auto raw = [](uint32_t v, uint32_t f) { return (f & SORT_FLOAT) && (v << 1) == 0u ? 0u : v; };
              if (np >= 1) CHECK(order_unmap_part((uint32_t)(pk >> 32), p0.flags) == raw(r.v0, s.f0), "first part back");
              if (np == 2) CHECK(order_unmap_part((uint32_t)pk, p1.flags) == raw(r.v1, s.f1), "second part back");
              if (np < 2) CHECK((uint32_t)pk == 0u, "d2 of a missing second part");
              if (np < 1) CHECK(pk == 0ull, "d1 : d2 without parts");
            }
          }
          std::vector<Row> by_key = rows, by_def = rows;
          std::sort(by_key.begin(), by_key.end(), [](const Row& a, const Row& b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); });
          std::sort(by_def.begin(), by_def.end(), [&](const Row& a, const Row& b) { return better(a, b, s); });
          for (int i = 0; i < N; ++i)
            if (by_key[(size_t)i].rowid != by_def[(size_t)i].rowid) {
              CHECK(false, "wf %u shape %d dirs %d float %d: (hi, lo) order differs from the definition at %d", wf, shape, dirs, fl, i);
              break;
            }
          // the weight's bin: monotone along the 128-bit order (walked best first: non-increasing), inside the histogram, for the
          // geometries the planner hands out -- the fallback (INT32_MIN, 31), a narrow band, a band the extreme weights fall outside of
          const struct { int32_t lo; uint32_t shift; } geoms[] = {{INT32_MIN, 31u}, {INT32_MIN, 22u}, {0, 2u}, {-100000, 8u}, {1000, 0u}, {INT32_MAX - 5, 0u}};
          for (const auto& g : geoms) {
            uint32_t prev = 1023u;
            for (const Row& r : by_key) {
              const uint32_t b = wfirst_bin(wf, g.lo, g.shift, wfirst_weight(wf, r.hi));
              CHECK(b <= prev && b < 1024u, "wf %u: bin %u after %u (lo %d shift %u)", wf, b, prev, g.lo, g.shift);
              prev = b;
            }
          }
          CHECK(wfirst_bin(wf, 1000, 2u, 1000 + 4 * 700) == (wf == 1 ? 700u : 1023u - 700u), "the relevance bin, complemented for weight ASC");
        }
  CHECK(variants == 2 * (1 + 4 + 12 + 2), "variants %d", variants);
  if (g_bad) return printf("%d checks failed\n", g_bad), 1;
  printf("ok variants %d\n", variants);
  return 0;
}
