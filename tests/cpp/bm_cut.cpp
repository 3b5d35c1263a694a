// bm_cut.cpp -- the two-bitmap AND kernel's per-threshold cutoff (mrk::bm_wmax_cut, csrc/mrk_kcommon.h) on the CPU, under AddressSanitizer + UBSan.
// The kernel used to test every match word's weight bound with
//   weight_bin(bin_lo, bin_shift, (int32_t)(((uint32_t)x + rmax1000) * index_weight)) < tau_bin
// (x = the bound's (int32_t)((acc + 0.5f) * 1000.0f)); it now tests x < bm_wmax_cut(bin_lo, bin_shift, tau_bin, rmax1000, index_weight), the
// cutoff worked out once per threshold.  The expression above stays here, verbatim, as the reference, and the two are compared
//   - for bin geometries made the way bins_by_weight (csrc/mrk_plan.cpp) makes them: idf pairs of either sign, field-weight sets with positive,
//     zero and negative entries (bin_lo < 0, T = bin_lo + (tau_bin << bin_shift) <= 0), index weights 1, 2, 3, 7, 1000 and 65535, and ranges of
//     x pushed up against the int32 ends the planner still accepts; the planner's own shift and every shift 0..22;
//   - for tau_bin 0, 1, 2, 511, 1022, 1023;
//   - at x within +-3 of the cutoff, at both ends of the reachable range of x, and at seeded random values inside it.
// Every geometry is asserted to meet the planner's acceptance test, and every product to fit int32 (the helper's precondition).
// Both forms of the helper run: the one that divides, and the one the kernel calls with the reciprocal it keeps (mrk::bm_cut_inv).
// Built and run by tests/test_bm_cut_cpu.py; no GPU, no libmrk.so.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_kcommon.h"
#include "../../manticoresearch_amd/csrc/mrk_sortkey.h"

static int g_bad = 0;
#define CHECK(c, ...)                                      \
  do {                                                     \
    if (!(c)) {                                            \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
      if (++g_bad > 20) exit(1);                           \
    }                                                      \
  } while (0)

static uint64_t g_s = 4242;
static uint64_t rnd() {
  g_s += 0x9E3779B97F4A7C15ull;
  uint64_t z = g_s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the parent kernel's test of a match word, verbatim
static bool parent_drops(int32_t bin_lo, uint32_t bin_shift, uint32_t tau_bin, uint32_t rmax1000, uint32_t index_weight, int32_t bmw) {
  uint32_t weight = (uint32_t)bmw + rmax1000;
  weight *= index_weight;
  return mrk::weight_bin(bin_lo, bin_shift, (int32_t)weight) < tau_bin;
}

struct Geo {
  int64_t bm_lo, bm_hi; // the range of x: bins_by_weight's bm_lo .. bm_hi
  int32_t w[3];         // field weights
  uint32_t iw;
};

static size_t g_n = 0, g_geos = 0, g_neg_T = 0, g_neg_lo = 0;

static void check_geo(const Geo& g) {
  // bins_by_weight: the field-weight sum over every field mask (the empty mask counts 1), four corners, the acceptance test
  int64_t rmin = INT64_MAX, rmax = INT64_MIN;
  for (uint32_t m = 0; m < 8; ++m) {
    int64_t r = 0;
    if (!m) r = 1;
    for (uint32_t f = 0; f < 3; ++f)
      if (m & (1u << f)) r += g.w[f];
    rmin = std::min(rmin, r), rmax = std::max(rmax, r);
  }
  const int64_t iw = g.iw;
  const int64_t c[4] = {(g.bm_lo + rmin * 1000) * iw, (g.bm_lo + rmax * 1000) * iw, (g.bm_hi + rmin * 1000) * iw, (g.bm_hi + rmax * 1000) * iw};
  const int64_t wlo = *std::min_element(c, c + 4), whi = *std::max_element(c, c + 4);
  const bool accepted = wlo > INT32_MIN && whi < INT32_MAX && llabs(rmin) < INT32_MAX / 1000 && llabs(rmax) < INT32_MAX / 1000 && (int32_t)g.iw > 0;
  CHECK(accepted, "geometry bm %lld..%lld weights %d %d %d iw %u: the planner would fall back (%lld..%lld)", (long long)g.bm_lo, (long long)g.bm_hi, g.w[0],
        g.w[1], g.w[2], g.iw, (long long)wlo, (long long)whi);
  if (!accepted) return;
  const int32_t lo = (int32_t)wlo;
  uint32_t plan_shift = 0;
  while (plan_shift < 31 && ((uint64_t)(whi - wlo) >> plan_shift) >= 1024u) ++plan_shift;
  CHECK(plan_shift <= 22u, "shift %u", plan_shift);
  // the kernel's rmax1000: every field with a positive weight
  uint32_t rmax1000 = 0;
  for (uint32_t f = 0; f < 3; ++f) rmax1000 += g.w[f] > 0 ? (uint32_t)g.w[f] : 0u;
  rmax1000 *= 1000u;
  CHECK((int64_t)rmax1000 >= rmin * 1000 && (int64_t)rmax1000 <= rmax * 1000, "rmax1000 %u outside %lld..%lld", rmax1000, (long long)rmin, (long long)rmax);
  ++g_geos;
  if (lo < 0) ++g_neg_lo;
  const uint32_t inv = mrk::bm_cut_inv(g.iw);
  const uint32_t taus[] = {0u, 1u, 2u, 511u, 1022u, 1023u};
  for (uint32_t sh = 0; sh <= 23u; ++sh) {
    const uint32_t shift = sh == 23u ? plan_shift : sh; // (the planner's own once more, whatever it is)
    for (uint32_t tau : taus) {
      const int32_t cut = mrk::bm_wmax_cut(lo, shift, tau, rmax1000, g.iw);
      const int32_t cut_k = mrk::bm_wmax_cut(lo, shift, tau, rmax1000, g.iw, inv);
      CHECK(cut == cut_k, "lo %d shift %u tau %u iw %u: cutoff %d, with the kept reciprocal %d", lo, shift, tau, g.iw, cut, cut_k);
      if (tau == 0) CHECK(cut == INT32_MIN, "tau 0: cutoff %d", cut);
      if (tau && (int64_t)lo + ((int64_t)tau << shift) <= 0) ++g_neg_T;
      std::vector<int64_t> xs;
      for (int d = -3; d <= 3; ++d) xs.push_back((int64_t)cut + d);
      for (int d = 0; d <= 3; ++d) xs.push_back(g.bm_lo + d), xs.push_back(g.bm_hi - d);
      for (int i = 0; i < 24; ++i) xs.push_back(g.bm_lo + (int64_t)(rnd() % (uint64_t)(g.bm_hi - g.bm_lo + 1)));
      for (int64_t x : xs) {
        if (x < g.bm_lo || x > g.bm_hi) continue; // (the cutoff's neighbours outside the reachable range: the product may wrap there)
        const int64_t w = (x + (int64_t)rmax1000) * iw;
        CHECK(w > INT32_MIN && w < INT32_MAX, "x %lld: weight %lld does not fit", (long long)x, (long long)w);
        const bool want = parent_drops(lo, shift, tau, rmax1000, g.iw, (int32_t)x);
        const bool got = (int32_t)x < cut;
        CHECK(want == got, "lo %d shift %u tau %u rmax1000 %u iw %u x %lld: parent %d, cutoff %d says %d", lo, shift, tau, rmax1000, g.iw, (long long)x,
              (int)want, cut, (int)got);
        ++g_n;
      }
    }
  }
}

int main() {
  const uint32_t iws[] = {1u, 2u, 3u, 7u, 1000u, 65535u};
  const int32_t wsets[][3] = {{1, 1, 1}, {3, -2, 0}, {0, 0, 0}, {-1, -4, -2}, {10, 0, -7}, {100, 50, 1}, {-30, 2, 0}};
  const double idfs[] = {-0.4, -0.05, 0.0, 1e-3, 0.19, 0.5, 0.7, 3.9};
  // 1. the planner's own estimate of the float sum's range, for pairs of idfs (pure AND: every keyword contributes)
  for (uint32_t iw : iws)
    for (const auto& ws : wsets)
      for (double ia : idfs)
        for (double ib : idfs) {
          const double lo = std::min(ia / 2.2, ia) + std::min(ib / 2.2, ib), hi = std::max(ia / 2.2, ia) + std::max(ib / 2.2, ib);
          Geo g = {(int64_t)floor((lo + 0.5) * 1000.0) - 2, (int64_t)ceil((hi + 0.5) * 1000.0) + 2, {ws[0], ws[1], ws[2]}, iw};
          // (a field weight of 100 at index weight 65535 leaves int32: there the planner falls back and the kernel does not prune)
          const int64_t top = (g.bm_hi + 1000 * (int64_t)(std::max(ws[0], 0) + std::max(ws[1], 0) + std::max(ws[2], 0) + 1)) * (int64_t)iw;
          const int64_t bot = (g.bm_lo + 1000 * (int64_t)(std::min(ws[0], 0) + std::min(ws[1], 0) + std::min(ws[2], 0))) * (int64_t)iw;
          if (top >= INT32_MAX || bot <= INT32_MIN) continue;
          check_geo(g);
        }
  // 2. ranges of x that push bin_lo and the top weight up against the int32 ends the planner still accepts
  for (uint32_t iw : iws)
    for (const auto& ws : wsets) {
      int64_t rmin = 0, rmax = 1; // as check_geo finds them
      for (uint32_t m = 1; m < 8; ++m) {
        int64_t r = 0;
        for (uint32_t f = 0; f < 3; ++f)
          if (m & (1u << f)) r += ws[f];
        rmin = std::min(rmin, r), rmax = std::max(rmax, r);
      }
      rmin = std::min<int64_t>(rmin, 1);
      const int64_t xhi = ((int64_t)INT32_MAX - 1) / (int64_t)iw - rmax * 1000; // (xhi + rmax * 1000) * iw <= INT32_MAX - 1
      const int64_t xlo = -(((int64_t)INT32_MAX) / (int64_t)iw) - rmin * 1000;   // (xlo + rmin * 1000) * iw >= -INT32_MAX
      if (xhi - xlo < 5000) continue; // (no range of x left: the planner falls back for every pair of keywords)
      check_geo(Geo{xlo, xhi, {ws[0], ws[1], ws[2]}, iw});
      check_geo(Geo{xlo, xlo + 5000, {ws[0], ws[1], ws[2]}, iw});
      check_geo(Geo{xhi - 5000, xhi, {ws[0], ws[1], ws[2]}, iw});
      if (xlo <= -3 && xhi >= 3) check_geo(Geo{-3, 3, {ws[0], ws[1], ws[2]}, iw}); // (field weights of 100 at index weight 65535 leave no such range)
    }
  printf("compared %zu geometries %zu lo<0 %zu T<=0 %zu\n", g_n, g_geos, g_neg_lo, g_neg_T);
  CHECK(g_neg_lo > 0 && g_neg_T > 0, "no geometry with a negative bin_lo / T");
  if (g_bad) return 1;
  printf("ok\n");
  return 0;
}
