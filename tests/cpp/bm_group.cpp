// bm_group.cpp -- the planner's grouping of scan_bm queries (mrk::plan_bm_groups, csrc/mrk_plan.cpp) on the CPU.
// Random batches over a few keywords and classes: every member lands in exactly one group, no group exceeds BM_GROUP_MAX,
// a group's members are of one class and all hold one keyword (so it needs at most BM_GROUP_TABS tfidf tables), a member
// whose keys no other member of its class holds is alone, and the same input gives the same groups.  Built and run by
// tests/test_bm_group_cpu.py; no GPU, no libmrk.so.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>

#include <set>
#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_host_int.h"

int mrk_fail(int code, const char*, ...) { return code; }
extern "C" const char* mrk_last_error(void) { return ""; }
extern "C" float mrk_idf(int64_t, int64_t, int, int, int, float) { return 0.0f; }

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_s += 0x9E3779B97F4A7C15ull;
  uint64_t z = g_s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      fprintf(stderr, "FAIL %s:%d: %s (iteration %d)\n", __FILE__, __LINE__, #c, it); \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

// `bm_group time`: microseconds per call for a bench-sized batch -- 256 members over 145 keys drawn Zipf-like, one class
static int timing() {
  std::vector<mrk::BmMember> m(256);
  std::vector<double> cdf(145);
  double acc = 0;
  for (int k = 0; k < 145; ++k) cdf[k] = acc += 1.0 / (k + 1);
  for (auto& x : m)
    for (int t = 0; t < 2; ++t) {
      const double u = (double)(rnd() >> 11) / 9007199254740992.0 * acc;
      uint64_t k = 0;
      while (k + 1 < 145 && cdf[k] < u) ++k;
      x.key[t] = k, x.bytes[t] = 12500000 + 1000 * (145 - k);
    }
  std::vector<uint32_t> order, sizes;
  const int reps = 2000;
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < reps; ++r) mrk::plan_bm_groups(m, order, sizes);
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
  size_t by[5] = {0, 0, 0, 0, 0};
  for (uint32_t sz : sizes) ++by[sz];
  printf("us_per_call %.2f groups1 %zu groups2 %zu groups3 %zu groups4 %zu\n", us, by[1], by[2], by[3], by[4]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "time")) return timing();
  const int iters = argc > 1 ? atoi(argv[1]) : 2000;
  size_t groups_total = 0, members_total = 0, singles = 0, full = 0;
  for (int it = 0; it < iters; ++it) {
    const uint32_t n = 1 + (uint32_t)(rnd() % (it % 4 == 0 ? 300 : 24));
    const uint32_t nkeys = 1 + (uint32_t)(rnd() % (it % 3 == 0 ? 200 : 12)), ncls = 1 + (uint32_t)(rnd() % 3);
    std::vector<mrk::BmMember> m(n);
    for (auto& x : m) {
      for (int t = 0; t < 2; ++t) {
        x.key[t] = rnd() % nkeys;
        x.bytes[t] = 1000 + x.key[t] * 37 % 500; // (a key's bytes do not depend on the member)
      }
      x.cls = (uint32_t)(rnd() % ncls);
    }
    std::vector<uint32_t> order, sizes, order2, sizes2;
    mrk::plan_bm_groups(m, order, sizes);
    mrk::plan_bm_groups(m, order2, sizes2);
    CHECK(order == order2 && sizes == sizes2); // deterministic
    CHECK(order.size() == n);
    std::vector<int> seen(n, 0);
    for (uint32_t i : order) CHECK(i < n && !seen[i]++); // each member exactly once
    size_t o = 0;
    for (uint32_t sz : sizes) {
      CHECK(sz >= 1 && sz <= (uint32_t)mrk::BM_GROUP_MAX);
      std::set<uint64_t> keys;
      for (uint32_t j = 0; j < sz; ++j) {
        const mrk::BmMember& x = m[order[o + j]];
        CHECK(x.cls == m[order[o]].cls);
        keys.insert(x.key[0]), keys.insert(x.key[1]);
      }
      if (sz > 1) { // one keyword held by every member: at most BM_GROUP_TABS distinct keys
        bool shared = false;
        for (uint64_t k : keys) {
          bool all = true;
          for (uint32_t j = 0; j < sz; ++j) all = all && (m[order[o + j]].key[0] == k || m[order[o + j]].key[1] == k);
          shared = shared || all;
        }
        CHECK(shared);
        CHECK(keys.size() <= (size_t)mrk::BM_GROUP_TABS);
      }
      if (sz == 1) ++singles;
      if (sz == (uint32_t)mrk::BM_GROUP_MAX) ++full;
      o += sz;
    }
    // a member whose keys no other member of its class holds is alone
    for (uint32_t i = 0; i < n; ++i) {
      bool shares = false;
      for (uint32_t j = 0; j < n; ++j)
        if (j != i && m[j].cls == m[i].cls)
          for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) shares = shares || m[i].key[a] == m[j].key[b];
      if (shares) continue;
      size_t oo = 0;
      for (uint32_t sz : sizes) {
        bool in = false;
        for (uint32_t j = 0; j < sz; ++j) in = in || order[oo + j] == i;
        if (in) CHECK(sz == 1);
        oo += sz;
      }
    }
    groups_total += sizes.size(), members_total += n;
  }
  // a hand-made batch: keyword 0 in seven members, the pair (1, 2) twice, (3, 4): groups of 4, 3, 2 and 1
  {
    const int it = -1;
    const uint64_t pairs[10][2] = {{0, 1}, {0, 2}, {0, 3}, {0, 5}, {0, 6}, {0, 7}, {0, 8}, {1, 2}, {2, 1}, {3, 4}};
    std::vector<mrk::BmMember> m(10);
    for (int i = 0; i < 10; ++i)
      for (int t = 0; t < 2; ++t) m[i].key[t] = pairs[i][t], m[i].bytes[t] = 1000;
    std::vector<uint32_t> order, sizes;
    mrk::plan_bm_groups(m, order, sizes);
    CHECK((sizes == std::vector<uint32_t>{4, 3, 2, 1}));
    CHECK(order[9] == 9);
  }
  printf("groups %zu members %zu singles %zu full %zu\n", groups_total, members_total, singles, full);
  return 0;
}
