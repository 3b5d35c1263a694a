// group_table.cpp -- the group table's hash, probe sequence and slot claim (csrc/mrk_kgroup.h: the very functions the kernels' emit
// points call, with the sequential GroupSeqOps policy instead of device atomics) on the CPU under AddressSanitizer + UBSan.  The table
// lives in a heap block of its EXACT size (group_table_words), so a probe or a count one slot past the end is a sanitizer report.
//   - keys 0 and 0xFFFFFFFF are ordinary keys; an empty table claims nothing
//   - keys that collide, and a probe run that wraps round the table's end
//   - exactly 4 K distinct keys: all answered, claimed == 4 K; the 4 K + 1st: still stored (the table has room), claimed == 4 K + 1,
//     which is what group_select_kernel declines on
//   - a full table: the probe for one more key ends after `slots` steps with false and changes nothing
//   - count and head of every key against a std::map, over random streams with repeats
//   - the slot count per K (K = 20 -> 256), group_order_key against a comparator written from the order's definition
// It also prints, for the GPU test's value generator (tests/group_expect.py: seeded_values), which seeds give a collision and a
// wrap-around at K = 1 and K = 2: lines "SEED k=<K> collide=<seed> wrap=<seed>", which tests/test_group_cpu.py compares with the seeds
// tests/test_gpu_group.py names.
// Built and run by tests/test_group_cpu.py; no GPU, no libmrk.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include <hip/hip_runtime.h> // (the function qualifiers of mrk_kgroup.h; no HIP call is made)

#include "../../manticoresearch_amd/csrc/mrk_kgroup.h"

using namespace mrk;

static int g_bad = 0;
#define CHECK(c, ...)                                 \
  do {                                                \
    if (!(c)) {                                       \
      if (g_bad < 50) {                               \
        printf("FAIL %s:%d: ", __FILE__, __LINE__);   \
        printf(__VA_ARGS__);                          \
        printf("\n");                                 \
      }                                               \
      ++g_bad;                                        \
    }                                                 \
  } while (0)

struct Table {
  uint64_t* mem;
  GroupTable T;
  explicit Table(uint32_t slots) {
    const size_t words = (size_t)group_table_words(slots);
    mem = (uint64_t*)calloc(words, 8); // exact size
    T = group_table_at(mem, slots);
  }
  ~Table() { free(mem); }
  bool push(uint32_t v, uint32_t count, uint64_t head) { return group_update<GroupSeqOps>(T, v, count, head); }
  // the slot that holds v, or -1
  int find(uint32_t v) const {
    for (uint32_t i = 0; i < T.slots; ++i)
      if (T.keys[i] == (GRP_TAG | v)) return (int)i;
    return -1;
  }
};

// the GPU test's value generator: the j-th of a seed's distinct values (tests/group_expect.py restates it)
static uint32_t seeded_value(uint32_t seed, uint32_t j) {
  uint32_t x = seed * 0x9E3779B1u + j * 0x85EBCA6Bu + 0x165667B1u;
  x ^= x >> 16, x *= 0x7FEB352Du, x ^= x >> 15, x *= 0x846CA68Bu, x ^= x >> 16;
  return x;
}

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}

static void against_map(uint32_t K, uint32_t n_keys, uint32_t n_push) {
  const uint32_t S = group_slots_for(K);
  Table t(S);
  std::vector<uint32_t> keys;
  while (keys.size() < n_keys) {
    const uint32_t v = keys.empty() ? 0u : keys.size() == 1 ? 0xFFFFFFFFu : (uint32_t)rnd();
    if (std::find(keys.begin(), keys.end(), v) == keys.end()) keys.push_back(v);
  }
  std::map<uint32_t, std::pair<uint64_t, uint64_t>> want; // value -> (count, head)
  uint32_t row = 0;
  auto one = [&](uint32_t v) {
    const uint32_t cnt = 1 + (uint32_t)(rnd() % 3);
    const uint64_t head = make_key((int32_t)(rnd() % 7) - 3, row++);
    const bool ok = t.push(v, cnt, head);
    if (ok) {
      auto& w = want[v];
      w.first += cnt, w.second = std::max(w.second, head);
    }
    return ok;
  };
  for (uint32_t v : keys) CHECK(one(v), "K %u: first sight of key %u refused", K, v);
  for (uint32_t i = 0; i < n_push; ++i) one(keys[rnd() % keys.size()]);
  CHECK(*t.T.claimed == n_keys, "K %u: claimed %u, distinct %u", K, *t.T.claimed, n_keys);
  uint32_t occupied = 0;
  for (uint32_t i = 0; i < S; ++i)
    if (t.T.keys[i]) {
      ++occupied;
      CHECK((t.T.keys[i] & GRP_TAG) != 0, "untagged key word");
      const uint32_t v = (uint32_t)t.T.keys[i];
      auto it = want.find(v);
      CHECK(it != want.end(), "slot holds %u, never pushed", v);
      if (it != want.end()) CHECK(t.T.counts[i] == it->second.first && t.T.heads[i] == it->second.second, "K %u value %u: count %u head %llx", K, v, t.T.counts[i], (unsigned long long)t.T.heads[i]);
    } else
      CHECK(t.T.counts[i] == 0 && t.T.heads[i] == 0, "an empty slot was written");
  CHECK(occupied == n_keys && want.size() == n_keys, "occupied %u", occupied);
}

int main() {
  // slot counts
  CHECK(group_slots_for(1) == 16 && group_slots_for(2) == 32 && group_slots_for(4) == 64 && group_slots_for(20) == 256 && group_slots_for(1000) == 8192 && group_slots_for(1024) == 16384, "slots per K");
  for (uint32_t k = 1; k <= MRK_MAX_K; ++k) {
    const uint32_t s = group_slots_for(k);
    CHECK((s & (s - 1)) == 0 && s >= 2 * (4 * k + 1) && (s == 8 || s / 2 < 2 * (4 * k + 1)), "slots %u for K %u", s, k);
  }
  CHECK(group_limit(1024) == GRP_MAX_GROUPS, "the selection kernel's LDS holds the largest limit");
  for (uint32_t s = 8; s <= 8192; s <<= 1)
    for (uint32_t i = 0; i < 1000; ++i) CHECK(group_hash((uint32_t)rnd(), s) < s, "hash outside the table");

  { // an untouched table; 0 and 0xFFFFFFFF
    Table t(16);
    CHECK(*t.T.claimed == 0, "fresh table");
    CHECK(t.push(0u, 1, make_key(1, 7)) && t.push(0xFFFFFFFFu, 1, make_key(1, 9)) && t.push(0u, 2, make_key(1, 3)), "push");
    CHECK(*t.T.claimed == 2, "claimed %u", *t.T.claimed);
    const int a = t.find(0u), b = t.find(0xFFFFFFFFu);
    CHECK(a >= 0 && b >= 0 && a != b, "0 and 0xFFFFFFFF are ordinary keys");
    if (a >= 0 && b >= 0) {
      CHECK(t.T.counts[a] == 3 && t.T.heads[a] == make_key(1, 3), "key 0: count %u", t.T.counts[a]); // equal weights: the lower rowid is the head
      CHECK(t.T.counts[b] == 1 && t.T.heads[b] == make_key(1, 9), "key ~0");
    }
  }
  { // collisions and the wrap round the end: keys that hash to the LAST slot
    const uint32_t S = 16;
    Table t(S);
    std::vector<uint32_t> last;
    for (uint32_t v = 1; last.size() < 3; ++v)
      if (group_hash(v, S) == S - 1) last.push_back(v);
    for (uint32_t v : last) CHECK(t.push(v, 1, make_key(5, v)), "push");
    CHECK(t.find(last[0]) == (int)S - 1 && t.find(last[1]) == 0 && t.find(last[2]) == 1, "wrap: slots %d %d %d", t.find(last[0]), t.find(last[1]), t.find(last[2]));
    CHECK(t.push(last[2], 4, make_key(6, 1)), "found again behind the wrap");
    CHECK(t.T.counts[1] == 5 && t.T.heads[1] == make_key(6, 1) && *t.T.claimed == 3, "count behind the wrap");
  }
  { // a full table: S keys fill it, one more probes S slots and gives up; nothing changes
    const uint32_t S = 16;
    Table t(S);
    for (uint32_t v = 0; v < S; ++v) CHECK(t.push(v * 977u, 1, make_key(1, v)), "fill");
    CHECK(*t.T.claimed == S, "full: claimed %u", *t.T.claimed);
    std::vector<uint64_t> before(t.mem, t.mem + group_table_words(S));
    CHECK(!t.push(0xABCDEF01u, 1, make_key(9, 0)), "a full table accepted a new key");
    CHECK(!memcmp(before.data(), t.mem, before.size() * 8), "a refused push changed the table");
    CHECK(t.push(5 * 977u, 1, make_key(0, 0)), "a key the full table holds");
  }
  // the limit: 4 K (answered), 4 K + 1 (the counter says so; the table still holds every key)
  for (uint32_t K : {1u, 2u, 4u, 20u, 1024u}) {
    against_map(K, 4 * K, 20 * K + 50);
    against_map(K, 4 * K + 1, 20 * K + 50);
    against_map(K, 1, 300);
  }
  // the groups' order: key vs a comparator from the definition
  {
    struct G { uint32_t v, c; int32_t w; uint32_t row; };
    std::vector<G> gs;
    const uint32_t vals[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    const int32_t ws[] = {-5, 0, 1, 1000};
    uint32_t row = 0;
    for (uint32_t v : vals)
      for (uint32_t c : {1u, 2u, 0xFFFFFFFFu})
        for (int32_t w : ws) gs.push_back(G{v, c, w, (row += 7)});
    for (uint32_t by = 0; by < 3; ++by)
      for (uint32_t desc = 0; desc < 2; ++desc)
        for (const G& a : gs)
          for (const G& b : gs) {
            if (&a == &b) continue;
            const int64_t pa = by == MRK_GROUPSORT_KEY ? (int64_t)a.v : by == MRK_GROUPSORT_COUNT ? (int64_t)a.c : (int64_t)a.w;
            const int64_t pb = by == MRK_GROUPSORT_KEY ? (int64_t)b.v : by == MRK_GROUPSORT_COUNT ? (int64_t)b.c : (int64_t)b.w;
            const bool a_first = pa != pb ? (desc ? pa > pb : pa < pb) : a.row < b.row;
            const uint64_t ka = group_order_key(by, desc, a.v, a.c, make_key(a.w, a.row)), kb = group_order_key(by, desc, b.v, b.c, make_key(b.w, b.row));
            CHECK((ka > kb) == a_first, "order by %u desc %u", by, desc);
          }
  }
  // seeds of the GPU test's generator that reach a collision and a wrap-around in the small tables
  for (uint32_t K : {1u, 2u}) {
    const uint32_t S = group_slots_for(K), n = 4 * K;
    int collide = -1, wrap = -1;
    for (uint32_t seed = 0; seed < 4096 && (collide < 0 || wrap < 0); ++seed) {
      Table t(S);
      bool c = false, w = false;
      for (uint32_t j = 0; j < n; ++j) {
        const uint32_t v = seeded_value(seed, j), home = group_hash(v, S);
        t.push(v, 1, make_key(1, j));
        const int at = t.find(v);
        if (at != (int)home) c = true;
        if (at >= 0 && (uint32_t)at < home) w = true;
      }
      if (c && collide < 0) collide = (int)seed;
      if (w && wrap < 0) wrap = (int)seed;
    }
    CHECK(collide >= 0 && wrap >= 0, "K %u: no seed below 4096 collides / wraps", K);
    printf("SEED k=%u collide=%d wrap=%d\n", K, collide, wrap);
  }
  if (g_bad) {
    printf("%d checks failed\n", g_bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
