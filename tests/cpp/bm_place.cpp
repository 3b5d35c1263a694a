// bm_place.cpp -- the dispatch order of a batch's scan_bm work items (mrk::place_bm_items, csrc/mrk_plan.cpp) on the CPU.
// Batches of two-keyword queries over dense keywords are laid out by mrk::layout_batch (bm_group 0 and 1) and placed under
// modes 0, 1 and 2.  Two sources: seeded random batches (1 to 300 queries over a pool of 2 to 60 keywords, several window
// counts, in a fifth of the batches window ranges of the queries' own, piece-major and query-major), and, from the file named in argv[1], the query sets of the benchmark (keyword ids and
// doc counts; tests/test_bm_place_cpu.py writes it from bench.make_queries).  Checked for every placement: disp is a
// permutation; mode 0 and fewer than two owners give the identity and no figures; the same input gives the same output; inside
// a class the items are dispatched by ascending blk_begin, then owner; an item sits in a slot of its owner's class unless that
// slot's class has run out; the keyword counts and bytes equal a count made here from the class assignment; the classes' bytes
// never exceed the owners'.  On the benchmark's sets: at most 8 % of the items outside their class's slots, and the classes'
// bytes at most 0.75 of the owners'.
// "time" as argv[2]: the cost per call on the benchmark's sets (built without sanitizers).
// Built and run by tests/test_bm_place_cpu.py; no GPU, no libmrk.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <set>
#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_host_int.h"

int mrk_fail(int code, const char*, ...) { return code; }
extern "C" const char* mrk_last_error(void) { return ""; }
extern "C" float mrk_idf(int64_t, int64_t, int, int, int, float) { return 0.0f; }

using mrk::BatchLayout;
using mrk::BatchPlan;
using mrk::BmGroup;
using mrk::BmPlacement;
using mrk::LayoutKnobs;

static uint64_t g_s;
static uint64_t rnd() {
  g_s += 0x9E3779B97F4A7C15ull;
  uint64_t z = g_s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
static bool chance(uint32_t pct) { return below(100) < pct; }

static char g_what[160] = "";
#define CHECK(c, ...)                                                  \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "FAIL %s:%d: %s [%s] ", __FILE__, __LINE__, #c, g_what); \
      fprintf(stderr, __VA_ARGS__);                                    \
      fprintf(stderr, "\n");                                           \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

struct Batch {
  std::vector<DevQuery> head;
  BatchPlan plan;
};

// a dense keyword: its bitmap, an idf that follows from its docs (one keyword = one key), its blocks
static DevTerm keyword(uint32_t id, uint64_t docs) {
  DevTerm t{};
  t.bm_off = (uint64_t)id * 1000003ull;
  t.idf = 1.0f / (float)(docs + 1);
  t.docs = (uint32_t)docs;
  t.nblocks = (uint32_t)((docs + 127) / 128);
  return t;
}

static void add_query(Batch& B, const DevTerm& a, const DevTerm& b, uint32_t nwin, uint32_t wclass) {
  static const int32_t wtab[2][8] = {{1, 1, 1, 1, 1, 1, 1, 1}, {3, 1, 2, 1, 1, 5, 1, 1}};
  DevQuery Q;
  memset(&Q, 0, sizeof Q);
  const uint32_t i = (uint32_t)B.head.size();
  Q.out_q = i;
  Q.tree_flags = mrk::TF_MULTIAND | mrk::TF_BITMAP;
  Q.ranker = MRK_RANK_BM25;
  Q.n_terms = 2;
  Q.t[0] = a.docs <= b.docs ? a : b, Q.t[1] = a.docs <= b.docs ? b : a;
  Q.n_weights = 8;
  memcpy(Q.weights, wtab[wclass], sizeof wtab[0]);
  Q.item_first = (uint32_t)B.plan.items_bm.size();
  Q.n_items = 1;
  DevItem it{};
  it.query = i, it.blk_end = nwin;
  B.plan.items_bm.push_back(it);
  B.head.push_back(Q);
}

static void random_batch(uint64_t seed, Batch& B) {
  g_s = 0xB17B17ull * (seed + 1);
  static const uint32_t windows[6] = {7, 74, 100, 611, 6104, 12207};
  const uint32_t nwin = windows[below(6)];
  const uint32_t n = chance(15) ? 1 + below(3) : 1 + below(300);
  const uint32_t npool = 2 + below(59);
  std::vector<DevTerm> pool;
  for (uint32_t k = 0; k < npool; ++k) pool.push_back(keyword(k, 1000 + rnd() % 3000000));
  B = Batch{};
  const bool own_ranges = chance(20); // window ranges of the queries' own (a rowid limit): many piece counts in one section
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t a = below(npool), b = below(npool);
    if (chance(40)) a = below(std::min(npool, 4u)); // (a few hot keywords)
    add_query(B, pool[a], pool[b], own_ranges ? 1 + below(nwin) / 7 * 7 : nwin, chance(85) ? 0 : 1);
  }
}

struct Figures {
  size_t items = 0, tail = 0;
  uint64_t owner_bytes = 0, class_bytes = 0;
  bool ran = false;
};

// one placement of a laid-out batch, checked
static Figures check_place(const Batch& B, const BatchLayout& L, bool nib, int mode) {
  const uint32_t n = (uint32_t)B.head.size();
  BmPlacement P, P2;
  mrk::place_bm_items(B.head.data(), n, B.plan.extra, L, nib, mode, P);
  P2.disp.assign(7, 99u), P2.owner_class.assign(3, 5), P2.owner_keys = 77, P2.ran = true; // (a used object: everything is rewritten)
  mrk::place_bm_items(B.head.data(), n, B.plan.extra, L, nib, mode, P2);
  CHECK(!P.mismatch && !P2.mismatch, "the ranges of the layout do not add up to its items");
  CHECK(P.disp == P2.disp && P.owner_class == P2.owner_class && P.owner_pass == P2.owner_pass && P.owner_keys == P2.owner_keys && P.class_keys == P2.class_keys &&
            P.owner_bytes == P2.owner_bytes && P.class_bytes == P2.class_bytes && P.ran == P2.ran,
        "the same section placed differently the second time");
  const size_t n0 = L.n_items_kind[0];
  const DevItem* it = L.items.data() + L.n_items_pk;
  Figures F;
  F.items = n0, F.ran = P.ran;
  // ---- a permutation
  CHECK(P.disp.size() == n0, "disp holds %zu entries for %zu items", P.disp.size(), n0);
  std::vector<uint8_t> seen(n0, 0);
  for (size_t i = 0; i < n0; ++i) {
    CHECK(P.disp[i] < n0 && !seen[P.disp[i]], "slot %zu runs item %u (out of range, or twice)", i, P.disp[i]);
    seen[P.disp[i]] = 1;
  }
  // ---- owners, as this test sees them
  const bool grouped = !L.groups.empty();
  std::map<uint32_t, uint32_t> own_of; // item.query -> owner: the group; ungrouped, the place the function gave the pass in owner_pass
  if (!grouped) {
    std::set<uint32_t> once(P.owner_pass.begin(), P.owner_pass.end());
    CHECK(once.size() == P.owner_pass.size(), "owner_pass names a pass twice");
  }
  for (size_t i = 0; i < n0; ++i)
    if (!own_of.count(it[i].query)) {
      uint32_t o = it[i].query;
      if (!grouped) {
        o = (uint32_t)(std::find(P.owner_pass.begin(), P.owner_pass.end(), it[i].query) - P.owner_pass.begin());
        CHECK(o < P.owner_pass.size(), "pass %u has items and is no owner", it[i].query);
      }
      own_of[it[i].query] = o;
    }
  const size_t n_owners = own_of.size();
  if (mode == 0 || n_owners < 2) {
    for (size_t i = 0; i < n0; ++i) CHECK(P.disp[i] == i, "identity expected, slot %zu runs %u", i, P.disp[i]);
    CHECK(!P.ran && !P.owner_keys && !P.class_keys && !P.owner_bytes && !P.class_bytes, "figures without a placement");
    return F;
  }
  CHECK(P.ran, "%zu owners and no placement", n_owners);
  CHECK(P.owner_class.size() == (grouped ? L.groups.size() : P.owner_pass.size()), "owner_class holds %zu entries", P.owner_class.size());
  const uint32_t n_cls = mode == 1 ? mrk::PLACE_CLASSES : 1;
  for (const auto& o : own_of) CHECK(P.owner_class[o.second] < n_cls, "owner %u in class %u", o.second, P.owner_class[o.second]);
  // ---- the figures, counted here: an owner's keywords, a keyword's bytes (the largest of its holders'), the classes' distinct keywords
  typedef std::pair<uint64_t, uint32_t> Key;
  auto key_of = [](const DevTerm& T) {
    uint32_t idf;
    memcpy(&idf, &T.idf, 4);
    return Key(T.bm_off, idf);
  };
  std::map<uint32_t, std::set<Key>> okeys; // by owner
  std::map<Key, uint64_t> kbytes;
  for (const auto& o : own_of) {
    uint32_t lo = ~0u, hi = 0;
    for (size_t i = 0; i < n0; ++i)
      if (it[i].query == o.first) lo = std::min(lo, it[i].blk_begin), hi = std::max(hi, it[i].blk_end);
    std::vector<uint32_t> passes;
    if (grouped)
      for (uint32_t j = 0; j < L.groups[o.first].n; ++j) passes.push_back(L.groups[o.first].q[j]);
    else
      passes.push_back(o.first);
    for (uint32_t p : passes)
      for (int t = 0; t < 2; ++t) {
        const DevTerm& T = B.head[p].t[t];
        okeys[o.second].insert(key_of(T));
        uint64_t& kb = kbytes[key_of(T)];
        kb = std::max(kb, (uint64_t)(hi - lo) * 256 + (uint64_t)T.nblocks * (nib ? 128 : 256));
      }
  }
  std::vector<std::set<Key>> ckeys(n_cls);
  uint64_t n_okeys = 0, n_ckeys = 0;
  for (const auto& o : okeys) {
    n_okeys += o.second.size();
    for (const Key& k : o.second) F.owner_bytes += kbytes[k], ckeys[P.owner_class[o.first]].insert(k);
  }
  for (const auto& c : ckeys) {
    n_ckeys += c.size();
    for (const Key& k : c) F.class_bytes += kbytes[k];
  }
  CHECK(P.owner_keys == n_okeys && P.class_keys == n_ckeys, "keys: (owner, keyword) %u, counted %llu; (class, keyword) %u, counted %llu", P.owner_keys,
        (unsigned long long)n_okeys, P.class_keys, (unsigned long long)n_ckeys);
  CHECK(P.owner_bytes == F.owner_bytes && P.class_bytes == F.class_bytes, "bytes: owners %llu, counted %llu; classes %llu, counted %llu",
        (unsigned long long)P.owner_bytes, (unsigned long long)F.owner_bytes, (unsigned long long)P.class_bytes, (unsigned long long)F.class_bytes);
  CHECK(F.class_bytes <= F.owner_bytes, "the classes hold more bytes than the owners");
  // ---- inside a class: ascending blk_begin, then owner; slots: the owner's class, unless the slot's class has run out
  std::vector<size_t> cls_items(n_cls, 0), cls_done(n_cls, 0);
  for (size_t i = 0; i < n0; ++i) ++cls_items[P.owner_class[own_of[it[i].query]]];
  std::vector<int64_t> last_begin(n_cls, -1), last_owner(n_cls, -1);
  for (size_t i = 0; i < n0; ++i) {
    const DevItem& x = it[P.disp[i]];
    const uint32_t o = own_of[x.query], c = P.owner_class[o];
    CHECK((int64_t)x.blk_begin > last_begin[c] || ((int64_t)x.blk_begin == last_begin[c] && (int64_t)o > last_owner[c]),
          "slot %zu: class %u runs [%u, owner %u) after [%lld, owner %lld)", i, c, x.blk_begin, o, (long long)last_begin[c], (long long)last_owner[c]);
    last_begin[c] = x.blk_begin, last_owner[c] = o;
    const uint32_t slot_cls = (uint32_t)(i % n_cls);
    if (c != slot_cls) {
      CHECK(cls_done[slot_cls] == cls_items[slot_cls], "slot %zu of class %u runs an item of class %u while class %u has %zu items left", i, slot_cls, c, slot_cls,
            cls_items[slot_cls] - cls_done[slot_cls]);
      for (uint32_t d = 0; d < n_cls; ++d)
        CHECK(cls_items[d] - cls_done[d] <= cls_items[c] - cls_done[c], "slot %zu: class %u has more items left than class %u", i, d, c);
      ++F.tail;
    }
    ++cls_done[c];
  }
  return F;
}

static void check_batch(Batch& B0, const LayoutKnobs& K, bool nib, bool bench_set, size_t stats[4]) {
  Batch B = B0;
  BatchLayout L;
  mrk::layout_batch(B.head.data(), (uint32_t)B.head.size(), B.plan, true, nib, K, L);
  const size_t what_len = strlen(g_what);
  for (int mode = 0; mode < 3; ++mode) {
    snprintf(g_what + what_len, sizeof g_what - what_len, " mode %d", mode);
    const Figures F = check_place(B, L, nib, mode);
    if (mode == 1 && F.ran) {
      ++stats[0], stats[1] += F.items, stats[2] += F.tail;
      if (F.class_bytes < F.owner_bytes) ++stats[3];
      if (bench_set) {
        printf("set%s items %zu tail %zu (%.2f %%) owner_bytes %llu class_bytes %llu ratio %.3f\n", g_what, F.items, F.tail, 100.0 * F.tail / F.items,
               (unsigned long long)F.owner_bytes, (unsigned long long)F.class_bytes, (double)F.class_bytes / (double)F.owner_bytes);
        CHECK(F.tail * 100 <= F.items * 8, "%zu of %zu items outside their class's slots", F.tail, F.items);
        CHECK((double)F.class_bytes <= 0.75 * (double)F.owner_bytes, "classes %llu B, owners %llu B", (unsigned long long)F.class_bytes, (unsigned long long)F.owner_bytes);
      }
    }
    g_what[what_len] = 0;
  }
}

static LayoutKnobs default_knobs() {
  LayoutKnobs K{};
  K.pk_min_items = 2048, K.item_order = 7, K.bm_target_items = 1 << 20, K.bm_min_windows = 256, K.bt_target_items = 6144, K.bm_group = 1, K.mq_max_chunks = 1 << 22;
  return K;
}

// the benchmark's sets: "nwin N" then per set "set Q" and Q lines "id_a docs_a id_b docs_b"
static std::vector<Batch> read_sets(const char* path) {
  std::vector<Batch> sets;
  FILE* f = fopen(path, "r");
  CHECK(f, "cannot open %s", path);
  unsigned nwin = 0, q = 0;
  CHECK(fscanf(f, " nwin %u", &nwin) == 1 && nwin, "no window count in %s", path);
  while (fscanf(f, " set %u", &q) == 1) {
    sets.emplace_back();
    for (unsigned i = 0; i < q; ++i) {
      unsigned ia, ib;
      unsigned long long da, db;
      CHECK(fscanf(f, " %u %llu %u %llu", &ia, &da, &ib, &db) == 4, "set %zu query %u", sets.size() - 1, i);
      add_query(sets.back(), keyword(ia, da), keyword(ib, db), nwin, 0);
    }
  }
  fclose(f);
  return sets;
}

int main(int argc, char** argv) {
  CHECK(argc > 1, "usage: bm_place SETS_FILE [BATCHES | time]");
  std::vector<Batch> sets = read_sets(argv[1]);
  if (argc > 2 && !strcmp(argv[2], "time")) {
    // per call, over the sets in turn: the layout, and the placement in each mode
    const LayoutKnobs K = default_knobs();
    std::vector<BatchLayout> L(sets.size());
    std::vector<Batch> B = sets;
    const int rounds = 20;
    double lay_us = 0, us[3] = {0, 0, 0};
    size_t items = 0;
    for (int r = 0; r < rounds; ++r)
      for (size_t s = 0; s < sets.size(); ++s) {
        B[s] = sets[s];
        const auto t0 = std::chrono::steady_clock::now();
        mrk::layout_batch(B[s].head.data(), (uint32_t)B[s].head.size(), B[s].plan, true, false, K, L[s]);
        lay_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        items = L[s].n_items_kind[0];
      }
    BmPlacement P;
    for (int mode = 0; mode < 3; ++mode)
      for (int r = 0; r < rounds; ++r)
        for (size_t s = 0; s < sets.size(); ++s) {
          const auto t0 = std::chrono::steady_clock::now();
          mrk::place_bm_items(B[s].head.data(), (uint32_t)B[s].head.size(), B[s].plan.extra, L[s], false, mode, P);
          us[mode] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        }
    const double calls = (double)rounds * (double)sets.size();
    printf("us_per_call layout %.1f place0 %.1f place1 %.1f place2 %.1f items %zu\n", lay_us / calls, us[0] / calls, us[1] / calls, us[2] / calls, items);
    return 0;
  }
  size_t stats[4] = {0, 0, 0, 0}; // placements with classes, their items, of those outside their class's slots, placements that saved bytes
  for (size_t s = 0; s < sets.size(); ++s)
    for (int group = 0; group < 2; ++group)
      for (int minw = 256; minw >= 128; minw /= 2) { // the context's item length, and the one the issue's figures were modelled at
        LayoutKnobs K = default_knobs();
        K.bm_group = group, K.bm_min_windows = minw;
        snprintf(g_what, sizeof g_what, "bench set %zu bm_group %d bm_min_windows %d", s, group, minw);
        check_batch(sets[s], K, false, group == 1, stats);
      }
  const int batches = argc > 2 ? atoi(argv[2]) : 200;
  for (int s = 0; s < batches; ++s) {
    Batch B0;
    random_batch((uint64_t)s, B0);
    for (int group = 0; group < 2; ++group)
      for (int alt = 0; alt < 3; ++alt) {
        LayoutKnobs K = default_knobs();
        K.bm_group = group;
        if (alt == 1) K.bm_min_windows = 16; // short pieces
        if (alt == 2) K.item_order = 5, K.bm_min_windows = 70; // query-major (and no groups: the grouped layout is piece-major only)
        snprintf(g_what, sizeof g_what, "batch %d bm_group %d alt %d", s, group, alt);
        check_batch(B0, K, (s & 1) != 0, false, stats);
      }
  }
  printf("ok placements %zu items %zu tail %zu saved %zu\n", stats[0], stats[1], stats[2], stats[3]);
  return 0;
}
