// layout_cap.cpp -- the cap on a block-scan work item's length (LayoutKnobs::p2_max_blocks, mrk::layout_batch in csrc/mrk_plan.cpp:
// what mrk_batch_submit sets for launches on the lean block-scan instance) on the CPU.
// The seeded batches of layout.cpp (the generator below is a copy) are laid out with the cap at 0, 4, 8 and 16 under item_order 0 / 7,
// bm_group 0 / 1 and pk_min_items 0 / 2048 / above the item count.  That cap 0 gives the layout of the code without the member is
// NOT checked here: this program relies on tests/test_layout_cpu.py for it, which lays the same batches out with the member
// value-initialised (0) and compares with the digests recorded before the member existed (tests/golden/layout_digests.json).
// What is checked here is that a cap above every item's length gives the cap-0 layout element for element.  Under a cap: no block item is longer than it; the pieces of a pass cover its block range
// exactly once, in order, cut at multiples of T0_BLOCKS; the piece count written back to the pass is the number of its items;
// with both rules in force no piece is longer than under either alone; and the window-range sections are those of cap 0.
// Built and run by tests/test_layout_cap_cpu.py; no GPU, no libmrk.so.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_host_int.h"

int mrk_fail(int code, const char*, ...) { return code; }
extern "C" const char* mrk_last_error(void) { return ""; }
extern "C" float mrk_idf(int64_t, int64_t, int, int, int, float) { return 0.0f; }

using mrk::BatchLayout;
using mrk::BatchPlan;
using mrk::BmGroup;
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

static const char* g_what = "";
#define CHECK(c, ...)                                                  \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "FAIL %s:%d: %s [%s] ", __FILE__, __LINE__, #c, g_what); \
      fprintf(stderr, __VA_ARGS__);                                    \
      fprintf(stderr, "\n");                                           \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

static void fnv(uint64_t& h, const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
}

struct Range {
  uint32_t begin = 0, end = 0;
};

// one planned batch, as the plan loop of mrk_batch_submit leaves it
struct Batch {
  uint32_t n = 0;
  std::vector<DevQuery> head;
  BatchPlan plan;
  std::vector<Range> blocks; // per pass: the block range its block-scan items cover ({0, 0}: none)
  std::vector<DevTerm> pool; // keywords of the scan_bm pairs
};

static DevTerm pool_term(uint32_t k) {
  static const float idfs[3] = {0.125f, 0.0625f, 0.3f};
  DevTerm t{};
  t.bm_off = (uint64_t)(k / 2) * 4096; // (neighbours share a bitmap and differ in idf: two keys, two tfidf tables)
  t.idf = idfs[k % 2 + (k % 7 == 0)];
  t.nblocks = 1 + (uint32_t)(k * 2654435761u % 90000);
  t.docs = t.nblocks * 100;
  return t;
}

static void make_batch(uint64_t seed, Batch& B) {
  g_s = 0xC0FFEEull * (seed + 1);
  static const uint32_t windows[5] = {7, 100, 611, 6104, 48829};
  const uint32_t nwin = windows[below(5)];
  const uint32_t n = chance(25) ? 1 + below(4) : chance(40) ? 256 : 1 + below(256);
  const bool queue_fed = chance(40);
  const uint32_t mix = below(4); // 0: every kind, 1: mostly blocks, 2: mostly scan_bm, 3: mostly scan_bt
  B = Batch{};
  B.n = n;
  B.head.resize(n);
  const uint32_t npool = 2 + below(40);
  for (uint32_t k = 0; k < npool; ++k) B.pool.push_back(pool_term(k));
  static const int32_t wtab[2][8] = {{1, 1, 1, 1, 1, 1, 1, 1}, {3, 1, 2, 1, 1, 5, 1, 1}};
  auto ranked = [&](DevQuery& P) { // a ranker and flags that may send the pass's matches through a match queue
    P.ranker = MRK_RANK_BM25;
    if (!queue_fed || chance(50)) return;
    static const uint32_t rk[4] = {MRK_RANK_PROXIMITY_BM25, MRK_RANK_SPH04, MRK_RANK_WORDCOUNT, MRK_RANK_PROXIMITY};
    P.ranker = rk[below(4)];
  };
  auto block_items = [&](DevQuery& P, uint32_t pass, uint32_t kind) { // as plan_query cuts a driver's blocks
    const uint32_t nb0 = chance(5) ? 0 : 1 + below(chance(10) ? 12000 : 600), bpi = 4 * (1 + below(150));
    P.t[0].nblocks = nb0, P.t[0].docs = nb0 * 128 - (nb0 ? below(128) : 0);
    std::vector<DevItem>& to = kind == 2 ? B.plan.items_bm : B.plan.items;
    P.item_first = (uint32_t)to.size();
    P.n_items = 0;
    for (uint32_t b = 0; b < nb0; b += bpi) {
      DevItem it{};
      it.query = pass, it.blk_begin = b, it.blk_end = std::min(nb0, b + bpi), it.kind = kind;
      to.push_back(it);
      ++P.n_items;
    }
    if (kind != 2) B.blocks[pass] = Range{0, nb0};
  };
  // (B.blocks is indexed by pass: heads first, the further passes as they come)
  B.blocks.assign(n, Range{});
  for (uint32_t i = 0; i < n; ++i) {
    DevQuery& Q = B.head[i];
    memset(&Q, 0, sizeof Q);
    Q.out_q = i;
    Q.n_terms = 1 + below(4);
    for (uint32_t t = 1; t < Q.n_terms; ++t) Q.t[t].docs = 1 + below(3000000);
    uint32_t what = below(100);
    if (mix == 1) what = what < 85 ? 0 : what;
    if (mix == 2) what = what < 80 ? 50 : what;
    if (mix == 3) what = what < 70 ? 75 : what;
    if (what < 40) { // block scan, sometimes as several passes
      ranked(Q);
      if (queue_fed && chance(40)) Q.tree_flags |= chance(50) ? mrk::TF_PHRASE : mrk::TF_PHRASE_LEAF;
      block_items(Q, i, 0);
      const uint32_t more = chance(25) ? 1 + below(3) : 0;
      for (uint32_t p = 0; p < more; ++p) {
        DevQuery P = Q;
        B.blocks.push_back(Range{});
        const uint32_t pass = n + (uint32_t)B.plan.extra.size();
        if (chance(30)) { // a further pass on bitmap words
          P.tree_flags |= mrk::TF_BTREE | mrk::TF_MULTIAND;
          P.item_first = (uint32_t)B.plan.items_bm.size();
          P.n_items = 1;
          DevItem it{};
          it.query = pass, it.blk_end = nwin, it.kind = 1;
          B.plan.items_bm.push_back(it);
        } else
          block_items(P, pass, 0);
        B.plan.extra.push_back(P);
      }
    } else if (what < 70) { // scan_bm: two keywords of the pool
      Q.tree_flags = mrk::TF_MULTIAND | mrk::TF_BITMAP;
      Q.ranker = chance(80) ? MRK_RANK_BM25 : MRK_RANK_NONE;
      Q.n_terms = 2;
      uint32_t a = below(npool), b = below(npool);
      if (chance(60)) a = below(std::min(npool, 3u)); // (a few hot keywords: groups form)
      Q.t[0] = B.pool[a], Q.t[1] = B.pool[b];
      Q.n_weights = chance(70) ? 8 : 3;
      memcpy(Q.weights, wtab[chance(80) ? 0 : 1], sizeof wtab[0]);
      Q.item_first = (uint32_t)B.plan.items_bm.size();
      Q.n_items = 1;
      DevItem it{};
      it.query = i, it.blk_end = nwin;
      B.plan.items_bm.push_back(it);
    } else if (what < 85) { // scan_bt
      ranked(Q);
      Q.tree_flags = mrk::TF_BTREE | (chance(50) ? mrk::TF_MULTIAND : 0);
      Q.t[0].docs = 1 + below(5000000);
      Q.item_first = (uint32_t)B.plan.items_bm.size();
      Q.n_items = 1;
      DevItem it{};
      it.query = i, it.blk_end = nwin, it.kind = 1;
      B.plan.items_bm.push_back(it);
    } else if (what < 93 && queue_fed) { // the generic evaluator (its matches always travel through queue 2)
      Q.ranker = MRK_RANK_PROXIMITY_BM25;
      Q.tree_flags = mrk::TF_GEN;
      block_items(Q, i, 2);
    } else { // declined
      Q.n_items = 0, Q.n_terms = 0;
    }
  }
  B.plan.any_prox = queue_fed;
}

static bool same_item(const DevItem& a, const DevItem& b) { return a.query == b.query && a.blk_begin == b.blk_begin && a.blk_end == b.blk_end && a.kind == b.kind; }

struct Laid {
  Batch B;
  BatchLayout L;
};

static void lay_out(const Batch& B0, bool nibble, LayoutKnobs K, int cap, Laid& out) {
  K.p2_max_blocks = cap;
  out.B = B0;
  mrk::layout_batch(out.B.head.data(), out.B.n, out.B.plan, true, nibble, K, out.L);
}

static uint32_t pass_items(const Batch& B, uint32_t pass) { return pass < B.n ? B.head[pass].n_items : B.plan.extra[pass - B.n].n_items; }

// the block section of a capped layout against the batch as planned (B0) and the same knobs' layout without the cap (Z)
static void check_capped(const Batch& B0, const Laid& Z, const Laid& C, uint32_t cap, size_t& pieces) {
  const std::vector<DevItem>& it = C.L.items;
  const size_t npk = C.L.n_items_pk;
  CHECK(npk <= it.size() && npk >= Z.L.n_items_pk, "%zu block items under the cap, %zu without", npk, Z.L.n_items_pk);
  std::map<uint32_t, std::vector<DevItem>> by, by0;
  for (size_t i = 0; i < npk; ++i) {
    CHECK(it[i].kind == 0 && it[i].blk_end > it[i].blk_begin, "block item %zu: kind %u [%u, %u)", i, it[i].kind, it[i].blk_begin, it[i].blk_end);
    CHECK(it[i].blk_end - it[i].blk_begin <= cap, "block item %zu holds %u blocks under a cap of %u", i, it[i].blk_end - it[i].blk_begin, cap);
    by[it[i].query].push_back(it[i]);
  }
  for (size_t i = 0; i < Z.L.n_items_pk; ++i) by0[Z.L.items[i].query].push_back(Z.L.items[i]);
  for (uint32_t pass = 0; pass < (uint32_t)B0.blocks.size(); ++pass) {
    const Range w = B0.blocks[pass];
    if (w.begin == w.end) {
      CHECK(!by.count(pass), "pass %u has no blocks and %zu items", pass, by[pass].size());
      continue;
    }
    CHECK(by.count(pass), "pass %u has blocks [%u, %u) and no items", pass, w.begin, w.end);
    uint32_t at = w.begin, longest = 0, longest0 = 0;
    for (const DevItem& p : by[pass]) { // (in launch order: a pass's pieces ascend whatever the order of the passes)
      CHECK(p.blk_begin == at, "pass %u: piece [%u, %u) where %u was due", pass, p.blk_begin, p.blk_end, at);
      CHECK(p.blk_begin % mrk::T0_BLOCKS == 0 && ((p.blk_end - p.blk_begin) % mrk::T0_BLOCKS == 0 || p.blk_end == w.end), "pass %u: piece [%u, %u) is not cut at whole tiles", pass, p.blk_begin, p.blk_end);
      longest = std::max(longest, p.blk_end - p.blk_begin);
      at = p.blk_end;
    }
    CHECK(at == w.end, "pass %u: pieces end at %u of %u", pass, at, w.end);
    CHECK(pass_items(C.B, pass) == by[pass].size(), "pass %u: n_items %u, %zu items laid out", pass, pass_items(C.B, pass), by[pass].size());
    for (const DevItem& p : by0[pass]) longest0 = std::max(longest0, p.blk_end - p.blk_begin);
    CHECK(longest <= longest0, "pass %u: pieces of %u blocks under the cap, %u without it", pass, longest, longest0);
    pieces += by[pass].size();
  }
  // the window-range sections and the groups: as without the cap
  CHECK(it.size() - npk == Z.L.items.size() - Z.L.n_items_pk, "window-range sections of %zu items under the cap, %zu without", it.size() - npk, Z.L.items.size() - Z.L.n_items_pk);
  for (size_t i = 0; i + npk < it.size(); ++i) CHECK(same_item(it[npk + i], Z.L.items[Z.L.n_items_pk + i]), "window-range item %zu differs under the cap", i);
  for (int k = 0; k < 3; ++k) CHECK(C.L.n_items_kind[k] == Z.L.n_items_kind[k], "section %d: %zu items under the cap, %zu without", k, C.L.n_items_kind[k], Z.L.n_items_kind[k]);
  CHECK(C.L.groups.size() == Z.L.groups.size() && (C.L.groups.empty() || !memcmp(C.L.groups.data(), Z.L.groups.data(), C.L.groups.size() * sizeof(BmGroup))), "the scan_bm groups differ under the cap");
}

int main(int argc, char** argv) {
  const int batches = argc > 1 ? atoi(argv[1]) : 60;
  size_t layouts = 0, pieces = 0, cut_more = 0;
  for (int s = 0; s < batches; ++s) {
    Batch B0;
    make_batch((uint64_t)s, B0);
    for (int order : {0, 7})
      for (int group = 0; group < 2; ++group)
        for (int pk = 0; pk < 3; ++pk) {
          LayoutKnobs K{};
          K.item_order = order, K.bm_group = group;
          K.pk_min_items = pk == 0 ? 0 : pk == 1 ? 2048 : (int)B0.plan.items.size() + 1 + (int)(B0.plan.items.size() / 3);
          K.bm_target_items = 1 << 20, K.bm_min_windows = 128, K.bt_target_items = 6144, K.mq_max_chunks = 1 << 22;
          static char what[128];
          snprintf(what, sizeof what, "batch %d item_order %d bm_group %d pk_min_items %d", s, order, group, K.pk_min_items);
          g_what = what;
          Laid Z, Hi;
          lay_out(B0, (s & 1) != 0, K, 0, Z);
          // a cap no item reaches: the layout of cap 0, element for element, and the same piece counts in the passes
          lay_out(B0, (s & 1) != 0, K, 1 << 20, Hi);
          CHECK(Hi.L.items.size() == Z.L.items.size() && Hi.L.n_items_pk == Z.L.n_items_pk, "a cap above every item changes the item count");
          for (size_t i = 0; i < Z.L.items.size(); ++i) CHECK(same_item(Hi.L.items[i], Z.L.items[i]), "a cap above every item changes item %zu", i);
          for (uint32_t p = 0; p < (uint32_t)B0.blocks.size(); ++p) CHECK(pass_items(Hi.B, p) == pass_items(Z.B, p), "a cap above every item changes pass %u's n_items", p);
          for (int k = 0; k < 3; ++k) CHECK(Hi.L.mq_chunks[k] == Z.L.mq_chunks[k], "a cap above every item changes match queue %d", k);
          for (int cap : {4, 8, 16}) {
            Laid C;
            lay_out(B0, (s & 1) != 0, K, cap, C);
            check_capped(B0, Z, C, (uint32_t)cap, pieces);
            cut_more += C.L.n_items_pk > Z.L.n_items_pk;
            ++layouts;
          }
        }
  }
  printf("ok layouts %zu pieces %zu cut_finer %zu\n", layouts, pieces, cut_more);
  return 0;
}
