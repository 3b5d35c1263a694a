// layout.cpp -- the launch layout of a planned batch (mrk::layout_batch, csrc/mrk_plan.cpp) on the CPU.
// Seeded random batches -- block-scan passes with and without further passes, scan_bm pairs over a small pool of keywords,
// scan_bt passes, generic-evaluator passes, declined queries; 1 to 256 queries, queue-fed or not -- are laid out under every
// item_order 0-15, bm_group 0 / 1 and pk_min_items 0 / 2048 / above the item count (default and one experiment setting of the
// other knobs), and each result is checked for what holds by construction: the sections and their counts, every whole range
// covered exactly once, the piece lengths, query-major or piece-major order, the group records, the piece counts written
// back to the passes, the match-queue sizes, and that the same input gives the same output.
// Prints one line per batch, "<batch> <FNV-1a digest of everything layout_batch returned over all the settings>": the
// digests recorded before the cutting loops were unified are in tests/golden/layout_digests.json.
// Built and run by tests/test_layout_cpu.py; no GPU, no libmrk.so.
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

// the section [a, b) of the laid-out items: every owner's pieces in order cover its whole range exactly once; returns the
// pieces per owner
static std::map<uint32_t, std::vector<DevItem>> check_cover(const std::vector<DevItem>& items, size_t a, size_t b, uint32_t kind,
                                                            const std::map<uint32_t, Range>& whole) {
  std::map<uint32_t, std::vector<DevItem>> by;
  for (size_t i = a; i < b; ++i) {
    CHECK(items[i].kind == kind, "item %zu has kind %u in the section of kind %u", i, items[i].kind, kind);
    CHECK(whole.count(items[i].query), "item %zu belongs to %u, which has no range in this section", i, items[i].query);
    by[items[i].query].push_back(items[i]);
  }
  for (const auto& w : whole) {
    if (w.second.begin == w.second.end) {
      CHECK(!by.count(w.first), "owner %u has an empty range and pieces", w.first);
      continue;
    }
    CHECK(by.count(w.first), "owner %u has no pieces", w.first);
    uint32_t at = w.second.begin;
    for (const DevItem& p : by[w.first]) {
      CHECK(p.blk_begin == at && p.blk_end > p.blk_begin, "owner %u: piece [%u, %u) where %u was due", w.first, p.blk_begin, p.blk_end, at);
      at = p.blk_end;
    }
    CHECK(at == w.second.end, "owner %u: pieces end at %u of %u", w.first, at, w.second.end);
  }
  return by;
}

// piece-major: neighbours belong to different owners unless no other owner has pieces left; query-major: an owner's pieces are
// contiguous (ascending: check_cover)
static void check_order(const std::vector<DevItem>& items, size_t a, size_t b, bool piece_major) {
  std::map<uint32_t, size_t> left;
  for (size_t i = a; i < b; ++i) ++left[items[i].query];
  size_t others = b - a; // pieces not yet emitted
  std::map<uint32_t, bool> closed;
  for (size_t i = a; i < b; ++i) {
    const uint32_t o = items[i].query;
    --left[o], --others;
    if (i + 1 == b) break;
    const uint32_t o2 = items[i + 1].query;
    if (piece_major) {
      if (o2 == o) CHECK(others == left[o], "items %zu and %zu both belong to %u while others have %zu pieces left", i, i + 1, o, others - left[o]);
    } else if (o2 != o) {
      CHECK(left[o] == 0, "owner %u is interrupted at item %zu", o, i);
    }
  }
}

static void check_layout(const Batch& B0, const Batch& B, const BatchLayout& L, bool use_packed, const LayoutKnobs& K, bool default_knobs) {
  const uint32_t n = B.n;
  const size_t n_pass = n + B.plan.extra.size();
  auto pass = [&](uint32_t p) -> const DevQuery& { return p < n ? B.head[p] : B.plan.extra[p - n]; };
  const std::vector<DevItem>& in_bm = B0.plan.items_bm;
  // ---- sections and counts
  CHECK(L.n_items_pk + L.n_items_kind[0] + L.n_items_kind[1] + L.n_items_kind[2] == L.items.size(), "the sections do not add up to %zu items", L.items.size());
  const size_t s0 = L.n_items_pk, s1 = s0 + L.n_items_kind[0], s2 = s1 + L.n_items_kind[1], s3 = L.items.size();
  CHECK(B.plan.items.empty(), "the block items stayed with the plan");
  if (!use_packed) { // the VLB path: the planner's items as they are
    CHECK(L.items.size() == B0.plan.items.size() && (L.items.empty() || !memcmp(L.items.data(), B0.plan.items.data(), L.items.size() * sizeof(DevItem))), "VLB items changed");
    CHECK(!L.mq_chunks[0] && !L.mq_chunks[1] && !L.mq_chunks[2], "VLB path with match queues");
    return;
  }
  // ---- block-scan section
  {
    std::map<uint32_t, Range> whole;
    for (uint32_t p = 0; p < n_pass; ++p)
      if (B.blocks[p].end) whole[p] = B.blocks[p];
    const auto by = check_cover(L.items, 0, s0, 0, whole);
    for (const auto& o : by)
      for (const DevItem& p : o.second)
        CHECK(p.blk_begin % mrk::T0_BLOCKS == 0 && ((p.blk_end - p.blk_begin) % mrk::T0_BLOCKS == 0 || p.blk_end == whole[o.first].end),
              "block piece [%u, %u) of pass %u", p.blk_begin, p.blk_end, o.first);
    const bool cut = !B0.plan.items.empty() && B0.plan.items.size() < (size_t)K.pk_min_items;
    if (!cut) CHECK(s0 == B0.plan.items.size(), "%zu block items became %zu without a cut", B0.plan.items.size(), s0);
    if (cut) CHECK(s0 >= B0.plan.items.size(), "a cut left fewer block items");
    for (uint32_t p = 0; p < n_pass; ++p) // the piece counts the match-queue sizing reads
      if (whole.count(p)) CHECK(pass(p).n_items == by.at(p).size(), "pass %u: n_items %u, %zu pieces", p, pass(p).n_items, by.at(p).size());
    check_order(L.items, 0, s0, (K.item_order & 1) && (!B.plan.any_prox || (K.item_order & 8)));
  }
  // ---- window-range sections: the burst unit and the documented piece length
  auto wpi_of = [&](uint32_t kind) {
    uint64_t total = 0;
    for (const DevItem& it : in_bm)
      if (it.kind == kind) total += it.blk_end - it.blk_begin;
    const uint64_t unit = 4 * mrk::WAVES;
    uint64_t wpi = total / (uint64_t)(kind == 0 ? K.bm_target_items : K.bt_target_items) / unit * unit;
    const uint64_t least = kind == 0 ? (uint64_t)K.bm_min_windows / unit * unit : 4 * unit;
    return std::min<uint64_t>(std::max(wpi, least), 4096);
  };
  auto check_lengths = [&](const std::vector<DevItem>& pieces, const Range& w, uint64_t want) {
    CHECK(want >= 1 && want <= 4096, "piece length %llu", (unsigned long long)want);
    for (const DevItem& p : pieces) CHECK(p.blk_end - p.blk_begin == want || (p.blk_end == w.end && p.blk_end - p.blk_begin < want), "piece [%u, %u), %llu wanted", p.blk_begin, p.blk_end, (unsigned long long)want);
  };
  {
    const bool grouped = K.bm_group && (K.item_order & 2);
    const uint64_t wpi = wpi_of(0);
    if (default_knobs) CHECK(wpi % (4 * mrk::WAVES) == 0 && wpi >= 128, "wpi %llu", (unsigned long long)wpi);
    std::map<uint32_t, Range> whole;
    std::vector<uint32_t> members; // scan_bm passes
    for (const DevItem& it : in_bm)
      if (it.kind == 0) members.push_back(it.query);
    if (grouped) {
      CHECK(L.groups.empty() == members.empty(), "%zu groups for %zu scan_bm passes", L.groups.size(), members.size());
      std::vector<uint32_t> seen;
      uint32_t by_size[mrk::BM_GROUP_MAX] = {};
      for (uint32_t g = 0; g < L.groups.size(); ++g) {
        const BmGroup& G = L.groups[g];
        CHECK(G.n >= 1 && G.n <= (uint32_t)mrk::BM_GROUP_MAX && G.per == mrk::WAVES / G.n && G.ntab >= 1 && G.ntab <= (uint32_t)mrk::BM_GROUP_TABS, "group %u: n %u per %u ntab %u", g, G.n, G.per, G.ntab);
        ++by_size[G.n - 1];
        for (uint32_t j = 0; j < G.n; ++j) {
          CHECK(G.q[j] < n_pass && (pass(G.q[j]).tree_flags & mrk::TF_BITMAP), "group %u member %u is pass %u", g, j, G.q[j]);
          seen.push_back(G.q[j]);
          for (uint32_t t = 0; t < 2; ++t) { // the member's keyword t reads table k, which was built from one of the group's own keywords
            const uint32_t k = (G.tab_idx >> (6 * j + 3 * t)) & 7;
            CHECK(k < G.ntab, "group %u member %u keyword %u: table %u of %u", g, j, t, k, G.ntab);
            const uint32_t src = G.tab_src[k];
            CHECK((src >> 1) < G.n, "group %u: table %u built from member %u", g, k, src >> 1);
            const DevTerm &mine = pass(G.q[j]).t[t], &from = pass(G.q[src >> 1]).t[src & 1];
            CHECK(mine.bm_off == from.bm_off && !memcmp(&mine.idf, &from.idf, 4), "group %u member %u keyword %u reads another keyword's table", g, j, t);
          }
        }
        for (uint32_t k = 0; k < G.ntab; ++k) // the tables are distinct keywords
          for (uint32_t k2 = 0; k2 < k; ++k2) {
            const DevTerm &x = pass(G.q[G.tab_src[k] >> 1]).t[G.tab_src[k] & 1], &y = pass(G.q[G.tab_src[k2] >> 1]).t[G.tab_src[k2] & 1];
            CHECK(x.bm_off != y.bm_off || memcmp(&x.idf, &y.idf, 4), "group %u: tables %u and %u hold one keyword", g, k, k2);
          }
        for (const DevItem& it : in_bm)
          if (it.kind == 0 && it.query == G.q[0]) whole[g] = Range{it.blk_begin, it.blk_end};
      }
      std::sort(seen.begin(), seen.end());
      std::sort(members.begin(), members.end());
      CHECK(seen == members, "the groups hold %zu passes, the batch %zu scan_bm passes (each exactly once)", seen.size(), members.size());
      CHECK(!memcmp(by_size, L.n_bm_groups, sizeof by_size), "n_bm_groups");
    } else {
      CHECK(L.groups.empty() && !L.n_bm_groups[0] && !L.n_bm_groups[1] && !L.n_bm_groups[2] && !L.n_bm_groups[3], "groups on the ungrouped layout");
      for (const DevItem& it : in_bm)
        if (it.kind == 0) whole[it.query] = Range{it.blk_begin, it.blk_end};
    }
    const auto by = check_cover(L.items, s0, s1, 0, whole);
    for (const auto& o : by) {
      // a group of n members: a wave walks wpi / WAVES windows, a member has WAVES / n waves (3 members walk like 4)
      const uint64_t want = grouped ? wpi * (mrk::WAVES / L.groups[o.first].n) / mrk::WAVES : wpi;
      check_lengths(o.second, whole[o.first], want);
      if (default_knobs && (!grouped || L.groups[o.first].n == 1)) CHECK(want % (4 * mrk::WAVES) == 0, "lone query with pieces of %llu", (unsigned long long)want);
    }
    check_order(L.items, s0, s1, (K.item_order & 2) != 0);
  }
  {
    const uint64_t wpi = wpi_of(1);
    if (default_knobs) CHECK(wpi % (4 * mrk::WAVES) == 0 && wpi >= 64, "wpi %llu", (unsigned long long)wpi);
    std::map<uint32_t, Range> whole;
    for (const DevItem& it : in_bm)
      if (it.kind == 1) whole[it.query] = Range{it.blk_begin, it.blk_end};
    const auto by = check_cover(L.items, s1, s2, 1, whole);
    for (const auto& o : by) check_lengths(o.second, whole[o.first], wpi);
    check_order(L.items, s1, s2, (K.item_order & 4) && (!B.plan.any_prox || (K.item_order & 8)));
  }
  { // the generic evaluator's items: as planned
    size_t at = s2;
    for (const DevItem& it : in_bm)
      if (it.kind == 2) {
        CHECK(at < s3 && !memcmp(&L.items[at], &it, sizeof it), "generic-evaluator item %zu", at - s2);
        ++at;
      }
    CHECK(at == s3, "%zu generic-evaluator items, %zu planned", s3 - s2, at - s2);
  }
  // ---- passes: only n_items may change, and only where block items were cut
  for (uint32_t p = 0; p < n_pass; ++p) {
    DevQuery was = p < n ? B0.head[p] : B0.plan.extra[p - n];
    if (B.blocks[p].end) was.n_items = pass(p).n_items;
    CHECK(!memcmp(&was, &pass(p), sizeof was), "pass %u changed", p);
  }
  // ---- match queues
  uint64_t chunks[3] = {0, 0, 0};
  if (B.plan.any_prox) {
    bool bt_feeds[3] = {false, false, false};
    for (uint32_t p = 0; p < n_pass; ++p) {
      const DevQuery& P = pass(p);
      bool fat = false;
      if (!P.n_items || !mrk::pass_queues_matches(P, fat)) continue;
      const int q = mrk::queue_of(P, fat);
      const bool bt = (P.tree_flags & mrk::TF_BTREE) != 0;
      // one entry per doc the pass can match, and per wave of its items a reservation of MQ_BATCH chunks + a partial one
      chunks[q] += mrk::pass_max_matches(P) / 64 + 1 + (bt ? 0 : 4ull * (mrk::MQ_BATCH + 1) * P.n_items);
      if (bt) bt_feeds[q] = true;
    }
    for (int q = 0; q < 3; ++q) {
      if (bt_feeds[q]) chunks[q] += 4ull * (mrk::MQ_BATCH + 1) * L.n_items_kind[1];
      chunks[q] = std::min<uint64_t>(chunks[q], (uint64_t)K.mq_max_chunks);
    }
  }
  for (int q = 0; q < 3; ++q)
    CHECK(L.mq_chunks[q] == chunks[q] && L.mq_chunks[q] <= (uint64_t)K.mq_max_chunks, "queue %d: %llu chunks, %llu by the formula", q, (unsigned long long)L.mq_chunks[q], (unsigned long long)chunks[q]);
}

static void digest(uint64_t& h, const Batch& B, const BatchLayout& L) {
  const uint64_t counts[4] = {L.n_items_pk, L.n_items_kind[0], L.n_items_kind[1], L.n_items_kind[2]};
  const uint64_t sizes[2] = {L.items.size(), L.groups.size()};
  fnv(h, sizes, sizeof sizes);
  fnv(h, counts, sizeof counts);
  fnv(h, L.items.data(), L.items.size() * sizeof(DevItem));
  fnv(h, L.groups.data(), L.groups.size() * sizeof(BmGroup));
  fnv(h, L.n_bm_groups, sizeof L.n_bm_groups);
  fnv(h, L.mq_chunks, sizeof L.mq_chunks);
  for (const DevQuery& P : B.head) fnv(h, &P.n_items, 4);
  for (const DevQuery& P : B.plan.extra) fnv(h, &P.n_items, 4);
}

int main(int argc, char** argv) {
  const int batches = argc > 1 ? atoi(argv[1]) : 100;
  size_t layouts = 0, items = 0, groups = 0;
  for (int s = 0; s < batches; ++s) {
    Batch B0;
    make_batch((uint64_t)s, B0);
    uint64_t h = 0xCBF29CE484222325ull;
    for (int alt = 0; alt < 2; ++alt)
      for (int order = 0; order < 16; ++order)
        for (int group = 0; group < 2; ++group)
          for (int pk = 0; pk < 3; ++pk) {
            LayoutKnobs K{};
            K.item_order = order, K.bm_group = group;
            K.pk_min_items = pk == 0 ? 0 : pk == 1 ? 2048 : (int)B0.plan.items.size() + 1 + (int)(B0.plan.items.size() / 3);
            // the context's defaults; `alt`: short pieces, small queues (experiment settings)
            K.bm_target_items = alt ? 2048 : 1 << 20, K.bm_min_windows = alt ? 70 : 128, K.bt_target_items = alt ? 512 : 6144;
            K.mq_max_chunks = alt ? 3000 : 1 << 22;
            const bool use_packed = !(alt && order == 5 && B0.plan.items_bm.empty()); // (the planner leaves the VLB path block items only)
            static char what[128];
            snprintf(what, sizeof what, "batch %d alt %d item_order %d bm_group %d pk_min_items %d", s, alt, order, group, K.pk_min_items);
            g_what = what;
            Batch B = B0, B2 = B0;
            BatchLayout L, L2;
            mrk::layout_batch(B.head.data(), B.n, B.plan, use_packed, (s & 1) != 0, K, L);
            check_layout(B0, B, L, use_packed, K, !alt);
            mrk::layout_batch(B2.head.data(), B2.n, B2.plan, use_packed, (s & 1) != 0, K, L2);
            uint64_t h1 = 0, h2 = 0;
            digest(h1, B, L), digest(h2, B2, L2);
            CHECK(h1 == h2 && L.items.size() == L2.items.size() && L.groups.size() == L2.groups.size(), "the same batch laid out differently the second time");
            digest(h, B, L);
            ++layouts, items += L.items.size(), groups += L.groups.size();
          }
    printf("%d %016llx\n", s, (unsigned long long)h);
  }
  printf("ok layouts %zu items %zu groups %zu\n", layouts, items, groups);
  return 0;
}
