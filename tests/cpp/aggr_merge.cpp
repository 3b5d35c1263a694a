// aggr_merge.cpp -- the merge of AGGREGATE rows (include/mrk.h: MRK_AROW_WORDS) restated sequentially over what merge_arows_kernel
// itself goes through -- csrc/mrk_kgroup.h: the row reader aggr_row_head, group_spec_unpack, aggr_spec_word / aggr_spec_unpack /
// aggr_spec_op, group_update_slot and group_aggr_update (GroupSeqOps in the place of the device atomics), aggr_map / aggr_unmap,
// group_order_key / group_order_key_aggr -- on the CPU under AddressSanitizer + UBSan.  Every input row and every table lives in a
// heap block of its EXACT size (a table: group_table_words(slots, n) for the n aggregates of the spec), so a read behind a row or an
// accumulator behind a table is a sanitizer report.
//   - random shards of one match set, all three funcs x {INT, widened, INT64}, with and without an ordering aggregate: the merged
//     row equals a std::map's answer over all matches, and a staged merge equals the one-step merge
//   - the identity edges: a 32-bit SUM that wraps across lists and its widened twin, an INT64 sum across INT64_MAX, MIN of only
//     0xFFFFFFFF, MAX of only 0, signed MAX of INT64_MIN, signed MIN of INT64_MAX, a group of only -1, an order reversed by the merge
//   - hostile rows in list 0 / a middle list / the last: an entry count above G, every kind of bad aggregate spec, an aggregate spec
//     over group spec 0 -- MRK_ROW_DECLINED, no entries, never an access outside a row
//   - RERUN, DECLINED with and without specs, aggregate specs that differ in one bit, "with aggregates" next to "without"
//   - the aggregate spec's pack / unpack round trip and the fifth decline bit's truth table
// Built and run by tests/test_aggr_merge_cpu.py; no GPU, no libmrk.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_host_int.h" // (aggr_row_decline_bit; it brings mrk_dev.h's RowKind and the HIP qualifiers)
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

static const uint64_t FLAGS = MRK_ROW_RERUN | MRK_ROW_DECLINED;
static const uint32_t G = GROW_GROUPS;

struct Row { // a heap block of exactly one row
  uint64_t* w;
  Row() { w = (uint64_t*)calloc(AROW_WORDS, 8); }
  Row(const Row& o) : Row() { memcpy(w, o.w, AROW_WORDS * 8); }
  Row& operator=(const Row& o) {
    memcpy(w, o.w, AROW_WORDS * 8);
    return *this;
  }
  ~Row() { free(w); }
  bool operator==(const Row& o) const { return memcmp(w, o.w, AROW_WORDS * 8) == 0; }
};

// The kernel's grouped path, one entry after another.  k: the call's k.
static Row merge(const std::vector<Row>& lists, uint32_t k) {
  Row out;
  uint64_t spec = 0, aspec = 0, flags = 0;
  bool have_spec = false, mismatch = false;
  for (const Row& r : lists) {
    uint64_t t, sp, asp;
    (void)aggr_row_head(r.w, t, sp, asp);
    flags |= t & FLAGS;
    if (!group_row_has_say(t, sp)) continue;
    if (!have_spec) spec = sp, aspec = asp, have_spec = true;
    mismatch = mismatch || sp != spec || asp != aspec;
  }
  if (mismatch) flags |= MRK_ROW_DECLINED;
  out.w[AROW_GSPEC] = spec, out.w[AROW_ASPEC] = aspec;
  if (spec == 0) { // (the narrow merge is mrk_topk_merge_rows' and tested there: here only its flags)
    if (aspec) abort(); // (the reader lets no aggregate spec stand over group spec 0)
    out.w[GROW_TOTAL] = flags;
    return out;
  }
  GroupSpec gs;
  AggrSpec as{0, 0};
  if (!group_spec_unpack(spec, gs) || (aspec && !aggr_spec_unpack(aspec, gs.sort_by, as))) abort(); // (an answering list's specs unpacked in aggr_row_head)
  if (gs.k > k) flags |= MRK_ROW_DECLINED;
  if (!flags) {
    const uint32_t slots = group_slots_for(gs.k);
    uint64_t* mem = (uint64_t*)calloc((size_t)group_table_words(slots, as.n), 8); // exact size: as.n planes
    const GroupTable T = group_table_at(mem, slots);
    unsigned long long sum_in = 0, sum_out = 0;
    bool ok = true;
    for (const Row& r : lists) {
      uint64_t t, sp, asp;
      const uint32_t c = aggr_row_head(r.w, t, sp, asp);
      for (uint32_t i = 0; i < c; ++i) {
        const uint64_t pw = r.w[GROW_PLANE + i];
        const uint32_t slot = group_update_slot<GroupSeqOps>(T, (uint32_t)(pw >> 32), (uint32_t)pw, r.w[i]);
        ok = ok && slot != 0xFFFFFFFFu;
        sum_in += (uint32_t)pw;
        if (slot != 0xFFFFFFFFu)
          for (uint32_t a = 0; a < as.n; ++a) {
            const uint32_t op = aggr_spec_op(aspec, a);
            group_aggr_update<GroupSeqOps>(T, slot, a, op, aggr_map(op, r.w[AROW_AGGR + a * G + i]));
          }
      }
    }
    if (!ok || *T.claimed > group_limit(gs.k) || *T.claimed > GRP_MAX_GROUPS)
      flags |= MRK_ROW_DECLINED;
    else {
      std::vector<std::pair<uint64_t, uint32_t>> ord;
      for (uint32_t i = 0; i < slots; ++i)
        if (T.keys[i]) {
          const uint64_t key = as.order ? group_order_key_aggr(gs.desc, (uint32_t)aggr_unmap(aggr_spec_op(aspec, as.order - 1), T.aggr[(uint64_t)(as.order - 1) * slots + i]), T.heads[i])
                                        : group_order_key(gs.sort_by, gs.desc, (uint32_t)T.keys[i], T.counts[i], T.heads[i]);
          ord.push_back({key, i}), sum_out += T.counts[i];
        }
      if (sum_out != sum_in)
        flags |= MRK_ROW_DECLINED; // a slot wrapped: it is short by 2^32
      else {
        std::sort(ord.begin(), ord.end(), [](const auto& a, const auto& b) { return a.first > b.first || (a.first == b.first && a.second < b.second); });
        for (size_t i = 0; i < ord.size(); ++i) {
          const uint32_t s = ord[i].second;
          out.w[i] = T.heads[s];
          out.w[GROW_PLANE + i] = group_plane_word((uint32_t)T.keys[s], T.counts[s]);
          for (uint32_t a = 0; a < as.n; ++a) out.w[AROW_AGGR + a * G + i] = aggr_unmap(aggr_spec_op(aspec, a), T.aggr[(uint64_t)a * slots + s]);
        }
        out.w[GROW_CNT] = out.w[GROW_TOTAL] = ord.size();
      }
    }
    free(mem);
  }
  if (flags) out.w[GROW_TOTAL] = flags;
  return out;
}

// ---- the expectation, from the format's and the aggregates' definitions: plain integer arithmetic in a std::map
struct Kind {
  uint32_t func;
  bool src64, widen;
};
struct Match {
  uint32_t rowid, value;
  int32_t weight;
  uint64_t src[MRK_MAX_AGGRS]; // an INT source zero-extended, an INT64 one its bits
};
struct Grp {
  uint64_t head = 0, count = 0;
  bool seen = false;
  uint64_t ag[MRK_MAX_AGGRS] = {};
};
static void push(Grp& g, const Match& m, const std::vector<Kind>& kinds) {
  g.count++;
  g.head = std::max(g.head, make_key(m.weight, m.rowid));
  for (size_t a = 0; a < kinds.size(); ++a) {
    const Kind& kd = kinds[a];
    const uint64_t v = m.src[a];
    if (!g.seen)
      g.ag[a] = v;
    else if (kd.func == MRK_AGGR_SUM)
      g.ag[a] += v;
    else if (kd.src64)
      g.ag[a] = (kd.func == MRK_AGGR_MIN) == ((int64_t)v < (int64_t)g.ag[a]) ? v : g.ag[a];
    else
      g.ag[a] = (kd.func == MRK_AGGR_MIN) == (v < g.ag[a]) ? v : g.ag[a];
  }
  g.seen = true;
}
static uint64_t result_of(const Grp& g, size_t a, const Kind& kd) { return kd.src64 || kd.widen ? g.ag[a] : (uint64_t)(uint32_t)g.ag[a]; }

static uint64_t aspec_of(const std::vector<Kind>& kinds, int order_by) {
  if (kinds.empty()) return 0;
  uint64_t w = 1ull | ((uint64_t)kinds.size() << 1) | ((uint64_t)(order_by + 1) << 4);
  for (size_t a = 0; a < kinds.size(); ++a) w |= (uint64_t)(kinds[a].func | (kinds[a].src64 ? 4u : 0u) | (kinds[a].widen ? 8u : 0u)) << (8 + 4 * a);
  return w;
}

static Row row_of(const std::vector<Match>& ms, uint32_t sort_by, uint32_t desc, uint32_t k, const std::vector<Kind>& kinds, int order_by) {
  std::map<uint32_t, Grp> g;
  for (const Match& m : ms) push(g[m.value], m, kinds);
  Row r;
  r.w[AROW_GSPEC] = group_spec_word(sort_by, desc, 32, k), r.w[AROW_ASPEC] = aspec_of(kinds, order_by);
  if (g.size() > 4 * (size_t)k) {
    r.w[GROW_TOTAL] = MRK_ROW_DECLINED;
    return r;
  }
  struct E {
    uint32_t v;
    Grp g;
  };
  std::vector<E> es;
  for (auto& kv : g) es.push_back({kv.first, kv.second});
  auto part = [&](const E& e) -> int64_t {
    if (order_by >= 0) return (int64_t)(uint32_t)result_of(e.g, (size_t)order_by, kinds[(size_t)order_by]);
    return sort_by == MRK_GROUPSORT_COUNT ? (int64_t)e.g.count : sort_by == MRK_GROUPSORT_KEY ? (int64_t)e.v : (int64_t)key_weight(e.g.head);
  };
  std::sort(es.begin(), es.end(), [&](const E& a, const E& b) {
    const int64_t pa = part(a), pb = part(b);
    if (pa != pb) return desc ? pa > pb : pa < pb;
    return key_rowid(a.g.head) < key_rowid(b.g.head);
  });
  for (size_t i = 0; i < es.size(); ++i) {
    r.w[i] = es[i].g.head, r.w[GROW_PLANE + i] = ((uint64_t)es[i].v << 32) | (uint32_t)es[i].g.count;
    for (size_t a = 0; a < kinds.size(); ++a) r.w[AROW_AGGR + a * G + i] = result_of(es[i].g, a, kinds[a]);
  }
  r.w[GROW_CNT] = r.w[GROW_TOTAL] = es.size();
  return r;
}

static uint32_t rnd_state = 12345;
static uint32_t rnd() {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}
static uint64_t rnd64() { return ((uint64_t)rnd() << 40) ^ ((uint64_t)rnd() << 20) ^ rnd(); }

static bool empty_under(const Row& r, uint64_t flags, uint64_t spec, uint64_t aspec) {
  for (int i = 0; i < AROW_GSPEC; ++i)
    if (i != GROW_TOTAL && r.w[i]) return false;
  return r.w[GROW_TOTAL] == flags && r.w[AROW_GSPEC] == spec && r.w[AROW_ASPEC] == aspec;
}
static bool empty_declined(const Row& r, uint64_t spec, uint64_t aspec) { return empty_under(r, MRK_ROW_DECLINED, spec, aspec); }

// one group (value 7) whose matches' sources are given per list; one aggregate
static Row one_group(const std::vector<uint64_t>& src, uint32_t first_rowid, Kind kd, uint32_t k = 4) {
  std::vector<Match> ms;
  for (size_t i = 0; i < src.size(); ++i) ms.push_back({first_rowid + (uint32_t)i, 7u, 1, {src[i]}});
  return row_of(ms, MRK_GROUPSORT_KEY, 1, k, {kd}, -1);
}

int main() {
  const Kind SUM32{MRK_AGGR_SUM, false, false}, SUMW{MRK_AGGR_SUM, false, true}, SUM64{MRK_AGGR_SUM, true, false};
  const Kind MIN32{MRK_AGGR_MIN, false, false}, MINW{MRK_AGGR_MIN, false, true}, MIN64{MRK_AGGR_MIN, true, false};
  const Kind MAX32{MRK_AGGR_MAX, false, false}, MAXW{MRK_AGGR_MAX, false, true}, MAX64{MRK_AGGR_MAX, true, false};

  // ---- the aggregate spec word: every func / kind / widen / order combination round-trips; the op word it rebuilds
  unsigned n_spec = 0;
  {
    const Kind all[] = {SUM32, SUMW, SUM64, MIN32, MINW, MIN64, MAX32, MAXW, MAX64};
    for (uint32_t n = 1; n <= (uint32_t)MRK_MAX_AGGRS; ++n)
      for (uint32_t c = 0; c < 9 * 9; ++c)
        for (int order = -1; order < (int)n; ++order) {
          std::vector<Kind> kinds;
          uint32_t ops[MRK_MAX_AGGRS] = {};
          for (uint32_t a = 0; a < n; ++a) {
            kinds.push_back(all[(c / (a % 2 ? 9 : 1) + a) % 9]);
            ops[a] = aggr_op_word(kinds[a].func, 5 + a, 32, kinds[a].src64, kinds[a].widen); // (shift and bits do not travel)
          }
          const bool order_ok = order < 0 || !(kinds[(size_t)order].src64 || kinds[(size_t)order].widen);
          const uint64_t w = aggr_spec_word(n, (uint32_t)(order + 1), ops);
          AggrSpec as;
          CHECK(w == aspec_of(kinds, order), "the word's layout");
          CHECK(aggr_spec_unpack(w, MRK_GROUPSORT_KEY, as) == order_ok, "n %u order %d: unpack", n, order);
          if (order_ok) CHECK(as.n == n && as.order == (uint32_t)(order + 1), "n / order round trip");
          CHECK(aggr_spec_unpack(w, MRK_GROUPSORT_COUNT, as) == (order < 0) && aggr_spec_unpack(w, MRK_GROUPSORT_WEIGHT, as) == (order < 0), "an order next to another sort_by");
          for (uint32_t a = 0; a < n; ++a) {
            const uint32_t op = aggr_spec_op(w, a);
            CHECK(aggr_func(op) == kinds[a].func && ((op & AGGR_SRC64) != 0) == kinds[a].src64 && ((op & AGGR_WIDEN) != 0) == kinds[a].widen && (op & 0x7FFu) == 0u, "the rebuilt op word");
            for (uint64_t v : {0ull, 1ull, 0xFFFFFFFFull, 1ull << 63, ~0ull, (1ull << 63) - 1}) {
              const uint64_t val = kinds[a].src64 || kinds[a].widen ? v : (uint32_t)v;
              CHECK(aggr_unmap(op, aggr_map(op, val)) == val, "map / unmap under the rebuilt op");
            }
          }
          ++n_spec;
        }
  }
  const uint64_t good2 = aspec_of({SUM32, MAX64}, 0);
  const uint64_t bad_aspecs[] = {
      good2 | (1ull << 7), good2 | (1ull << 24), good2 | (1ull << 63), good2 & ~1ull, // a stray bit; bit 0 clear
      aspec_of({}, -1) | 1ull,                                                           // n = 0
      (good2 & ~0xEull) | (5ull << 1),                                                   // n = 5
      aspec_of({SUM32, Kind{0, false, false}}, -1),                                      // func 0 inside n
      good2 | (1ull << 16),                                                              // a nonzero field beyond n
      aspec_of({SUM32, Kind{MRK_AGGR_MAX, true, true}}, -1),                             // both width bits
      aspec_of({SUM32, MAX64}, 1), aspec_of({SUMW, MAX64}, 0),                           // an order that names a 64-bit result
      aspec_of({SUM32, MAX64}, 2), aspec_of({SUM32}, 1)};                                // an order with an index >= n
  {
    AggrSpec as;
    CHECK(aggr_spec_unpack(good2, MRK_GROUPSORT_KEY, as) && as.n == 2 && as.order == 1, "the good word");
    for (uint64_t b : bad_aspecs) CHECK(!aggr_spec_unpack(b, MRK_GROUPSORT_KEY, as), "aggregate spec %llx unpacked", (unsigned long long)b);
    CHECK(!aggr_spec_unpack(0ull, MRK_GROUPSORT_KEY, as), "0 is no spec to unpack");
  }

  // ---- the fifth decline bit: status, sort bits, an order -- not the aggregates
  for (int status : {0, -1, -2})
    for (uint32_t bits : {0u, 32u})
      for (uint32_t order : {0u, 1u, 2u, 3u}) {
        const uint32_t want = status != 0 || bits != 0 || order != 0 ? 1u << 4 : 0u;
        CHECK(aggr_row_decline_bit(status, bits, order) == want && (ROWS_AGGR == 4), "decline bit %d %u %u", status, bits, order);
        CHECK((group_row_decline_bit(status, bits, order) != 0) == (want != 0) && group_row_decline_bit(status, bits, order) <= 1u << 3, "beside the group row's");
      }
  CHECK(MRK_AROW_WORDS == 6 * MRK_GROW_GROUPS + 4 && AROW_AGGR == 2 * GROW_GROUPS + 2 && AROW_AGGR + MRK_MAX_AGGRS * GROW_GROUPS == AROW_GSPEC && AROW_ASPEC == AROW_WORDS - 1, "the layout");

  // ---- random shards against a std::map over all matches; staged == one step
  unsigned n_merged = 0;
  const std::vector<std::vector<Kind>> sets = {{SUM32, MIN32, MAX32}, {SUMW, MINW, MAXW, SUM32}, {SUM64, MIN64, MAX64}, {MAX32, SUM64, MINW, SUM32}, {MIN32}, {}};
  for (uint32_t K : {1u, 2u, 4u, 20u})
    for (size_t si = 0; si < sets.size(); ++si)
      for (int order : {-1, 0, 3})
        for (uint32_t desc = 0; desc < 2; ++desc)
          for (uint32_t card : {1u, 3u, 4u * K, 4u * K + 1u}) {
            const std::vector<Kind>& kinds = sets[si];
            if (order >= (int)kinds.size() || (order >= 0 && (kinds[(size_t)order].src64 || kinds[(size_t)order].widen))) continue;
            const uint32_t by = order >= 0 ? (uint32_t)MRK_GROUPSORT_KEY : (uint32_t)((si + K) % 3);
            const uint32_t S = 1 + rnd() % 8;
            std::vector<Row> lists;
            std::vector<Match> every;
            for (uint32_t s = 0; s < S; ++s) {
              std::vector<Match> ms;
              const uint32_t n = rnd() % 300;
              for (uint32_t i = 0; i < n; ++i) {
                Match m{s * 1000 + i, (rnd() % card) * 0x9E3779B1u, (int32_t)(rnd() % 5) - 2, {}};
                for (size_t a = 0; a < kinds.size(); ++a) m.src[a] = kinds[a].src64 ? rnd64() : (rnd() % 3 ? 0xF0000000u | rnd() : rnd() % 4);
                ms.push_back(m);
              }
              every.insert(every.end(), ms.begin(), ms.end());
              lists.push_back(row_of(ms, by, desc, K, kinds, order));
            }
            const Row got = merge(lists, 1024);
            const Row want = row_of(every, by, desc, K, kinds, order);
            CHECK(got == want, "K %u set %zu order %d desc %u card %u: merged row != the row of all matches", K, si, order, desc, card);
            Row acc = lists[0];
            for (uint32_t s = 1; s < S; ++s) acc = merge({acc, lists[s]}, 1024);
            if (S == 1) acc = merge({acc}, 1024);
            CHECK(acc == got, "K %u set %zu order %d desc %u card %u: staged != one step", K, si, order, desc, card);
            ++n_merged;
          }

  // ---- the identity edges
  unsigned n_edges = 0;
  auto value0 = [](const Row& r) { return r.w[AROW_AGGR]; };
  auto edge = [&](const char* what, const std::vector<std::vector<uint64_t>>& per_list, Kind kd, uint64_t want) {
    std::vector<Row> lists;
    uint32_t rowid = 0;
    for (const auto& src : per_list) lists.push_back(one_group(src, rowid, kd)), rowid += 100;
    const Row m = merge(lists, 4);
    CHECK(m.w[GROW_TOTAL] == 1 && m.w[GROW_CNT] == 1 && value0(m) == want, "%s: %llx, want %llx", what, (unsigned long long)value0(m), (unsigned long long)want);
    std::vector<Row> rev(lists.rbegin(), lists.rend());
    CHECK(merge(rev, 4).w[AROW_AGGR] == want, "%s: the lists reversed", what);
    ++n_edges;
  };
  const uint64_t ones = 0xFFFFFFFFull, i64min = 1ull << 63, i64max = (1ull << 63) - 1, m1 = ~0ull;
  edge("a 32-bit SUM wraps across lists, every list's own sum below 2^32", {{ones}, {ones}, {ones}}, SUM32, (3 * ones) & ones);
  edge("... its widened twin does not", {{ones}, {ones}, {ones}}, SUMW, 3 * ones);
  edge("an INT64 sum crosses INT64_MAX", {{i64max}, {1}, {5}}, SUM64, i64max + 6);
  edge("an INT64 sum of negatives", {{m1, m1}, {i64min}, {3}}, SUM64, i64min + 1);
  edge("MIN of only 0xFFFFFFFF (mapped 0)", {{ones}, {ones, ones}}, MIN32, ones);
  edge("widened MIN of only 0xFFFFFFFF", {{ones}, {ones}}, MINW, ones);
  edge("MAX of only 0", {{0}, {0, 0}}, MAX32, 0);
  edge("signed MAX of INT64_MIN", {{i64min}, {i64min}}, MAX64, i64min);
  edge("signed MIN of INT64_MAX", {{i64max}, {i64max}}, MIN64, i64max);
  edge("a group of only -1: signed MIN", {{m1}, {m1}}, MIN64, m1);
  edge("a group of only -1: signed MAX", {{m1}, {m1}}, MAX64, m1);
  edge("a group of only -1: SUM", {{m1}, {m1, m1}}, SUM64, (uint64_t)-3ll);
  edge("signed MIN next to positives", {{5}, {m1}, {i64max}}, MIN64, m1);
  edge("unsigned MAX: 0xFFFFFFFF is the largest", {{5}, {ones}, {0}}, MAX32, ones);
  edge("the extreme of a MIN sits in one list of 8", {{9}, {9}, {9}, {9}, {9}, {2}, {9}, {9}}, MIN32, 2);
  edge("the extreme of a MAX sits in one list of 8", {{9}, {9}, {11}, {9}, {9}, {9}, {9}, {9}}, MAXW, 11);
  { // a group in one list of 8 (first, middle, last) next to a group in all 8
    for (uint32_t where : {0u, 3u, 7u}) {
      std::vector<Row> lists;
      std::vector<Match> every;
      for (uint32_t l = 0; l < 8; ++l) {
        std::vector<Match> ms = {{l * 10, 1u, 1, {l + 1}}};
        if (l == where) ms.push_back({l * 10 + 1, 2u, 1, {40}});
        every.insert(every.end(), ms.begin(), ms.end());
        lists.push_back(row_of(ms, MRK_GROUPSORT_KEY, 0, 4, {SUM32}, -1));
      }
      const Row m = merge(lists, 4);
      CHECK(m == row_of(every, MRK_GROUPSORT_KEY, 0, 4, {SUM32}, -1) && m.w[GROW_TOTAL] == 2 && m.w[AROW_AGGR] == 36 && m.w[AROW_AGGR + 1] == 40, "a group in list %u only", where);
      ++n_edges;
    }
  }
  { // the order reversed by the merge: group 1 is worst in every list's own order (descending sums) and best after merging ...
    std::vector<Row> lists;
    std::vector<Match> every;
    for (uint32_t l = 0; l < 3; ++l) {
      std::vector<Match> ms = {{l * 10, 1u, 1, {4}}, {l * 10 + 1, 2u + l, 1, {5}}};
      every.insert(every.end(), ms.begin(), ms.end());
      lists.push_back(row_of(ms, MRK_GROUPSORT_KEY, 1, 4, {SUM32}, 0));
      CHECK((uint32_t)(lists.back().w[GROW_PLANE + 1] >> 32) == 1u, "group 1 is last in list %u", l);
    }
    const Row m = merge(lists, 4);
    CHECK(m == row_of(every, MRK_GROUPSORT_KEY, 1, 4, {SUM32}, 0) && (uint32_t)(m.w[GROW_PLANE] >> 32) == 1u && m.w[AROW_AGGR] == 12, "sums add up: last becomes first");
    // ... and through a wrap: group 1 is best in both lists and wraps to the worst
    std::vector<Match> a = {{0, 1u, 1, {0x80000000u}}, {1, 2u, 1, {7}}}, b = {{10, 1u, 1, {0x80000001u}}, {11, 2u, 1, {7}}};
    const Row ra = row_of(a, MRK_GROUPSORT_KEY, 1, 4, {SUM32}, 0), rb = row_of(b, MRK_GROUPSORT_KEY, 1, 4, {SUM32}, 0);
    CHECK((uint32_t)(ra.w[GROW_PLANE] >> 32) == 1u && (uint32_t)(rb.w[GROW_PLANE] >> 32) == 1u, "group 1 is first in both lists");
    const Row w = merge({ra, rb}, 4);
    CHECK((uint32_t)(w.w[GROW_PLANE] >> 32) == 2u && w.w[AROW_AGGR] == 14 && w.w[AROW_AGGR + 1] == 1, "the sum wraps to 1: first becomes last");
    n_edges += 2;
  }

  // ---- hostile rows, in list 0 / a middle list / the last
  unsigned n_hostile = 0;
  {
    auto ms_of = [](uint32_t shard) {
      std::vector<Match> ms;
      for (uint32_t i = 0; i < 40; ++i) ms.push_back({shard * 100 + i, shard * 1000 + i % 5, 7, {i, i}});
      return ms;
    };
    const std::vector<Kind> kinds = {SUM32, MAX64};
    const Row a = row_of(ms_of(0), 0, 1, 4, kinds, 0), b = row_of(ms_of(1), 0, 1, 4, kinds, 0), c = row_of(ms_of(2), 0, 1, 4, kinds, 0);
    const uint64_t spec = a.w[AROW_GSPEC], aspec = a.w[AROW_ASPEC];
    CHECK(aspec == good2 && merge({a, b, c}, 4).w[GROW_TOTAL] == 15, "the three lists answer");
    auto everywhere = [&](const char* what, const Row& h) {
      CHECK(empty_declined(merge({h, b, c}, 4), b.w[AROW_GSPEC], aspec) && empty_declined(merge({a, h, c}, 4), spec, aspec) && empty_declined(merge({a, b, h}, 4), spec, aspec), "%s", what);
      CHECK(empty_declined(merge({h, h}, 4), 0, 0), "%s: alone", what);
      ++n_hostile;
    };
    Row h = b;
    h.w[GROW_CNT] = G + 1;
    everywhere("entry count > G", h);
    h.w[GROW_CNT] = ~0ull;
    everywhere("entry count 2^64 - 1", h);
    for (uint64_t bad : bad_aspecs) {
      h = b, h.w[AROW_ASPEC] = bad;
      everywhere("a bad aggregate spec", h);
    }
    h = b, h.w[AROW_GSPEC] = group_spec_word(MRK_GROUPSORT_COUNT, 1, 32, 4); // the order's sort_by must be the key
    everywhere("an order next to sort_by @count", h);
    h = b, h.w[AROW_GSPEC] = 0;
    everywhere("an aggregate spec over group spec 0", h);
    h = b, h.w[AROW_GSPEC] = spec | (1ull << 40);
    everywhere("a group spec that does not unpack", h);
    // counts past 2^32 - 1 decline under both spec words
    Row x = a, y = a;
    x.w[GROW_PLANE] = (x.w[GROW_PLANE] & ~0xFFFFFFFFull) | 0xFFFFFFF0ull, y.w[GROW_PLANE] = (y.w[GROW_PLANE] & ~0xFFFFFFFFull) | 0x10ull;
    CHECK(empty_declined(merge({x, y}, 4), spec, aspec), "a count of 2^32");
    y.w[GROW_PLANE] -= 1;
    CHECK(merge({x, y}, 4).w[GROW_TOTAL] == 5, "a count of 2^32 - 1");
  }

  // ---- flags and specs
  {
    auto ms_of = [](uint32_t shard, uint32_t n) {
      std::vector<Match> ms;
      for (uint32_t i = 0; i < 40; ++i) ms.push_back({shard * 100 + i, shard * 1000 + i % n, 7, {i, i, i}});
      return ms;
    };
    const std::vector<Kind> kinds = {MIN32, SUMW, SUM64};
    const Row a = row_of(ms_of(0, 6), 2, 0, 4, kinds, -1), b = row_of(ms_of(1, 5), 2, 0, 4, kinds, -1), b6 = row_of(ms_of(1, 6), 2, 0, 4, kinds, -1), c = row_of(ms_of(2, 5), 2, 0, 4, kinds, -1);
    const uint64_t spec = a.w[AROW_GSPEC], aspec = a.w[AROW_ASPEC];
    CHECK(merge({a, b, c}, 4).w[GROW_TOTAL] == 16, "6 + 5 + 5 = 16 answered");
    CHECK(empty_declined(merge({a, b6, c}, 4), spec, aspec) && empty_declined(merge({merge({a, b6}, 4), c}, 4), spec, aspec), "6 + 6 + 5 = 17 declined, both spec words kept, staged too");
    CHECK(empty_declined(merge({a, b, c}, 3), spec, aspec), "max_matches above the call's k");
    Row rr;
    rr.w[AROW_GSPEC] = spec, rr.w[AROW_ASPEC] = aspec, rr.w[GROW_TOTAL] = MRK_ROW_RERUN;
    Row dd;
    dd.w[GROW_TOTAL] = MRK_ROW_DECLINED; // a shard whose planner declined: spec words 0, no say
    Row own;
    own.w[AROW_GSPEC] = spec, own.w[AROW_ASPEC] = aspec, own.w[GROW_TOTAL] = MRK_ROW_DECLINED; // declined while it ran: keeps its say
    for (const std::vector<Row>& l : {std::vector<Row>{rr, a, b}, {a, rr, b}, {a, b, rr}}) CHECK(empty_under(merge(l, 4), MRK_ROW_RERUN, spec, aspec), "a list with RERUN");
    for (const std::vector<Row>& l : {std::vector<Row>{dd, a, b}, {a, dd, b}, {a, b, dd}}) CHECK(empty_declined(merge(l, 4), spec, aspec), "a list declined under spec 0");
    for (const std::vector<Row>& l : {std::vector<Row>{own, a, b}, {a, own, b}, {a, b, own}}) CHECK(empty_declined(merge(l, 4), spec, aspec), "a list declined under its own specs");
    CHECK(empty_under(merge({rr, dd, a}, 4), FLAGS, spec, aspec), "RERUN and DECLINED");
    CHECK(empty_declined(merge({dd, dd}, 4), 0, 0), "every list declined");
    // aggregate spec words that differ in one bit (func, width, n, order), and "with aggregates" next to "without"
    const uint64_t others[] = {aspec ^ (1ull << 8), aspec ^ (1ull << 15), aspec_of({MIN32, SUMW}, -1), 0ull};
    for (uint64_t other : others) {
      Row o = b;
      o.w[AROW_ASPEC] = other;
      uint64_t t, sp, asp;
      (void)aggr_row_head(o.w, t, sp, asp);
      CHECK(sp == spec && asp == other, "the other spec reads as written");
      CHECK(empty_declined(merge({a, o, c}, 1024), spec, aspec) && empty_declined(merge({o, a, c}, 1024), spec, other) && empty_declined(merge({a, c, o}, 1024), spec, aspec),
            "aggregate spec %llx next to %llx: the first answering list's", (unsigned long long)other, (unsigned long long)aspec);
    }
    Row rel;
    rel.w[0] = make_key(5, 1), rel.w[GROW_CNT] = 1, rel.w[GROW_TOTAL] = 1;
    CHECK(empty_declined(merge({a, rel}, 4), spec, aspec) && empty_declined(merge({rel, a}, 4), 0, 0), "grouped next to spec 0");
    // a grouped query without aggregates: the group rows' merge under zero planes
    const Row p = row_of(ms_of(0, 6), 1, 1, 4, {}, -1), r2 = row_of(ms_of(1, 5), 1, 1, 4, {}, -1);
    const Row m = merge({p, r2}, 4);
    bool planes_zero = true;
    for (int i = AROW_AGGR; i < AROW_GSPEC; ++i) planes_zero = planes_zero && m.w[i] == 0;
    CHECK(m.w[GROW_TOTAL] == 11 && m.w[AROW_ASPEC] == 0 && planes_zero, "no aggregates: zero planes, aggregate spec 0");
  }

  if (g_bad) {
    printf("%d checks failed\n", g_bad);
    return 1;
  }
  printf("ok aggr merge specs %u merges %u edges %u hostile %u\n", n_spec, n_merged, n_edges, n_hostile);
  return 0;
}
