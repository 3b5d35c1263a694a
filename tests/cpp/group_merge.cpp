// group_merge.cpp -- the merge of GROUP rows (include/mrk.h: MRK_GROW_WORDS) restated sequentially over what merge_grows_kernel
// itself goes through -- csrc/mrk_kgroup.h: the row reader group_row_head, group_spec_unpack, group_update (with GroupSeqOps in the
// place of the device atomics), group_order_key, group_plane_word -- on the CPU under AddressSanitizer + UBSan.  Every input row
// and every table lives in a heap block of its EXACT size, so a read behind a row or a probe behind a table is a sanitizer report.
//   - random shards of one match set: the merged row equals a std::map's answer, and a staged merge equals the one-step merge
//   - the limit counted over ALL lists: 6 + 5 + 5 values answer at K = 4, 6 + 6 + 5 decline although every list is inside its limit
//   - hostile rows: an entry count above G, a spec word that does not unpack (a stray bit, sort_by 3, bit_count 0, max_matches 0 or
//     above MRK_MAX_K), counts that add up to more than 2^32 - 1: MRK_ROW_DECLINED and no entries, never an access outside a row
//   - RERUN, DECLINED, spec mismatches, a grouped list next to a spec-0 one; the spec word's pack / unpack round trip
// Built and run by tests/test_group_merge_cpu.py; no GPU, no libmrk.so.
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

static const uint64_t FLAGS = MRK_ROW_RERUN | MRK_ROW_DECLINED;

struct Row { // a heap block of exactly one row
  uint64_t* w;
  Row() { w = (uint64_t*)calloc(GROW_WORDS, 8); }
  Row(const Row& o) : Row() { memcpy(w, o.w, GROW_WORDS * 8); }
  Row& operator=(const Row& o) {
    memcpy(w, o.w, GROW_WORDS * 8);
    return *this;
  }
  ~Row() { free(w); }
  bool operator==(const Row& o) const { return memcmp(w, o.w, GROW_WORDS * 8) == 0; }
};

// The kernel's grouped path, one entry after another.  k: the call's k (sizes the table as the arena's stride does).
static Row merge(const std::vector<Row>& lists, uint32_t k) {
  Row out;
  uint64_t spec = 0, flags = 0;
  bool have_spec = false, mismatch = false;
  for (const Row& r : lists) {
    uint64_t t, sp;
    (void)group_row_head(r.w, t, sp);
    flags |= t & FLAGS;
    if (!group_row_has_say(t, sp)) continue;
    if (!have_spec) spec = sp, have_spec = true;
    mismatch = mismatch || sp != spec;
  }
  if (mismatch) flags |= MRK_ROW_DECLINED;
  out.w[GROW_SPEC] = spec;
  if (spec == 0) { // (the narrow merge is mrk_topk_merge_rows' and tested there: here only its flags)
    out.w[GROW_TOTAL] = flags;
    return out;
  }
  GroupSpec gs;
  if (!group_spec_unpack(spec, gs)) abort(); // (an answering list's spec unpacked in group_row_head)
  if (gs.k > k) flags |= MRK_ROW_DECLINED;
  if (!flags) {
    const uint32_t slots = group_slots_for(gs.k);
    uint64_t* mem = (uint64_t*)calloc((size_t)group_table_words(slots), 8); // exact size
    const GroupTable T = group_table_at(mem, slots);
    unsigned long long sum_in = 0, sum_out = 0;
    bool ok = true;
    for (const Row& r : lists) {
      uint64_t t, sp;
      const uint32_t c = group_row_head(r.w, t, sp);
      for (uint32_t i = 0; i < c; ++i) {
        const uint64_t pw = r.w[GROW_PLANE + i];
        ok = group_update<GroupSeqOps>(T, (uint32_t)(pw >> 32), (uint32_t)pw, r.w[i]) && ok;
        sum_in += (uint32_t)pw;
      }
    }
    if (!ok || *T.claimed > group_limit(gs.k) || *T.claimed > GRP_MAX_GROUPS)
      flags |= MRK_ROW_DECLINED;
    else {
      std::vector<std::pair<uint64_t, uint32_t>> ord;
      for (uint32_t i = 0; i < slots; ++i)
        if (T.keys[i]) ord.push_back({group_order_key(gs.sort_by, gs.desc, (uint32_t)T.keys[i], T.counts[i], T.heads[i]), i}), sum_out += T.counts[i];
      if (sum_out != sum_in)
        flags |= MRK_ROW_DECLINED; // a slot wrapped: it is short by 2^32
      else {
        std::sort(ord.begin(), ord.end(), [](const auto& a, const auto& b) { return a.first > b.first || (a.first == b.first && a.second < b.second); });
        for (size_t i = 0; i < ord.size(); ++i) {
          const uint32_t s = ord[i].second;
          out.w[i] = T.heads[s];
          out.w[GROW_PLANE + i] = group_plane_word((uint32_t)T.keys[s], T.counts[s]);
        }
        out.w[GROW_CNT] = out.w[GROW_TOTAL] = ord.size();
      }
    }
    free(mem);
  }
  if (flags) out.w[GROW_TOTAL] = flags;
  return out;
}

struct Match {
  uint32_t rowid, value;
  int32_t weight;
};
struct Grp {
  uint64_t head = 0;
  uint64_t count = 0;
};

// a list's row from its matches, written from the format's definition (a std::map, a comparator from the order's definition)
static Row row_of(const std::vector<Match>& ms, uint32_t sort_by, uint32_t desc, uint32_t k, std::map<uint32_t, Grp>* into = nullptr) {
  std::map<uint32_t, Grp> g;
  for (const Match& m : ms) {
    Grp& x = g[m.value];
    x.count++;
    x.head = std::max(x.head, make_key(m.weight, m.rowid));
    if (into) {
      Grp& y = (*into)[m.value];
      y.count++;
      y.head = std::max(y.head, make_key(m.weight, m.rowid));
    }
  }
  Row r;
  r.w[GROW_SPEC] = group_spec_word(sort_by, desc, 32, k);
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
  std::sort(es.begin(), es.end(), [&](const E& a, const E& b) {
    const int64_t pa = sort_by == MRK_GROUPSORT_COUNT ? (int64_t)a.g.count : sort_by == MRK_GROUPSORT_KEY ? (int64_t)a.v : (int64_t)key_weight(a.g.head);
    const int64_t pb = sort_by == MRK_GROUPSORT_COUNT ? (int64_t)b.g.count : sort_by == MRK_GROUPSORT_KEY ? (int64_t)b.v : (int64_t)key_weight(b.g.head);
    if (pa != pb) return desc ? pa > pb : pa < pb;
    return key_rowid(a.g.head) < key_rowid(b.g.head);
  });
  for (size_t i = 0; i < es.size(); ++i) r.w[i] = es[i].g.head, r.w[GROW_PLANE + i] = ((uint64_t)es[i].v << 32) | (uint32_t)es[i].g.count;
  r.w[GROW_CNT] = r.w[GROW_TOTAL] = es.size();
  return r;
}

static uint32_t rnd_state = 12345;
static uint32_t rnd() {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}

static bool empty_declined(const Row& r, uint64_t spec) {
  for (int i = 0; i < GROW_GROUPS; ++i)
    if (r.w[i] || r.w[GROW_PLANE + i]) return false;
  return r.w[GROW_CNT] == 0 && r.w[GROW_TOTAL] == MRK_ROW_DECLINED && r.w[GROW_SPEC] == spec;
}

int main() {
  // ---- the spec word
  unsigned n_spec = 0;
  for (uint32_t by = 0; by < 3; ++by)
    for (uint32_t desc = 0; desc < 2; ++desc)
      for (uint32_t bits : {1u, 7u, 31u, 32u})
        for (uint32_t k : {1u, 2u, 20u, 1023u, 1024u}) {
          GroupSpec gs;
          const uint64_t w = group_spec_word(by, desc, bits, k);
          CHECK(w != 0 && group_spec_unpack(w, gs) && gs.sort_by == by && gs.desc == desc && gs.bit_count == bits && gs.k == k, "spec round trip %u %u %u %u", by, desc, bits, k);
          ++n_spec;
        }
  {
    GroupSpec gs;
    const uint64_t good = group_spec_word(1, 1, 32, 20);
    const uint64_t bad[] = {0ull, good & ~1ull, good | (1ull << 4), good | (1ull << 27), good | (1ull << 63), group_spec_word(3, 0, 32, 20), group_spec_word(0, 0, 0, 20),
                            group_spec_word(0, 0, 33, 20), group_spec_word(0, 0, 32, 0), group_spec_word(0, 0, 32, 1025)};
    for (uint64_t b : bad) CHECK(!group_spec_unpack(b, gs), "spec %llx unpacked", (unsigned long long)b);
  }

  // ---- random shards against a std::map over all matches; staged == one step; all six orders; K in {1, 2, 4, 20}
  unsigned n_merged = 0;
  for (uint32_t K : {1u, 2u, 4u, 20u})
    for (uint32_t by = 0; by < 3; ++by)
      for (uint32_t desc = 0; desc < 2; ++desc)
        for (uint32_t card : {1u, 3u, 4u * K, 4u * K + 1u}) {
          const uint32_t S = 1 + rnd() % 8;
          std::vector<Row> lists;
          std::map<uint32_t, Grp> all;
          std::vector<Match> every;
          for (uint32_t s = 0; s < S; ++s) {
            std::vector<Match> ms;
            const uint32_t n = rnd() % 300;
            for (uint32_t i = 0; i < n; ++i) ms.push_back({s * 1000 + i, (rnd() % card) * 0x9E3779B1u, (int32_t)(rnd() % 5) - 2});
            every.insert(every.end(), ms.begin(), ms.end());
            lists.push_back(row_of(ms, by, desc, K, &all));
          }
          const Row got = merge(lists, 1024);
          const Row want = row_of(every, by, desc, K);
          CHECK(got == want, "K %u by %u desc %u card %u: merged row != the row of all matches", K, by, desc, card);
          CHECK((all.size() > 4 * (size_t)K) == (got.w[GROW_TOTAL] == MRK_ROW_DECLINED), "limit over all lists");
          Row acc = lists[0];
          for (uint32_t s = 1; s < S; ++s) acc = merge({acc, lists[s]}, 1024);
          if (S == 1) acc = merge({acc}, 1024);
          CHECK(acc == got, "K %u by %u desc %u card %u: staged != one step", K, by, desc, card);
          ++n_merged;
        }

  // ---- the limit is counted over all lists: shard-disjoint values, K = 4
  auto disjoint = [](uint32_t shard, uint32_t n) {
    std::vector<Match> ms;
    for (uint32_t i = 0; i < 40; ++i) ms.push_back({shard * 100 + i, shard * 1000 + i % n, 7});
    return ms;
  };
  {
    const Row a = row_of(disjoint(0, 6), 0, 1, 4), b5 = row_of(disjoint(1, 5), 0, 1, 4), b6 = row_of(disjoint(1, 6), 0, 1, 4), c = row_of(disjoint(2, 5), 0, 1, 4);
    CHECK(merge({a, b5, c}, 4).w[GROW_TOTAL] == 16 && merge({a, b5, c}, 4).w[GROW_CNT] == 16, "6 + 5 + 5 = 16 answered");
    CHECK(a.w[GROW_TOTAL] == 6 && b6.w[GROW_TOTAL] == 6 && empty_declined(merge({a, b6, c}, 4), a.w[GROW_SPEC]), "6 + 6 + 5 = 17 declined");
    CHECK(empty_declined(merge({merge({a, b6}, 4), c}, 4), a.w[GROW_SPEC]), "... at the last step of a staged merge");
    CHECK(empty_declined(merge({a, b5, c}, 3), a.w[GROW_SPEC]), "max_matches above the call's k");
  }

  // ---- hostile rows
  {
    const Row a = row_of(disjoint(0, 6), 1, 1, 4), b = row_of(disjoint(1, 5), 1, 1, 4);
    const uint64_t spec = a.w[GROW_SPEC];
    Row h = b;
    h.w[GROW_CNT] = GROW_GROUPS + 1; // an entry count past the row: no entry of it is read
    CHECK(empty_declined(merge({a, h}, 4), spec) && empty_declined(merge({h, a}, 4), spec), "entry count > G");
    h.w[GROW_CNT] = ~0ull;
    CHECK(empty_declined(merge({a, h}, 4), spec) && empty_declined(merge({h, a}, 4), spec), "entry count 2^64 - 1");
    h = b;
    const uint64_t bad_specs[] = {spec | (1ull << 5), spec | (1ull << 40), group_spec_word(3, 1, 32, 4), group_spec_word(1, 1, 0, 4), group_spec_word(1, 1, 32, 0), 2};
    for (uint64_t bad : bad_specs) {
      h.w[GROW_SPEC] = bad;
      CHECK(empty_declined(merge({a, h}, 4), spec) && empty_declined(merge({h, a}, 4), spec), "spec %llx", (unsigned long long)bad);
    }
    // counts: 2^32 - 1 is a count like any other, one more is declined -- never wrapped, never saturated
    Row x = a, y = a;
    x.w[GROW_PLANE] = (x.w[GROW_PLANE] & ~0xFFFFFFFFull) | 0xFFFFFFF0ull;
    y.w[GROW_PLANE] = (y.w[GROW_PLANE] & ~0xFFFFFFFFull) | 0xFull;
    const uint32_t v0 = (uint32_t)(a.w[GROW_PLANE] >> 32);
    Row m = merge({x, y}, 4);
    bool found = false;
    for (uint32_t i = 0; i < m.w[GROW_CNT]; ++i)
      if ((uint32_t)(m.w[GROW_PLANE + i] >> 32) == v0) found = (uint32_t)m.w[GROW_PLANE + i] == 0xFFFFFFFFu;
    CHECK(m.w[GROW_TOTAL] == 6 && found, "a count of 2^32 - 1");
    y.w[GROW_PLANE] += 1;
    CHECK(empty_declined(merge({x, y}, 4), spec) && empty_declined(merge({y, x}, 4), spec), "a count of 2^32");
    y.w[GROW_PLANE] |= 0xFFFFFFFFull;
    CHECK(empty_declined(merge({x, y, y, y, y, y, y, y}, 4), spec), "eight lists of huge counts");
  }

  // ---- flags and specs
  {
    const Row a = row_of(disjoint(0, 6), 2, 0, 4), b = row_of(disjoint(1, 5), 2, 0, 4);
    const uint64_t spec = a.w[GROW_SPEC];
    Row rr;
    rr.w[GROW_SPEC] = spec, rr.w[GROW_TOTAL] = MRK_ROW_RERUN; // a list that is being rerun: empty under the query's spec
    for (const std::vector<Row>& l : {std::vector<Row>{rr, a, b}, {a, rr, b}, {a, b, rr}}) {
      const Row m = merge(l, 4);
      CHECK(m.w[GROW_TOTAL] == MRK_ROW_RERUN && m.w[GROW_CNT] == 0 && m.w[GROW_SPEC] == spec && m.w[0] == 0 && m.w[GROW_PLANE] == 0, "a list with RERUN");
    }
    Row dd;
    dd.w[GROW_TOTAL] = MRK_ROW_DECLINED; // a shard whose planner declined: spec 0, no say
    for (const std::vector<Row>& l : {std::vector<Row>{dd, a, b}, {a, dd, b}, {a, b, dd}}) CHECK(empty_declined(merge(l, 4), spec), "a list with DECLINED");
    Row both = merge({rr, dd, a}, 4);
    CHECK(both.w[GROW_TOTAL] == FLAGS && both.w[GROW_CNT] == 0 && both.w[GROW_SPEC] == spec, "RERUN and DECLINED");
    const uint64_t others[] = {group_spec_word(1, 0, 32, 4), group_spec_word(2, 1, 32, 4), group_spec_word(2, 0, 32, 5), group_spec_word(2, 0, 31, 4)};
    for (uint64_t other : others) {
      Row o = b;
      o.w[GROW_SPEC] = other;
      CHECK(empty_declined(merge({a, o}, 1024), spec) && empty_declined(merge({o, a}, 1024), other), "spec mismatch: the first answering list's");
    }
    Row rel;
    rel.w[0] = make_key(5, 1), rel.w[GROW_CNT] = 1, rel.w[GROW_TOTAL] = 1;
    CHECK(empty_declined(merge({a, rel}, 4), spec) && empty_declined(merge({rel, a}, 4), 0), "grouped next to spec 0");
    CHECK(merge({dd, dd}, 4).w[GROW_TOTAL] == MRK_ROW_DECLINED && merge({dd, dd}, 4).w[GROW_SPEC] == 0, "every list declined");
  }

  if (g_bad) {
    printf("%d checks failed\n", g_bad);
    return 1;
  }
  printf("ok group merge specs %u merges %u\n", n_spec, n_merged);
  return 0;
}
