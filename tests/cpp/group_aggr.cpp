// group_aggr.cpp -- the group table's aggregate accumulators (csrc/mrk_kgroup.h: group_update with aggregates, aggr_map / aggr_unmap,
// aggr_source -- the functions the kernels call, under the sequential GroupSeqOps policy) on the CPU under AddressSanitizer + UBSan,
// against a std::map model written from the aggregates' definition (include/mrk.h).  The table lives in a heap block of its EXACT
// size (group_table_words(slots, n_aggr)): an accumulator one slot or one plane past the end is a sanitizer report.
//   - random values in random groups; all matches in one group; one match per group
//   - sources of 0 and of all ones (the mapped value of a MAX of 0, and of a MIN of all ones, equals the empty word)
//   - INT64_MIN / INT64_MAX (signed MIN / MAX whose mapped value is 0; sums that wrap in two's complement)
//   - a 32-bit SUM that wraps modulo 2^32 next to its widened twin that passes 2^32
//   - a 7-bit field between all-ones neighbours; an INT64 read as two dwords, low first
//   - a full table (4 K + 1 .. slots groups): every slot's accumulators still right, nothing written past a plane
//   - pushes combined first (the flush's per-wave combine: one update with the sum / the maximum of several mapped values)
//   - the three planes in front read unchanged by group_table_at, and group_table_words(slots) == group_table_words(slots, 0)
//   - group_order_key_aggr against @count's order
// Built and run by tests/test_group_aggr_cpu.py; no GPU, no libmrk.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include <hip/hip_runtime.h> // (the function qualifiers of mrk_kgroup.h; no HIP call is made)

#include "../../manticoresearch_amd/csrc/mrk_kgroup.h"

using namespace mrk;

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

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}

// an aggregate as the test states it, and its op word
struct Spec {
  uint32_t func, item, shift, bits;
  bool src64, widen;
  uint32_t op() const { return aggr_op_word(func, shift, src64 ? 0u : bits, src64, widen); }
};
// the model: the aggregate's value from the definition -- unsigned 32-bit wrap, 64-bit two's complement, unsigned / signed compare
struct Model {
  bool any = false;
  uint64_t v = 0;
  void push(const Spec& s, uint64_t src) {
    if (s.func == MRK_AGGR_SUM) {
      v = s.src64 || s.widen ? v + src : (uint64_t)(uint32_t)((uint32_t)v + (uint32_t)src);
    } else if (!any) {
      v = src;
    } else if (s.src64) {
      const int64_t a = (int64_t)v, b = (int64_t)src;
      v = (uint64_t)(s.func == MRK_AGGR_MIN ? (b < a ? b : a) : (b > a ? b : a));
    } else {
      v = s.func == MRK_AGGR_MIN ? (src < v ? src : v) : (src > v ? src : v);
    }
    any = true;
  }
};

struct Table {
  uint64_t* mem;
  size_t words;
  GroupTable T;
  Table(uint32_t slots, uint32_t n_aggr) {
    words = (size_t)group_table_words(slots, n_aggr);
    mem = (uint64_t*)calloc(words, 8); // exact size
    T = group_table_at(mem, slots);
  }
  ~Table() { free(mem); }
};

static const uint32_t STRIDE = 6; // [0] a 32-bit value | [1] a 7-bit field at bit 9 between ones | [2..3] an int64 | [4] zero | [5] all ones
static void make_row(uint32_t* row, uint32_t v32, uint32_t seven, int64_t v64) {
  row[0] = v32, row[1] = (0xFFFFFFFFu & ~(127u << 9)) | ((seven & 127u) << 9), row[2] = (uint32_t)(uint64_t)v64, row[3] = (uint32_t)((uint64_t)v64 >> 32), row[4] = 0u, row[5] = 0xFFFFFFFFu;
}

// n_rows rows dealt to n_groups groups, pushed `combine` at a time per group (1 = one update per match), all against the model
static void run(uint32_t K, uint32_t n_groups, uint32_t n_rows, const std::vector<Spec>& specs, int values, uint32_t combine, const char* what) {
  const uint32_t S = group_slots_for(K), na = (uint32_t)specs.size();
  Table t(S, na);
  uint32_t ops[MRK_MAX_AGGRS] = {0, 0, 0, 0};
  for (uint32_t a = 0; a < na; ++a) ops[a] = specs[a].op();
  std::map<uint32_t, std::vector<Model>> model;
  std::map<uint32_t, uint32_t> counts;
  struct Pending { uint32_t n = 0; uint64_t head = 0, mapped[MRK_MAX_AGGRS] = {0, 0, 0, 0}; };
  std::map<uint32_t, Pending> pend;
  auto flush = [&](uint32_t g, Pending& p) {
    if (!p.n) return;
    const bool ok = group_update<GroupSeqOps>(t.T, g, p.n, p.head, na, ops, p.mapped);
    CHECK(ok, "%s: update of group %u refused", what, g);
    p = Pending{};
  };
  for (uint32_t r = 0; r < n_rows; ++r) {
    const uint32_t g = (uint32_t)(rnd() % n_groups) * 0x9E3779B1u;
    uint32_t row[STRIDE];
    const uint64_t x = rnd();
    switch (values) {
      case 0: make_row(row, (uint32_t)x, (uint32_t)(x >> 32), (int64_t)rnd()); break;                             // random
      case 1: make_row(row, 0xF0000000u | (uint32_t)x, 127u, (int64_t)(0x7000000000000000ull | rnd())); break;    // sums that wrap
      case 2: make_row(row, 0u, 0u, r & 1 ? INT64_MIN : INT64_MAX); break;                                         // the extremes
      default: make_row(row, 0xFFFFFFFFu, 127u, r % 3 == 0 ? INT64_MIN : r % 3 == 1 ? INT64_MAX : -1); break;
    }
    Pending& p = pend[g];
    const uint64_t head = make_key((int32_t)(x % 7), r);
    for (uint32_t a = 0; a < na; ++a) {
      const uint64_t src = aggr_source(row, specs[a].item, ops[a]);
      // the source as the definition reads it, without aggr_source
      const uint64_t want_src = specs[a].src64 ? ((uint64_t)row[specs[a].item + 1] << 32) | row[specs[a].item]
                                               : specs[a].bits == 32 ? row[specs[a].item] : (row[specs[a].item] >> specs[a].shift) & ((1u << specs[a].bits) - 1u);
      CHECK(src == want_src, "%s: aggr_source %llx, row says %llx", what, (unsigned long long)src, (unsigned long long)want_src);
      auto& m = model[g];
      m.resize(na);
      m[a].push(specs[a], src);
      const uint64_t mp = aggr_map(ops[a], src);
      p.mapped[a] = !p.n ? mp : aggr_is_add(ops[a]) ? p.mapped[a] + mp : (mp > p.mapped[a] ? mp : p.mapped[a]);
    }
    p.head = !p.n || head > p.head ? head : p.head;
    ++p.n, ++counts[g];
    if (p.n >= combine) flush(g, p);
  }
  for (auto& kv : pend) flush(kv.first, kv.second);
  CHECK(*t.T.claimed == model.size(), "%s: claimed %u, groups %zu", what, *t.T.claimed, model.size());
  std::map<uint32_t, int> slot_of;
  for (uint32_t i = 0; i < S; ++i)
    if (t.T.keys[i]) slot_of[(uint32_t)t.T.keys[i]] = (int)i;
  for (auto& kv : model) {
    const int slot = slot_of.count(kv.first) ? slot_of[kv.first] : -1;
    CHECK(slot >= 0, "%s: group %u not in the table", what, kv.first);
    if (slot < 0) continue;
    CHECK(t.T.counts[slot] == counts[kv.first], "%s: count", what);
    for (uint32_t a = 0; a < na; ++a) {
      const uint64_t got = aggr_unmap(ops[a], t.T.aggr[(size_t)a * S + (uint32_t)slot]);
      CHECK(got == kv.second[a].v, "%s: aggregate %u (func %u src64 %d widen %d) of group %u: %llx, model %llx", what, a, specs[a].func, (int)specs[a].src64, (int)specs[a].widen,
            kv.first, (unsigned long long)got, (unsigned long long)kv.second[a].v);
      if (!aggr_result64(ops[a])) CHECK((got >> 32) == 0, "%s: a 32-bit result is zero-extended", what);
    }
  }
  // an empty slot's accumulators were never touched
  for (uint32_t i = 0; i < S; ++i)
    if (!t.T.keys[i])
      for (uint32_t a = 0; a < na; ++a) CHECK(t.T.aggr[(size_t)a * S + i] == 0, "%s: accumulator of an empty slot", what);
}

int main() {
  static_assert(MRK_AGGR_SUM == 1 && MRK_AGGR_MIN == 2 && MRK_AGGR_MAX == 3 && MRK_AGGR_WIDEN == 1 && MRK_MAX_AGGRS == 4, "constants");
  static_assert(sizeof(mrk_aggr) == 20 && sizeof(mrk_aggrs) == 8 + 4 * 20, "mrk_aggr / mrk_aggrs");
  for (uint32_t k : {1u, 2u, 20u, 1024u}) {
    const uint32_t S = group_slots_for(k);
    CHECK(group_table_words(S) == group_table_words(S, 0) && group_table_words(S) == 1ull + 2ull * S + S / 2u, "the table without aggregates keeps its size");
    CHECK(group_table_words(S, 3) == group_table_words(S) + 3ull * S, "one plane of S words per aggregate");
    std::vector<uint64_t> block((size_t)group_table_words(S, 1));
    uint64_t* base = block.data();
    const GroupTable T = group_table_at(base, S);
    CHECK((uint64_t*)T.claimed == base && T.keys == base + 1 && T.heads == base + 1 + S && (uint64_t*)T.counts == base + 1 + 2ull * S && T.aggr == base + group_table_words(S), "planes");
  }
  const Spec sum32{MRK_AGGR_SUM, 0, 0, 32, false, false}, sum32w{MRK_AGGR_SUM, 0, 0, 32, false, true}, min32{MRK_AGGR_MIN, 0, 0, 32, false, false}, max32{MRK_AGGR_MAX, 0, 0, 32, false, false};
  const Spec sum7{MRK_AGGR_SUM, 1, 9, 7, false, false}, min7{MRK_AGGR_MIN, 1, 9, 7, false, false}, max7w{MRK_AGGR_MAX, 1, 9, 7, false, true}, min32w{MRK_AGGR_MIN, 0, 0, 32, false, true};
  const Spec sum64{MRK_AGGR_SUM, 2, 0, 64, true, false}, min64{MRK_AGGR_MIN, 2, 0, 64, true, false}, max64{MRK_AGGR_MAX, 2, 0, 64, true, false};
  const Spec min0{MRK_AGGR_MIN, 4, 0, 32, false, false}, max0{MRK_AGGR_MAX, 4, 0, 32, false, false}, minF{MRK_AGGR_MIN, 5, 0, 32, false, false}, maxF{MRK_AGGR_MAX, 5, 0, 32, false, false};
  const std::vector<std::vector<Spec>> lists = {{sum32}, {sum32, sum32w, min32, max32}, {sum7, min7, max7w, min32w}, {sum64, min64, max64}, {min0, max0, minF, maxF}, {sum64, sum32w, max64, min7}};
  int n_runs = 0;
  for (const auto& specs : lists)
    for (int values = 0; values < 4; ++values)
      for (uint32_t combine : {1u, 5u, 1000000u}) {
        run(20, 64, 3000, specs, values, combine, "64 groups"), ++n_runs;
        run(20, 1, 500, specs, values, combine, "one group"), ++n_runs;
        run(1024, 4096, 4096, specs, values, combine, "about a match per group"), ++n_runs;
        run(1, group_slots_for(1), 400, specs, values, combine, "a full table"), ++n_runs; // 16 groups in 16 slots
      }
  // a table that is full refuses one more group and leaves every accumulator as it was
  {
    const uint32_t S = group_slots_for(1);
    Table t(S, 2);
    const uint32_t ops[2] = {sum32.op(), max64.op()};
    for (uint32_t g = 0; g < S; ++g) {
      const uint64_t mp[2] = {g + 1ull, aggr_map(ops[1], (uint64_t)g)};
      CHECK(group_update<GroupSeqOps>(t.T, g * 77u, 1, make_key(1, g), 2, ops, mp), "filling the table");
    }
    std::vector<uint64_t> before(t.mem, t.mem + t.words);
    const uint64_t mp[2] = {5, 5};
    CHECK(!group_update<GroupSeqOps>(t.T, 0xABCDEF01u, 1, make_key(1, 99), 2, ops, mp), "a full table took one more group");
    CHECK(!memcmp(before.data(), t.mem, t.words * 8), "a refused update changed the table");
  }
  // the order by a 32-bit aggregate is @count's order over the aggregate's value
  for (int i = 0; i < 1000; ++i) {
    const uint32_t v = (uint32_t)rnd() >> (rnd() % 32), desc = (uint32_t)(rnd() & 1);
    const uint64_t head = make_key((int32_t)(rnd() % 100), (uint32_t)rnd());
    CHECK(group_order_key_aggr(desc, v, head) == group_order_key(MRK_GROUPSORT_COUNT, desc, 0u, v, head), "group_order_key_aggr");
  }
  if (g_bad) {
    printf("%d checks failed\n", g_bad);
    return 1;
  }
  printf("ok runs %d\n", n_runs);
  return 0;
}
