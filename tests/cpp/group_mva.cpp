// group_mva.cpp -- GROUP BY a multi-value attribute on the host, under AddressSanitizer + UBSan: the functions the kernels call
// (csrc/mrk_kgroup.h) over pools written from the blob row's definition (attribute.cpp:495-513: a length-size byte, the blob
// attributes' cumulative lengths in 1 / 2 / 4 bytes, their data back to back).
//   - blob_mva_span / blob_mva_value32: the three length classes; the MVA as attribute 0 of 1 and as 0, 1 and 2 of 3 next to a string
//     of odd length (so that the values are unaligned) and a 64-bit MVA; an empty MVA; an MVA that ends on the pool's last byte (every
//     pool is a heap block of exactly its size: a read past it is an ASan report);
//   - the expansion -- one group_update per stored value -- into a GroupSeqOps table against a std::map: 4 K and 4 K + 1 distinct
//     values for K = 1 and 2, over several docs and on one doc alone, duplicate stored values, the values 0 and 0xFFFFFFFF;
//   - the tie order as a plain comparator: GROUP / ORDER lines that tests/test_group_mva_cpu.py checks the numpy model against.
// Built and run by tests/test_group_mva_cpu.py; no GPU, no libmrk.so.
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

typedef std::vector<uint8_t> Bytes;
static Bytes u32s(const std::vector<uint32_t>& v) {
  Bytes b;
  for (uint32_t x : v)
    for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(x >> (8 * i)));
  return b;
}
// one blob row appended to `pool`; kind < 0: the class the data's size asks for (CalcBlobRowFlags, attribute.cpp:28-37)
static uint64_t add_blob_row(Bytes& pool, const std::vector<Bytes>& attrs, int kind = -1) {
  size_t total = 0;
  for (const Bytes& a : attrs) total += a.size();
  if (kind < 0) kind = total < 0xFF ? 0 : total < 0xFFFF ? 1 : 2;
  const int sz = kind == 0 ? 1 : kind == 1 ? 2 : 4;
  const uint64_t off = pool.size();
  pool.push_back((uint8_t)kind);
  size_t acc = 0;
  for (const Bytes& a : attrs) {
    acc += a.size();
    for (int i = 0; i < sz; ++i) pool.push_back((uint8_t)(acc >> (8 * i)));
  }
  for (const Bytes& a : attrs) pool.insert(pool.end(), a.begin(), a.end());
  return off;
}
// the pool as a heap block of exactly its size
struct Exact {
  uint8_t* p;
  explicit Exact(const Bytes& b) : p((uint8_t*)malloc(b.size() ? b.size() : 1)) { memcpy(p, b.data(), b.size()); }
  ~Exact() { free(p); }
};
static void check_span(const uint8_t* pool, uint64_t off, uint32_t id, uint32_t nblob, const std::vector<uint32_t>& want, const char* what) {
  const uint32_t row[4] = {0xDEADBEEFu, 7u, (uint32_t)off, (uint32_t)(off >> 32)};
  const MvaSpan s = blob_mva_span(pool, row, group_mva_word(32, id, nblob));
  CHECK(s.n == want.size(), "%s: %u values, wanted %zu", what, s.n, want.size());
  for (uint32_t i = 0; i < s.n && i < want.size(); ++i) CHECK(blob_mva_value32(s, i) == want[i], "%s: value %u = %u, wanted %u", what, i, blob_mva_value32(s, i), want[i]);
}

struct Doc {
  uint64_t key;
  std::vector<uint32_t> values;
};
struct Ref {
  uint32_t count;
  uint64_t head;
};
// every doc's values through the pool and the span into a table of K's size, against the map.  -> distinct values claimed
static uint32_t run_expansion(const std::vector<Doc>& docs, uint32_t K, const char* what) {
  Bytes pool(8, 0);
  std::vector<uint64_t> offs;
  for (const Doc& d : docs) offs.push_back(add_blob_row(pool, {u32s(d.values)}));
  Exact P(pool);
  const uint32_t S = group_slots_for(K);
  std::vector<uint64_t> words(group_table_words(S), 0ull);
  const GroupTable T = group_table_at(words.data(), S);
  std::map<uint32_t, Ref> ref;
  bool ok = true;
  for (size_t d = 0; d < docs.size(); ++d) {
    const uint32_t row[4] = {0u, 0u, (uint32_t)offs[d], (uint32_t)(offs[d] >> 32)};
    const MvaSpan s = blob_mva_span(P.p, row, group_mva_word(32, 0, 1));
    CHECK(s.n == docs[d].values.size(), "%s: doc %zu", what, d);
    for (uint32_t i = 0; i < s.n; ++i) {
      const uint32_t v = blob_mva_value32(s, i);
      ok = group_update<GroupSeqOps>(T, v, 1u, docs[d].key) && ok;
      Ref& r = ref[v];
      r.count += 1, r.head = std::max(r.head, docs[d].key);
    }
  }
  CHECK(ok, "%s: a table sized for K = %u filled up", what, K); // (2 (4 K + 1) slots: 4 K + 1 values fit, the selection declines by the count)
  CHECK(*T.claimed == ref.size(), "%s: %u claimed, %zu distinct", what, *T.claimed, ref.size());
  uint32_t seen = 0;
  for (uint32_t i = 0; i < S; ++i) {
    if (!T.keys[i]) continue;
    ++seen;
    const auto it = ref.find((uint32_t)T.keys[i]);
    CHECK((T.keys[i] & GRP_TAG) && it != ref.end() && it->second.count == T.counts[i] && it->second.head == T.heads[i], "%s: slot %u", what, i);
  }
  CHECK(seen == ref.size(), "%s: slots", what);
  return *T.claimed;
}

// the groups' order with the tie rule: the order key descending (group_order_key), then the smaller group value first
struct Grp {
  uint32_t value, count;
  int32_t weight;
  uint32_t rowid;
};
static bool group_before(const Grp& a, const Grp& b, uint32_t sort_by, uint32_t desc) {
  const uint64_t ka = group_order_key(sort_by, desc, a.value, a.count, make_key(a.weight, a.rowid)), kb = group_order_key(sort_by, desc, b.value, b.count, make_key(b.weight, b.rowid));
  if (ka != kb) return ka > kb;
  return a.value < b.value;
}

int main() {
  static_assert(sizeof(mrk_group_mva) == 12, "mrk_group_mva");
  int n_span = 0;
  // ---- spans.  Attribute 0 of 1, the three classes forced over the same small data, then the classes the sizes ask for
  for (int kind = 0; kind < 3; ++kind) {
    const std::vector<uint32_t> v = {0u, 5u, 5u, 0x80000000u, 0xFFFFFFFFu}; // (stored order, a duplicate: the span hands out what is stored)
    Bytes pool(8, 0);
    const uint64_t off = add_blob_row(pool, {u32s(v)}, kind);
    Exact P(pool); // (the MVA ends on the pool's last byte)
    check_span(P.p, off, 0, 1, v, "0 of 1, forced class"), ++n_span;
  }
  for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 16383u, 16384u}) { // 63 / 64 values: 252 / 256 bytes straddle 0xFF; 16383 / 16384: 0xFFFF
    std::vector<uint32_t> v;
    for (uint32_t i = 0; i < n; ++i) v.push_back(i * 2654435761u + n);
    Bytes pool(8, 0);
    add_blob_row(pool, {u32s({1u, 2u})});
    const uint64_t off = add_blob_row(pool, {u32s(v)});
    CHECK(pool[off] == (n * 4 < 0xFF ? 0 : n * 4 < 0xFFFF ? 1 : 2), "class of %u values", n);
    Exact P(pool);
    check_span(P.p, off, 0, 1, v, "0 of 1"), ++n_span;
  }
  // attribute 0, 1 and 2 of 3 next to a string of odd length and a 64-bit MVA, in every class; the other two may be empty
  for (int kind = 0; kind < 3; ++kind)
    for (uint32_t id = 0; id < 3; ++id)
      for (int variant = 0; variant < 3; ++variant) {
        const std::vector<uint32_t> v = variant == 1 ? std::vector<uint32_t>{} : std::vector<uint32_t>{7u, 0u, 0xFFFFFFFFu, 7u};
        const Bytes str = variant == 2 ? Bytes{} : Bytes{'a', 'b', 'c', 'd', 'e'};
        Bytes m64;
        for (int i = 0; i < (variant == 2 ? 0 : 16); ++i) m64.push_back((uint8_t)(0xF0 + i));
        std::vector<Bytes> attrs;
        for (uint32_t a = 0, other = 0; a < 3; ++a) attrs.push_back(a == id ? u32s(v) : (other++ ? m64 : str));
        Bytes pool(8, 0);
        add_blob_row(pool, {Bytes{1, 2, 3}, Bytes{}, Bytes{9}}, 0);
        const uint64_t off = add_blob_row(pool, attrs, kind);
        Exact P(pool); // (id == 2: the MVA is the row's last data, and the row the pool's)
        check_span(P.p, off, id, 3, v, "x of 3"), ++n_span;
      }
  // a row in the 4-byte class because of a 70 000-byte neighbour, its MVA of three values
  {
    const std::vector<uint32_t> v = {3u, 1u, 2u};
    Bytes pool(8, 0);
    const uint64_t off = add_blob_row(pool, {Bytes(70000, 0x55), u32s(v)});
    CHECK(pool[off] == 2, "the 4-byte class");
    Exact P(pool);
    check_span(P.p, off, 1, 2, v, "behind a long string"), ++n_span;
  }

  // ---- the expansion against a map
  int n_exp = 0;
  for (uint32_t K : {1u, 2u})
    for (uint32_t extra : {0u, 1u}) {
      const uint32_t nv = 4 * K + extra;
      std::vector<Doc> spread, alone(1);
      for (uint32_t d = 0; d < 3 * nv; ++d) // three docs per value, two values per doc, one of them stored twice
        spread.push_back(Doc{make_key(1000 + (int32_t)(d % 7), 100 + d), {(d % nv) * 0x01000193u, ((d + 1) % nv) * 0x01000193u, (d % nv) * 0x01000193u}});
      alone[0].key = make_key(5, 9);
      for (uint32_t j = 0; j < nv; ++j) alone[0].values.push_back(j ? 0xFFFFFFFFu - (j - 1) : 0u); // 0, 0xFFFFFFFF, 0xFFFFFFFE, ...
      const uint32_t a = run_expansion(spread, K, "spread"), b = run_expansion(alone, K, "one doc");
      CHECK(a == nv && b == nv, "K %u: %u / %u distinct of %u", K, a, b, nv);
      CHECK((a > group_limit(K)) == (extra != 0) && (b > group_limit(K)) == (extra != 0), "the limit at K %u", K);
      n_exp += 2;
    }
  { // an empty doc among others joins no group; 0 and 0xFFFFFFFF are ordinary values
    const std::vector<Doc> docs = {{make_key(3, 1), {}}, {make_key(3, 2), {0u, 0xFFFFFFFFu, 0u}}, {make_key(4, 3), {0xFFFFFFFFu}}, {make_key(1, 4), {}}};
    CHECK(run_expansion(docs, 1, "empties") == 2, "empties");
    ++n_exp;
  }

  // ---- the tie order
  const Grp groups[] = {{10, 1, 1500, 4}, {3, 1, 1500, 4}, {7, 2, 1500, 4}, {0, 2, 2000, 1}, {0xFFFFFFFFu, 2, 2000, 1}, {5, 2, 1500, 6}, {6, 1, 1700, 9}, {2, 3, 1700, 9}};
  for (const Grp& g : groups) printf("GROUP %u %u %d %u\n", g.value, g.count, g.weight, g.rowid);
  for (uint32_t by : {(uint32_t)MRK_GROUPSORT_KEY, (uint32_t)MRK_GROUPSORT_COUNT, (uint32_t)MRK_GROUPSORT_WEIGHT})
    for (uint32_t desc : {1u, 0u}) {
      std::vector<Grp> v(groups, groups + sizeof groups / sizeof groups[0]);
      std::sort(v.begin(), v.end(), [&](const Grp& a, const Grp& b) { return group_before(a, b, by, desc); });
      printf("ORDER %u %u", by, desc);
      for (const Grp& g : v) printf(" %u", g.value);
      printf("\n");
    }

  if (g_bad) {
    printf("%d checks failed\n", g_bad);
    return 1;
  }
  printf("ok spans %d expansions %d\n", n_span, n_exp);
  return 0;
}
