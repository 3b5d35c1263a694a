// group_aggr_plan.cpp -- the planner's aggregate stage (csrc/mrk_plan.cpp: check_aggrs / decline_aggrs / reserve_group) on the host,
// under AddressSanitizer + UBSan: the DevQuery words of every accepted aggregate spec, the larger tables laid end to end in one batch,
// every MRK_E_INVAL and MRK_E_UNSUPPORTED of include/mrk.h with its message (hostile specs refused before a row is read, whatever
// the group is), the decline masks, and a query without aggregates planned to the same DevQuery group members and group_total as
// through mrk_batch_submit_grouped's signature.
// Built and run by tests/test_group_aggr_cpu.py; no GPU, no libmrk.so (the segment is a host-side stand-in as in group_plan.cpp).
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_host_int.h"

static char g_err[512];
int mrk_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
extern "C" const char* mrk_last_error(void) { return g_err; }
extern "C" float mrk_idf(int64_t docs, int64_t total, int plain, int normalized, int n_qwords, float boost) {
  if (docs <= 0 || total <= 0) return 0.0f;
  float v = plain ? logf((float)total / (float)docs) : logf((float)(total - docs + 1) / (float)docs);
  v /= 2.0f * logf((float)(1 + total));
  if (normalized && n_qwords > 0) v /= (float)n_qwords;
  return v * boost;
}

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

struct Q {
  std::vector<mrk_node> nodes;
  std::vector<int32_t> children;
  mrk_query q;
};
static void make_query(Q& out, const int* terms, int n, int op, int ranker, int k) {
  out.nodes.assign((size_t)n + (n > 1 ? 1 : 0), mrk_node{});
  out.children.clear();
  for (int i = 0; i < n; ++i) {
    mrk_node& N = out.nodes[(size_t)i];
    N.op = MRK_OP_TERM, N.term_id = terms[i], N.atom_pos = i + 1, N.field_mask = 0xFFFFFFFFu, N.boost = 1.0f;
    out.children.push_back(i);
  }
  if (n > 1) {
    mrk_node& N = out.nodes[(size_t)n];
    N.op = op, N.n_children = n, N.first_child = 0, N.field_mask = 0xFFFFFFFFu, N.boost = 1.0f;
  }
  memset(&out.q, 0, sizeof out.q);
  out.q.nodes = out.nodes.data(), out.q.n_nodes = (int32_t)out.nodes.size(), out.q.children = out.children.data(), out.q.root = (int32_t)out.nodes.size() - 1;
  out.q.ranker = ranker, out.q.max_matches = k, out.q.normalized_tfidf = 1;
}

int main() {
  static_assert(sizeof(mrk_group) == 16, "mrk_group keeps its size");
  static_assert(sizeof(mrk_aggr) == 20 && offsetof(mrk_aggr, func) == 0 && offsetof(mrk_aggr, kind) == 4 && offsetof(mrk_aggr, bit_offset) == 8 && offsetof(mrk_aggr, bit_count) == 12 && offsetof(mrk_aggr, flags) == 16, "mrk_aggr");
  static_assert(sizeof(mrk_aggrs) == 88 && offsetof(mrk_aggrs, n) == 0 && offsetof(mrk_aggrs, order_by) == 4 && offsetof(mrk_aggrs, a) == 8, "mrk_aggrs");
  static_assert(offsetof(DevQuery, grp_naggr) > offsetof(DevQuery, grp_off), "new descriptor words sit behind the existing ones");

  mrk_ctx ctx;
  mrk_segment S;
  static uint32_t dummy[16];
  S.ctx = &ctx;
  S.total_docs = 50000;
  S.n_fields = 3;
  S.has_packed = true;
  uint32_t blk = 0;
  for (int t = 0; t < 8; ++t) {
    HostTerm h;
    h.docs = (uint32_t)(S.total_docs / (uint64_t)(t + 2));
    h.hits = h.docs * 2, h.nblocks = (h.docs + 127) / 128, h.blk_first = blk, blk += h.nblocks;
    h.doclist_off = 1 + (uint64_t)t * 1000000, h.doclist_len = h.docs * 3ull, h.packed_bytes = h.docs * 2ull;
    h.last_rowid = (uint32_t)S.total_docs - 1 - (uint32_t)t;
    h.bm_off = (uint64_t)t * 4096, h.dir_off = (uint64_t)t * 64;
    S.terms.push_back(h);
  }
  S.dev.n_windows = (uint32_t)((S.total_docs + 2047) / 2048);
  S.dev.pk_attr = dummy, S.dev.pk_hit = dummy, S.dev.bm = dummy, S.dev.attrs = dummy;
  S.bitmaps_on = true;
  const uint32_t stride = 4; // [0] a category, [1] bit-fields, [2..3] a 64-bit attribute
  S.dev.attr_stride = stride;
  S.attr_rows = S.total_docs;
  S.h_attrs.assign((size_t)S.total_docs * stride, 0u);
  for (uint64_t r = 0; r < S.total_docs; ++r) S.h_attrs[r * stride] = (uint32_t)(r % 37), S.h_attrs[r * stride + 1] = (uint32_t)(r * 40503ull);

  const int t1[] = {3}, t2[] = {0, 1}, tor[] = {2, 5};
  struct Shape { const int* t; int n, op, ranker; };
  const Shape shapes[] = {{t1, 1, MRK_OP_AND, MRK_RANK_BM25}, {t2, 2, MRK_OP_AND, MRK_RANK_BM25}, {t2, 2, MRK_OP_AND, MRK_RANK_NONE}, {tor, 2, MRK_OP_OR, MRK_RANK_BM25}, {t2, 2, MRK_OP_PHRASE, MRK_RANK_PROXIMITY_BM25},
                          {t2, 2, MRK_OP_AND, MRK_RANK_PROXIMITY_BM25}};
  const mrk_group by_key{0, 32, MRK_GROUPSORT_KEY, 1}, by_count{32 + 3, 5, MRK_GROUPSORT_COUNT, 0};
  auto A = [](int func, int kind, int off, int cnt, int flags) { return mrk_aggr{func, kind, off, cnt, flags}; };
  auto list = [](int order_by, std::initializer_list<mrk_aggr> l) {
    mrk_aggrs a;
    memset(&a, 0, sizeof a);
    a.n = (int32_t)l.size(), a.order_by = order_by;
    int i = 0;
    for (const mrk_aggr& x : l)
      if (i < MRK_MAX_AGGRS) a.a[i++] = x;
    return a;
  };

  // ---- accepted: every func x source kind x widen, 1..4 per query, orders by a 32-bit aggregate
  struct Acc { mrk_aggrs a; const mrk_group* g; };
  std::vector<Acc> accs;
  for (int f : {MRK_AGGR_SUM, MRK_AGGR_MIN, MRK_AGGR_MAX}) {
    accs.push_back({list(-1, {A(f, MRK_SORTKEY_INT, 0, 32, 0)}), &by_key});
    accs.push_back({list(-1, {A(f, MRK_SORTKEY_INT, 32 + 9, 7, 0)}), &by_count});
    accs.push_back({list(-1, {A(f, MRK_SORTKEY_INT, 32 + 31, 1, MRK_AGGR_WIDEN)}), &by_count});
    accs.push_back({list(-1, {A(f, MRK_SORTKEY_INT64, 64, 64, 0)}), &by_key});
    accs.push_back({list(0, {A(f, MRK_SORTKEY_INT, 0, 32, 0)}), &by_key});
    accs.push_back({list(2, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT64, 64, 64, 0), A(MRK_AGGR_MAX, MRK_SORTKEY_INT, 0, 32, MRK_AGGR_WIDEN), A(f, MRK_SORTKEY_INT, 32, 5, 0), A(MRK_AGGR_MIN, MRK_SORTKEY_INT, 0, 32, 0)}), &by_key});
  }
  int n_acc = 0;
  {
    mrk::BatchPlan plan;
    uint64_t expect_off = 0;
    uint32_t qi = 0;
    for (const Shape& sh : shapes)
      for (int k : {1, 20, 1024})
        for (const Acc& ac : accs) {
          Q q;
          make_query(q, sh.t, sh.n, sh.op, sh.ranker, k);
          DevQuery dq;
          const int rc = mrk::plan_query(&S, q.q, 128 << 10, true, dq, 1000, qi++, plan, 0xFFFFFFFFu, ac.g, &ac.a);
          CHECK(rc == MRK_OK, "accepted spec declined: %s", g_err);
          if (rc != MRK_OK) continue;
          ++n_acc;
          CHECK(dq.grp_on == 1 && dq.grp_naggr == (uint32_t)ac.a.n && dq.grp_order_aggr == (uint32_t)(ac.a.order_by + 1) && dq.grp_pad == 0, "counts");
          for (int i = 0; i < MRK_MAX_AGGRS; ++i) {
            if (i >= ac.a.n) {
              CHECK(dq.grp_aggr_item[i] == 0 && dq.grp_aggr_op[i] == 0, "words behind the list");
              continue;
            }
            const mrk_aggr& g = ac.a.a[i];
            const uint32_t op = dq.grp_aggr_op[i];
            const bool s64 = g.kind == MRK_SORTKEY_INT64;
            CHECK(dq.grp_aggr_item[i] == (uint32_t)g.bit_offset / 32 && mrk::aggr_func(op) == (uint32_t)g.func && ((op & mrk::AGGR_SRC64) != 0) == s64 && ((op & mrk::AGGR_WIDEN) != 0) == ((g.flags & MRK_AGGR_WIDEN) != 0), "op word");
            CHECK(s64 || ((op & 31u) == (uint32_t)g.bit_offset % 32 && ((op >> 5) & 63u) == (uint32_t)g.bit_count), "locator in the op word");
            CHECK(mrk::aggr_result64(op) == (s64 || (g.flags & MRK_AGGR_WIDEN)), "result width");
          }
          CHECK(dq.grp_off == expect_off, "table offset");
          expect_off += mrk::group_table_words(dq.grp_slots) + (uint64_t)ac.a.n * dq.grp_slots;
          CHECK(plan.group_total == expect_off, "arena total: %d planes behind the table", ac.a.n);
          for (const DevQuery& e : plan.extra)
            if (e.out_q == dq.out_q)
              CHECK(e.grp_naggr == dq.grp_naggr && e.grp_order_aggr == dq.grp_order_aggr && !memcmp(e.grp_aggr_item, dq.grp_aggr_item, sizeof dq.grp_aggr_item) && !memcmp(e.grp_aggr_op, dq.grp_aggr_op, sizeof dq.grp_aggr_op),
                    "a tree's further passes carry the aggregates");
        }
  }

  // ---- no aggregates: the DevQuery, the passes and group_total of the grouped signature, aggregate words zero
  for (const Shape& sh : shapes)
    for (const mrk_group* g : {(const mrk_group*)nullptr, &by_key, &by_count}) {
      Q qa, qb;
      make_query(qa, sh.t, sh.n, sh.op, sh.ranker, 20), make_query(qb, sh.t, sh.n, sh.op, sh.ranker, 20);
      mrk::BatchPlan pa, pb;
      DevQuery da, db;
      const int ra = mrk::plan_query(&S, qa.q, 128 << 10, true, da, 1, 0, pa, 0xFFFFFFFFu, g), rb = mrk::plan_query(&S, qb.q, 128 << 10, true, db, 1, 0, pb, 0xFFFFFFFFu, g, nullptr);
      CHECK(ra == MRK_OK && rb == MRK_OK && !memcmp(&da, &db, sizeof da), "NULL aggregates differ from the grouped signature");
      CHECK(pa.extra.size() == pb.extra.size() && (pa.extra.empty() || !memcmp(pa.extra.data(), pb.extra.data(), pa.extra.size() * sizeof(DevQuery))), "passes differ");
      CHECK(pa.group_total == pb.group_total && pa.group_total == (g ? mrk::group_table_words(mrk::group_slots_for(20)) : 0ull) && pa.cand_total == pb.cand_total, "group_total");
      CHECK(da.grp_naggr == 0 && da.grp_order_aggr == 0 && da.grp_aggr_item[0] == 0 && da.grp_aggr_op[0] == 0 && da.grp_aggr_item[3] == 0 && da.grp_aggr_op[3] == 0, "aggregate words of a query without aggregates");
    }

  // ---- declined, with a message
  mrk_segment bare = S;
  bare.dev.attrs = nullptr, bare.h_attrs.clear(), bare.sort_ranges.clear();
  const mrk_group blob_group{-1, 0, MRK_GROUPSORT_KEY, 1}, bad_group{0, 32, 7, 1};
  const mrk_aggr ok32 = A(MRK_AGGR_SUM, MRK_SORTKEY_INT, 0, 32, 0);
  struct Dec { mrk_aggrs a; const mrk_group* g; const mrk_segment* seg; bool packed; int want; const char* what; };
  const Dec decs[] = {
      // MRK_E_UNSUPPORTED, each naming what it declines
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_FLOAT, 0, 32, 0)}), &by_key, &S, true, MRK_E_UNSUPPORTED, "SUM of a float"},
      {list(-1, {ok32, A(MRK_AGGR_MIN, MRK_SORTKEY_FLOAT, 32, 32, 0)}), &by_key, &S, true, MRK_E_UNSUPPORTED, "aggregate 1: MIN of a float"},
      {list(-1, {A(MRK_AGGR_MAX, MRK_SORTKEY_INT, -1, 0, 0)}), &by_key, &S, true, MRK_E_UNSUPPORTED, "MAX of a blob-stored"},
      {list(-1, {A(MRK_AGGR_MAX, MRK_SORTKEY_INT64, -3, 64, 0)}), &by_key, &S, true, MRK_E_UNSUPPORTED, "blob-stored"},
      {list(0, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT64, 64, 64, 0)}), &by_key, &S, true, MRK_E_UNSUPPORTED, "64-bit result"},
      {list(1, {ok32, A(MRK_AGGR_SUM, MRK_SORTKEY_INT, 0, 32, MRK_AGGR_WIDEN)}), &by_key, &S, true, MRK_E_UNSUPPORTED, "64-bit result"},
      // ... and what declines the group declines the query
      {list(-1, {ok32}), &blob_group, &S, true, MRK_E_UNSUPPORTED, "group by a blob-stored"},
      {list(-1, {ok32}), &by_key, &bare, true, MRK_E_UNSUPPORTED, "attribute rows"},
      {list(-1, {ok32}), &by_key, &S, false, MRK_E_UNSUPPORTED, "packed path only"},
      // hostile: MRK_E_INVAL before a row is read, whatever the group is
      {list(-1, {}), &by_key, &S, true, MRK_E_INVAL, "0 aggregates"},
      {list(-1, {ok32, ok32, ok32, ok32, ok32}), &by_key, &S, true, MRK_E_INVAL, "5 aggregates"},
      {list(-1, {ok32}), nullptr, &S, true, MRK_E_INVAL, "without a group"},
      {list(-1, {A(0, MRK_SORTKEY_INT, 0, 32, 0)}), &by_key, &S, true, MRK_E_INVAL, "function 0"},
      {list(-1, {A(4, MRK_SORTKEY_INT, 0, 32, 0)}), &by_key, &S, true, MRK_E_INVAL, "function 4"},
      {list(-1, {A(MRK_AGGR_SUM, 3, 0, 32, 0)}), &by_key, &S, true, MRK_E_INVAL, "source kind 3"},
      {list(-1, {A(MRK_AGGR_SUM, -1, 0, 32, 0)}), &by_key, &S, true, MRK_E_INVAL, "source kind -1"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT, 0, 32, 2)}), &by_key, &S, true, MRK_E_INVAL, "flags 0x2"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT64, 64, 64, MRK_AGGR_WIDEN)}), &by_key, &S, true, MRK_E_INVAL, "MRK_AGGR_WIDEN on a source"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_FLOAT, 0, 32, MRK_AGGR_WIDEN)}), &by_key, &S, true, MRK_E_INVAL, "MRK_AGGR_WIDEN on a source"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT, (int32_t)stride * 32, 32, 0)}), &by_key, &S, true, MRK_E_INVAL, "outside the"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT, 0x7FFFFFE0, 32, 0)}), &by_key, &S, true, MRK_E_INVAL, "outside the"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT, 30, 7, 0)}), &by_key, &S, true, MRK_E_INVAL, "inside one dword"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT, 0, 0, 0)}), &by_key, &S, true, MRK_E_INVAL, "inside one dword"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT, 0, 33, 0)}), &by_key, &S, true, MRK_E_INVAL, "inside one dword"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT, 64, 64, 0)}), &by_key, &S, true, MRK_E_INVAL, "inside one dword"}, // (a 64 needs kind INT64)
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_FLOAT, 0, 16, 0)}), &by_key, &S, true, MRK_E_INVAL, "32-bit attribute"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT64, 40, 64, 0)}), &by_key, &S, true, MRK_E_INVAL, "64 dword-aligned"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT64, 64, 32, 0)}), &by_key, &S, true, MRK_E_INVAL, "64 dword-aligned"},
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_INT64, 96, 64, 0)}), &by_key, &S, true, MRK_E_INVAL, "outside the"},
      {list(1, {ok32}), &by_key, &S, true, MRK_E_INVAL, "order_by 1 of 1"},
      {list(-2, {ok32}), &by_key, &S, true, MRK_E_INVAL, "order_by -2"},
      {list(0, {ok32}), &by_count, &S, true, MRK_E_INVAL, "next to group sort_by"},
      {list(-1, {A(9, MRK_SORTKEY_INT, 0, 32, 0)}), &blob_group, &S, true, MRK_E_INVAL, "function 9"}, // (in front of the group's own decline)
      {list(-1, {ok32}), &bad_group, &S, true, MRK_E_INVAL, "sort_by"},                              // (the group's own INVAL in front of the aggregates' declines)
      {list(-1, {A(MRK_AGGR_SUM, MRK_SORTKEY_FLOAT, 0, 32, 0)}), &bad_group, &S, true, MRK_E_INVAL, "sort_by"},
  };
  int n_inval = 0, n_unsup = 0;
  for (const Dec& d : decs) {
    Q q;
    make_query(q, t2, 2, MRK_OP_AND, MRK_RANK_BM25, 20);
    mrk::BatchPlan plan;
    DevQuery dq;
    g_err[0] = 0;
    const int rc = mrk::plan_query(d.seg, q.q, 128 << 10, d.packed, dq, 1, 0, plan, 0xFFFFFFFFu, d.g, &d.a);
    CHECK(rc == d.want && strstr(g_err, d.what), "decline: rc %d, message '%s' (wanted %d, '%s')", rc, g_err, d.want, d.what);
    CHECK(plan.group_total == 0, "a declined query reserved a table");
    (d.want == MRK_E_INVAL ? n_inval : n_unsup)++;
  }

  // ---- the decline masks are the group's (a query with aggregates gets the GROUP row's bit where the batch fills the masks)
  const uint32_t all3 = (1u << mrk::ROWS_NARROW) | (1u << mrk::ROWS_WIDE) | (1u << mrk::ROWS_ORDER);
  CHECK(mrk::query_decline_mask(MRK_OK, 0, 0, false, true) == all3 && mrk::group_row_decline_bit(MRK_OK, 0, 0) == 0, "the masks of a grouped query");

  if (g_bad) {
    printf("%d checks failed\n", g_bad);
    return 1;
  }
  printf("ok accepted %d inval %d unsupported %d\n", n_acc, n_inval, n_unsup);
  return 0;
}
