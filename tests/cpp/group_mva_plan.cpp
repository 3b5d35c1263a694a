// group_mva_plan.cpp -- the planner's stage for a group by a multi-value attribute (csrc/mrk_plan.cpp: resolve_group_mva /
// reserve_group) on the host, under AddressSanitizer + UBSan: the DevQuery words of every accepted mrk_group_mva (the MVA word in
// grp_pad, grp_item / grp_shift / grp_bits 0 / 0 / 32, the table a row attribute's group gets), every MRK_E_INVAL and
// MRK_E_UNSUPPORTED of include/mrk.h with its message, and a query without an mrk_group_mva planned word for word as through
// mrk_batch_submit_aggr's signature.
// Built and run by tests/test_group_mva_cpu.py; no GPU, no libmrk.so (the segment is a host-side stand-in as in group_plan.cpp).
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
  static_assert(sizeof(mrk_group_mva) == 12 && offsetof(mrk_group_mva, mva_bits) == 0 && offsetof(mrk_group_mva, blob_attr_id) == 4 && offsetof(mrk_group_mva, n_blob_attrs) == 8, "mrk_group_mva");
  static_assert(offsetof(DevQuery, grp_pad) + 4 == offsetof(DevQuery, grp_off) && offsetof(DevQuery, grp_pad) == offsetof(DevQuery, grp_slots) + 4, "the MVA word is the group's former padding");

  mrk_ctx ctx;
  mrk_segment S;
  static uint32_t dummy[16];
  static uint8_t dummy_pool[16];
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
  const uint32_t stride = 5; // [0..1] the id, [2..3] the blob row offset, [4] a category
  S.dev.attr_stride = stride;
  S.attr_rows = S.total_docs;
  S.h_attrs.assign((size_t)S.total_docs * stride, 0u);
  S.dev.blobs = dummy_pool;
  S.n_blob_attrs = 3;

  const int t1[] = {3}, t2[] = {0, 1}, tor[] = {2, 5};
  struct Shape { const int* t; int n, op, ranker; };
  const Shape shapes[] = {{t1, 1, MRK_OP_AND, MRK_RANK_BM25}, {t2, 2, MRK_OP_AND, MRK_RANK_BM25}, {tor, 2, MRK_OP_OR, MRK_RANK_BM25}, {t2, 2, MRK_OP_PHRASE, MRK_RANK_PROXIMITY_BM25},
                          {t2, 2, MRK_OP_AND, MRK_RANK_PROXIMITY_BM25}};
  // (the group's locator is ignored next to an mrk_group_mva: a blob-stored one, one outside the row and a hostile width all plan)
  const mrk_group groups[] = {{0, 32, MRK_GROUPSORT_KEY, 1}, {-1, 0, MRK_GROUPSORT_COUNT, 0}, {1 << 20, 77, MRK_GROUPSORT_WEIGHT, 1}};

  // ---- accepted
  int n_acc = 0;
  {
    mrk::BatchPlan plan;
    uint64_t expect_off = 0;
    uint32_t qi = 0;
    for (const Shape& sh : shapes)
      for (int k : {1, 20, 1024})
        for (const mrk_group& g : groups)
          for (int id = 0; id < 3; ++id) {
            Q q;
            make_query(q, sh.t, sh.n, sh.op, sh.ranker, k);
            const mrk_group_mva mv{32, id, 3};
            DevQuery dq;
            const int rc = mrk::plan_query(&S, q.q, 128 << 10, true, dq, 1000, qi++, plan, 0xFFFFFFFFu, &g, nullptr, &mv);
            CHECK(rc == MRK_OK, "accepted spec declined: %s", g_err);
            if (rc != MRK_OK) continue;
            ++n_acc;
            CHECK(dq.grp_on == 1 && dq.grp_item == 0 && dq.grp_shift == 0 && dq.grp_bits == 32, "locator words of an MVA group");
            CHECK(dq.grp_pad == (32u | ((uint32_t)id << 16) | (3u << 24)) && dq.grp_pad == mrk::group_mva_word(32, (uint32_t)id, 3), "the MVA word");
            CHECK(dq.grp_sort_by == (uint32_t)g.sort_by && dq.grp_desc == (uint32_t)g.desc && dq.grp_naggr == 0 && dq.grp_order_aggr == 0, "order words");
            CHECK(dq.grp_slots == mrk::group_slots_for((uint32_t)k) && dq.cand_cap == 0 && dq.sort_cap == 0 && dq.sort_on == 0, "the table of a row attribute's group");
            CHECK(dq.grp_off == expect_off, "table offset");
            expect_off += mrk::group_table_words(dq.grp_slots);
            CHECK(plan.group_total == expect_off, "arena total");
            for (const DevQuery& e : plan.extra)
              if (e.out_q == dq.out_q) CHECK(e.grp_on == 1 && e.grp_pad == dq.grp_pad && e.grp_off == dq.grp_off && e.grp_bits == 32, "a tree's further passes carry the MVA word");
          }
  }

  // ---- no mrk_group_mva: word for word the aggregates' signature
  for (const Shape& sh : shapes)
    for (const mrk_group* g : {(const mrk_group*)nullptr, &groups[0]}) {
      Q qa, qb;
      make_query(qa, sh.t, sh.n, sh.op, sh.ranker, 20), make_query(qb, sh.t, sh.n, sh.op, sh.ranker, 20);
      mrk::BatchPlan pa, pb;
      DevQuery da, db;
      const int ra = mrk::plan_query(&S, qa.q, 128 << 10, true, da, 1, 0, pa, 0xFFFFFFFFu, g, nullptr), rb = mrk::plan_query(&S, qb.q, 128 << 10, true, db, 1, 0, pb, 0xFFFFFFFFu, g, nullptr, nullptr);
      CHECK(ra == MRK_OK && rb == MRK_OK && !memcmp(&da, &db, sizeof da) && da.grp_pad == 0, "a NULL mrk_group_mva differs from the aggregates' signature");
      CHECK(pa.extra.size() == pb.extra.size() && (pa.extra.empty() || !memcmp(pa.extra.data(), pb.extra.data(), pa.extra.size() * sizeof(DevQuery))), "passes differ");
      CHECK(pa.group_total == pb.group_total && pa.cand_total == pb.cand_total, "totals");
    }

  // ---- declined, with a message
  mrk_segment no_pool = S, bare = S, narrow = S;
  no_pool.dev.blobs = nullptr, no_pool.n_blob_attrs = 0; // never set, or dropped by a later mrk_segment_set_attrs: the segment looks the same
  bare.dev.attrs = nullptr, bare.h_attrs.clear(), bare.sort_ranges.clear();
  narrow.dev.attr_stride = 3;
  const mrk_group by_key = groups[0], bad_sort{0, 32, 7, 1}, bad_desc{0, 32, MRK_GROUPSORT_KEY, 2};
  mrk_aggrs ag;
  memset(&ag, 0, sizeof ag);
  ag.n = 1, ag.order_by = -1, ag.a[0] = mrk_aggr{MRK_AGGR_SUM, MRK_SORTKEY_INT, 128, 32, 0};
  mrk_aggrs bad_ag = ag;
  bad_ag.a[0].func = 9;
  mrk_sort srt;
  memset(&srt, 0, sizeof srt);
  srt.kind = MRK_SORTKEY_INT, srt.bit_offset = 128, srt.bit_count = 32, srt.desc = 1, srt.then_weight = 1;
  struct Dec { mrk_group_mva m; const mrk_group* g; const mrk_aggrs* a; const mrk_segment* seg; bool packed; int cutoff; const mrk_sort* sort; int want; const char* what; };
  const Dec decs[] = {
      // MRK_E_INVAL before a row is read: the tests and the wording of the MVA filter
      {{0, 0, 3}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "MVA width 0"},
      {{16, 0, 3}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "MVA width 16"},
      {{-32, 0, 3}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "MVA width -32"},
      {{32, -1, 3}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "blob attribute -1 of 3"},
      {{32, 3, 3}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "blob attribute 3 of 3"},
      {{32, 0, 0}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "blob attribute 0 of 0"},
      {{32, 0, 256}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "blob attribute 0 of 256"},
      {{32, 0, 2}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "the segment's rows hold 3"},
      {{64, 1, 4}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "the segment's rows hold 3"}, // (not the segment's, in front of the 64-bit decline)
      {{32, 0, 3}, &by_key, nullptr, &narrow, true, 0, nullptr, MRK_E_INVAL, "hold no blob locator"},
      {{32, 0, 3}, nullptr, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "without a group"},
      {{32, 0, 3}, &bad_sort, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "sort_by 7"},
      {{32, 0, 3}, &bad_desc, nullptr, &S, true, 0, nullptr, MRK_E_INVAL, "desc 2"},
      {{32, 5, 3}, &by_key, nullptr, &no_pool, true, 0, nullptr, MRK_E_INVAL, "blob attribute 5 of 3"}, // (out of range whatever the segment holds)
      {{32, 0, 3}, &by_key, &bad_ag, &S, true, 0, nullptr, MRK_E_INVAL, "function 9"},                 // (hostile aggregates in front of the decline of aggregates)
      // MRK_E_UNSUPPORTED per query
      {{64, 1, 3}, &by_key, nullptr, &S, true, 0, nullptr, MRK_E_UNSUPPORTED, "64-bit MVA"},
      {{32, 0, 3}, &by_key, nullptr, &no_pool, true, 0, nullptr, MRK_E_UNSUPPORTED, "blob pool"},
      {{64, 0, 3}, &by_key, nullptr, &no_pool, true, 0, nullptr, MRK_E_UNSUPPORTED, "blob pool"},
      {{32, 0, 3}, &by_key, &ag, &S, true, 0, nullptr, MRK_E_UNSUPPORTED, "aggregates next to a group by an MVA"},
      // ... and everything that declines a group
      {{32, 0, 3}, &by_key, nullptr, &S, true, 0, &srt, MRK_E_UNSUPPORTED, "next to mrk_query.sort"},
      {{32, 0, 3}, &by_key, nullptr, &S, true, 5, nullptr, MRK_E_UNSUPPORTED, "cutoff next to a group"},
      {{32, 0, 3}, &by_key, nullptr, &S, false, 0, nullptr, MRK_E_UNSUPPORTED, "packed path only"},
  };
  int n_inval = 0, n_unsup = 0;
  for (const Dec& d : decs) {
    Q q;
    make_query(q, t2, 2, MRK_OP_AND, MRK_RANK_BM25, 20);
    q.q.cutoff = d.cutoff, q.q.sort = d.sort;
    mrk::BatchPlan plan;
    DevQuery dq;
    g_err[0] = 0;
    const int rc = mrk::plan_query(d.seg, q.q, 128 << 10, d.packed, dq, 1, 0, plan, 0xFFFFFFFFu, d.g, d.a, &d.m);
    CHECK(rc == d.want && strstr(g_err, d.what), "decline: rc %d, message '%s' (wanted %d, '%s')", rc, g_err, d.want, d.what);
    CHECK(plan.group_total == 0, "a declined query reserved a table");
    (d.want == MRK_E_INVAL ? n_inval : n_unsup)++;
  }
  { // a segment without attribute rows has no pool either (mrk_segment_set_blobs walks the rows): the pool's decline stands
    Q q;
    make_query(q, t2, 2, MRK_OP_AND, MRK_RANK_BM25, 20);
    mrk_segment nothing = bare;
    nothing.dev.blobs = nullptr, nothing.n_blob_attrs = 0;
    mrk::BatchPlan plan;
    DevQuery dq;
    const mrk_group_mva mv{32, 0, 3};
    CHECK(mrk::plan_query(&nothing, q.q, 128 << 10, true, dq, 1, 0, plan, 0xFFFFFFFFu, &by_key, nullptr, &mv) == MRK_E_UNSUPPORTED, "no rows, no pool");
    ++n_unsup;
  }
  // ---- the row kinds: a group's masks (GROUP rows carry it, the other kinds decline it); the spec word is a 32-bit key's
  const uint32_t all3 = (1u << mrk::ROWS_NARROW) | (1u << mrk::ROWS_WIDE) | (1u << mrk::ROWS_ORDER);
  CHECK(mrk::query_decline_mask(MRK_OK, 0, 0, false, true) == all3 && mrk::group_row_decline_bit(MRK_OK, 0, 0) == 0, "the masks of a grouped query");

  if (g_bad) {
    printf("%d checks failed\n", g_bad);
    return 1;
  }
  printf("ok accepted %d inval %d unsupported %d\n", n_acc, n_inval, n_unsup);
  return 0;
}
