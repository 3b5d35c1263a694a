// group_plan.cpp -- the planner's group stage (csrc/mrk_plan.cpp: resolve_group / reserve_group) on the host, under
// AddressSanitizer + UBSan: the DevQuery words of a grouped query, the table offsets of several grouped queries in one batch, the
// slot count per K, every plan-time decline with its message, hostile specs refused before a row is read, the decline mask (all
// three row formats), and an ungrouped batch planned to the same bytes as through the old signature.
// Built and run by tests/test_group_cpu.py; no GPU, no libmrk.so (the segment is a host-side stand-in as in order_plan.cpp).
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
  static_assert(sizeof(mrk_group) == 16 && offsetof(mrk_group, bit_offset) == 0 && offsetof(mrk_group, bit_count) == 4 && offsetof(mrk_group, sort_by) == 8 && offsetof(mrk_group, desc) == 12, "mrk_group");
  static_assert(offsetof(mrk_result, group_key) == offsetof(mrk_result, order_key) + sizeof(void*) && offsetof(mrk_result, group_count) == offsetof(mrk_result, group_key) + sizeof(void*), "behind order_key");
  static_assert(MRK_GROUPSORT_KEY == 0 && MRK_GROUPSORT_COUNT == 1 && MRK_GROUPSORT_WEIGHT == 2, "sort_by values");

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

  // ---- accepted: the words of the descriptor, the tables laid end to end in one batch, no candidates, routed off the bitmap kernels
  const int ks[] = {1, 2, 4, 20, 1000, 1024};
  const uint32_t want_slots[] = {16, 32, 64, 256, 8192, 16384};
  const mrk_group specs[] = {{0, 32, MRK_GROUPSORT_KEY, 1}, {32 + 3, 5, MRK_GROUPSORT_COUNT, 0}, {32 + 31, 1, MRK_GROUPSORT_WEIGHT, 1}, {32, 32, MRK_GROUPSORT_WEIGHT, 0}};
  int n_acc = 0;
  {
    mrk::BatchPlan plan;
    uint64_t expect_off = 0;
    uint32_t qi = 0;
    for (const Shape& sh : shapes)
      for (size_t ki = 0; ki < sizeof ks / sizeof *ks; ++ki)
        for (const mrk_group& g : specs) {
          Q q;
          make_query(q, sh.t, sh.n, sh.op, sh.ranker, ks[ki]);
          DevQuery dq;
          const uint64_t cand_before = plan.cand_total, sort_before = plan.sort_total;
          const size_t bm_before = plan.items_bm.size();
          const int rc = mrk::plan_query(&S, q.q, 128 << 10, true, dq, 1000, qi++, plan, 0xFFFFFFFFu, &g);
          CHECK(rc == MRK_OK, "accepted shape declined: n %d op %d ranker %d k %d: %s", sh.n, sh.op, sh.ranker, ks[ki], g_err);
          if (rc != MRK_OK) continue;
          ++n_acc;
          CHECK(dq.grp_on == 1 && dq.grp_item == (uint32_t)g.bit_offset / 32 && dq.grp_shift == (uint32_t)g.bit_offset % 32 && dq.grp_bits == (uint32_t)g.bit_count, "locator words");
          CHECK(dq.grp_sort_by == (uint32_t)g.sort_by && dq.grp_desc == (uint32_t)g.desc && dq.grp_pad == 0, "order words");
          CHECK(dq.grp_slots == want_slots[ki] && dq.grp_slots == mrk::group_slots_for((uint32_t)ks[ki]), "k %d: %u slots", ks[ki], dq.grp_slots);
          CHECK(dq.grp_off == expect_off, "table offset %llu, expected %llu", (unsigned long long)dq.grp_off, (unsigned long long)expect_off);
          expect_off += mrk::group_table_words(dq.grp_slots);
          CHECK(plan.group_total == expect_off, "arena total");
          CHECK(dq.cand_cap == 0 && dq.sort_cap == 0 && dq.sort_on == 0 && plan.cand_total == cand_before && plan.sort_total == sort_before, "a grouped query publishes no candidates");
          CHECK(plan.items_bm.size() == bm_before && !(dq.tree_flags & (mrk::TF_BITMAP | mrk::TF_BTREE)), "a grouped query runs on the block scan");
          for (const DevQuery& e : plan.extra)
            if (e.out_q == dq.out_q) CHECK(e.grp_on == 1 && e.grp_off == dq.grp_off && e.grp_slots == dq.grp_slots && e.grp_item == dq.grp_item, "a tree's further passes share the table");
        }
  }

  // ---- an ungrouped query: the same bytes as through the old signature, group words zero
  for (const Shape& sh : shapes) {
    Q qa, qb;
    make_query(qa, sh.t, sh.n, sh.op, sh.ranker, 20), make_query(qb, sh.t, sh.n, sh.op, sh.ranker, 20);
    mrk::BatchPlan pa, pb;
    DevQuery da, db;
    const int ra = mrk::plan_query(&S, qa.q, 128 << 10, true, da, 1, 0, pa), rb = mrk::plan_query(&S, qb.q, 128 << 10, true, db, 1, 0, pb, 0xFFFFFFFFu, nullptr);
    CHECK(ra == MRK_OK && rb == MRK_OK && !memcmp(&da, &db, sizeof da), "NULL group differs from the old signature");
    CHECK(pa.extra.size() == pb.extra.size() && (pa.extra.empty() || !memcmp(pa.extra.data(), pb.extra.data(), pa.extra.size() * sizeof(DevQuery))), "passes differ");
    CHECK(pa.group_total == 0 && pb.group_total == 0 && pa.cand_total == pb.cand_total, "no table for an ungrouped query");
    CHECK(da.grp_on == 0 && da.grp_item == 0 && da.grp_shift == 0 && da.grp_bits == 0 && da.grp_sort_by == 0 && da.grp_desc == 0 && da.grp_slots == 0 && da.grp_pad == 0 && da.grp_off == 0, "group words of an ungrouped query");
  }

  // ---- declined, with a message
  mrk_segment bare = S;
  bare.dev.attrs = nullptr, bare.h_attrs.clear(), bare.sort_ranges.clear();
  const mrk_sort a_sort{MRK_SORTKEY_INT, 0, 32, 1, 1};
  mrk_order an_order;
  memset(&an_order, 0, sizeof an_order);
  an_order.n_parts = 2, an_order.parts[0] = mrk_order_part{MRK_SORTKEY_INT, 0, 32, 1}, an_order.parts[1] = mrk_order_part{MRK_SORTKEY_INT, 32, 32, 0};
  struct Dec { mrk_group g; bool packed; int cutoff; const mrk_segment* seg; const mrk_sort* sort; const mrk_order* order; int want; const char* what; };
  const Dec decs[] = {
      {{0, 32, 0, 1}, true, 0, &S, &a_sort, nullptr, MRK_E_UNSUPPORTED, "next to mrk_query.sort"},
      {{0, 32, 0, 1}, true, 0, &S, nullptr, &an_order, MRK_E_UNSUPPORTED, "next to mrk_query.sort"},
      {{0, 32, 0, 1}, true, 7, &S, nullptr, nullptr, MRK_E_UNSUPPORTED, "cutoff next to a group"},
      {{-1, 0, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_UNSUPPORTED, "blob-stored"},
      {{-5, 32, 0, 1}, true, 0, &bare, nullptr, nullptr, MRK_E_UNSUPPORTED, "blob-stored"},
      {{64, 64, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_UNSUPPORTED, "64-bit attribute"},
      {{0, 32, 0, 1}, true, 0, &bare, nullptr, nullptr, MRK_E_UNSUPPORTED, "attribute rows"},
      {{0, 32, 0, 1}, false, 0, &S, nullptr, nullptr, MRK_E_UNSUPPORTED, "packed path only"},
      // hostile specs: MRK_E_INVAL, before a row is read
      {{(int32_t)stride * 32, 32, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "outside the"},
      {{0x7FFFFFE0, 32, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "outside the"},
      {{30, 7, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "inside one dword"},
      {{0, 0, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "inside one dword"},
      {{0, 33, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "inside one dword"},
      {{0, -1, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "inside one dword"},
      {{96, 64, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "inside one dword"}, // 64 bits that leave the row
      {{40, 64, 0, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "inside one dword"}, // 64 unaligned bits
      {{0, 32, 3, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "sort_by"},
      {{0, 32, -1, 1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "sort_by"},
      {{0, 32, 0, 2}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "desc"},
      {{0, 32, 0, -1}, true, 0, &S, nullptr, nullptr, MRK_E_INVAL, "desc"},
  };
  for (const Dec& d : decs) {
    Q q;
    make_query(q, t2, 2, MRK_OP_AND, MRK_RANK_BM25, 20);
    q.q.sort = d.sort, q.q.order = d.order, q.q.cutoff = d.cutoff;
    mrk::BatchPlan plan;
    DevQuery dq;
    g_err[0] = 0;
    const int rc = mrk::plan_query(d.seg, q.q, 128 << 10, d.packed, dq, 1, 0, plan, d.cutoff ? 5000u : 0xFFFFFFFFu, &d.g);
    CHECK(rc == d.want && strstr(g_err, d.what), "decline %d/%d by %d desc %d: rc %d, message '%s' (wanted %d, '%s')", d.g.bit_offset, d.g.bit_count, d.g.sort_by, d.g.desc, rc, g_err, d.want, d.what);
    CHECK(plan.group_total == 0, "a declined query reserved a table");
  }

  // ---- the decline mask: a grouped query leaves in no row format
  const uint32_t all3 = (1u << mrk::ROWS_NARROW) | (1u << mrk::ROWS_WIDE) | (1u << mrk::ROWS_ORDER);
  CHECK(mrk::query_decline_mask(MRK_OK, 0, 0, false, true) == all3 && mrk::query_decline_mask(MRK_OK, 0, 0, true, true) == all3, "grouped: all three bits");
  CHECK(mrk::query_decline_mask(MRK_OK, 0, 0, false, false) == 0 && mrk::query_decline_mask(MRK_OK, 32, 0, false, false) == mrk::row_decline_mask(MRK_OK, 32, 0, false), "ungrouped: row_decline_mask");
  CHECK(mrk::query_decline_mask(MRK_E_UNSUPPORTED, 0, 0, false, false) == all3, "declined at plan time");

  if (g_bad) {
    printf("%d checks failed\n", g_bad);
    return 1;
  }
  printf("ok accepted %d declines %d\n", n_acc, (int)(sizeof decs / sizeof *decs));
  return 0;
}
