// weight_first_plan.cpp -- the planner's answers (csrc/mrk_plan.cpp) for the weight in front of an order (mrk_order::then_weight =
// MRK_ORDER_WEIGHT_FIRST_DESC / _ASC; `wf` 1 / 2 below) on the host, under
// AddressSanitizer + UBSan: every accepted shape plans with the weight's bins, every refusal answers its code before a row is read,
// and an order without it plans what it planned before.  Built and run by tests/test_weight_first_cpu.py; no GPU, no
// libmrk.so (the segment is a host-side stand-in as in order_plan.cpp).
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_host_int.h"
#include "../../manticoresearch_amd/csrc/mrk_sortkey.h"

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

static uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

struct Q {
  std::vector<mrk_node> nodes;
  std::vector<int32_t> children;
  mrk_query q;
};
static void make_query(Q& out, const int* terms, int n, int op, int ranker) {
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
  out.q.ranker = ranker, out.q.max_matches = 1000, out.q.normalized_tfidf = 1;
}

static mrk_order order_of(int wf, int n_parts, mrk_order_part a = mrk_order_part{}, mrk_order_part b = mrk_order_part{}, int tie = 0) {
  mrk_order o;
  memset(&o, 0, sizeof o);
  o.n_parts = n_parts, o.parts[0] = a, o.parts[1] = b, o.then_weight = wf ? (MRK_ORDER_WEIGHT_FIRST | wf) : tie; // (wf outside 1..2: no value the header names)
  return o;
}

int main() {
  static_assert(sizeof(mrk_order) == 4 + 2 * 16 + 4 && MRK_ORDER_WEIGHT_FIRST_DESC == 0x101 && MRK_ORDER_WEIGHT_FIRST_ASC == 0x102, "mrk_order keeps its size: then_weight says where the weight stands");
  static_assert(sizeof(mrk::OrderGeom) == 16, "the bins' geometry keeps its size");
  static_assert(offsetof(DevQuery, wf_parts) > offsetof(DevQuery, ord_geom), "new descriptor words sit behind the existing ones");

  mrk_ctx ctx;
  mrk_segment S;
  static uint32_t dummy[16];
  S.ctx = &ctx;
  S.total_docs = 100000;
  S.n_fields = 3;
  S.has_packed = true;
  uint32_t blk = 0;
  for (int t = 0; t < 12; ++t) {
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
  // rows: [0] timestamps, [1] bit-fields, [2] floats, [3] floats with one NaN, [4..5] a signed 64-bit attribute, [6] a constant
  const uint32_t stride = 7;
  S.dev.attr_stride = stride;
  S.attr_rows = S.total_docs;
  S.h_attrs.resize((size_t)S.total_docs * stride);
  for (uint64_t r = 0; r < S.total_docs; ++r) {
    uint32_t* row = &S.h_attrs[r * stride];
    row[0] = 1700000000u + (uint32_t)((r * 2654435761ull) % 5000000ull);
    row[1] = (uint32_t)(r * 40503ull);
    row[2] = fbits((float)((int64_t)(r % 2001) - 1000) * 0.25f);
    row[3] = r == 777 ? 0x7FC00000u : row[2];
    const int64_t big = ((int64_t)r - 50000) * 1000003ll * 4099ll;
    row[4] = (uint32_t)(uint64_t)big, row[5] = (uint32_t)((uint64_t)big >> 32);
    row[6] = 42;
  }
  mrk_segment bare = S; // no attribute rows at all
  bare.dev.attrs = nullptr, bare.dev.attr_stride = 0, bare.h_attrs.clear(), bare.sort_ranges.clear();

  const int t1[] = {3}, t2[] = {0, 1}, t8[] = {0, 1, 2, 3, 4, 5, 6, 7}, tor[] = {2, 5};
  const int rankers[] = {MRK_RANK_NONE, MRK_RANK_BM25, MRK_RANK_PROXIMITY_BM25, MRK_RANK_SPH04};
  struct Shape { const int* t; int n, op; };
  const Shape shapes[] = {{t1, 1, MRK_OP_AND}, {t2, 2, MRK_OP_AND}, {t8, 8, MRK_OP_AND}, {tor, 2, MRK_OP_OR}, {t2, 2, MRK_OP_PHRASE}};
  const mrk_order_part TS{MRK_SORTKEY_INT, 0, 32, 1}, F5{MRK_SORTKEY_INT, 32 + 3, 5, 0}, FL{MRK_SORTKEY_FLOAT, 64, 32, 0}, I64D{MRK_SORTKEY_INT64, 4 * 32, 64, 1}, I64A{MRK_SORTKEY_INT64, 4 * 32, 64, 0};

  // ---- accepted: (one part | two parts | one INT64) x both weight directions, and weight ASC without parts
  std::vector<mrk_order> orders;
  for (int wf = 1; wf <= 2; ++wf) {
    for (const mrk_order_part& p : {TS, F5, FL, I64D, I64A}) orders.push_back(order_of(wf, 1, p));
    orders.push_back(order_of(wf, 2, TS, F5));
    orders.push_back(order_of(wf, 2, F5, FL));
    orders.push_back(order_of(wf, 2, FL, TS));
  }
  orders.push_back(order_of(2, 0));
  int n_acc = 0;
  for (const Shape& sh : shapes)
    for (int rk : rankers)
      for (const mrk_order& o : orders)
        for (const mrk_segment* seg : {(const mrk_segment*)&S, (const mrk_segment*)&bare}) {
          if (seg == &bare && o.n_parts) continue; // (declined below)
          Q q, qr;
          make_query(q, sh.t, sh.n, sh.op, rk);
          make_query(qr, sh.t, sh.n, sh.op, rk == MRK_RANK_NONE ? MRK_RANK_BM25 : rk);
          q.q.order = &o;
          mrk::BatchPlan plan, plan_r;
          DevQuery dq, dr;
          const int rc = mrk::plan_query(seg, q.q, 128 << 10, true, dq, 1, 0, plan);
          CHECK(rc == MRK_OK, "accepted shape declined: n %d op %d ranker %d parts %d kind %d wf %d: %s", sh.n, sh.op, rk, o.n_parts, o.parts[0].kind, o.then_weight & 3, g_err);
          if (rc != MRK_OK) continue;
          ++n_acc;
          CHECK(dq.sort_on == mrk::SORT_ON_WEIGHT && (dq.sort_flags & mrk::SORT_WFIRST) && !(dq.sort_flags & mrk::SORT_WIDE) && dq.sort_tie == (uint32_t)(o.then_weight & 3), "weight-first words");
          CHECK(dq.cand_cap == 0 && dq.sort_cap > 0 && plan.sort_total == dq.sort_cap && plan.cand_total == 0, "the 16-byte candidate arena");
          CHECK(!(dq.tree_flags & (mrk::TF_BITMAP | mrk::TF_BTREE)), "a weight-first query on a bitmap kernel");
          for (const DevItem& it : plan.items_bm) CHECK(it.kind == 2, "a weight-first query laid out as a scan_bm / scan_bt item");
          for (const DevQuery& P : plan.extra)
            CHECK(P.sort_on == dq.sort_on && P.sort_flags == dq.sort_flags && P.sort_tie == dq.sort_tie && P.wf_parts == dq.wf_parts && P.ord_item == dq.ord_item && P.ord_bits == dq.ord_bits, "pass without the order");
          const bool i64 = o.n_parts == 1 && o.parts[0].kind == MRK_SORTKEY_INT64;
          CHECK(dq.wf_parts == (i64 ? 2u : (uint32_t)o.n_parts), "wf_parts %u", dq.wf_parts);
          if (i64)
            CHECK(dq.sort_item == 5 && dq.ord_item == 4 && (dq.sort_flags & mrk::SORT_SIGNED) && !(dq.ord_flags & mrk::SORT_SIGNED) && dq.sort_bits == 32 && dq.ord_bits == 32 &&
                      ((dq.sort_flags & mrk::SORT_DESC) != 0) == (o.parts[0].desc != 0) && ((dq.ord_flags & mrk::SORT_DESC) != 0) == (o.parts[0].desc != 0),
                  "64-bit locator");
          else {
            if (o.n_parts >= 1)
              CHECK(dq.sort_item == (uint32_t)o.parts[0].bit_offset / 32 && dq.sort_shift == (uint32_t)o.parts[0].bit_offset % 32 && dq.sort_bits == (uint32_t)o.parts[0].bit_count &&
                        ((dq.sort_flags & mrk::SORT_FLOAT) != 0) == (o.parts[0].kind == MRK_SORTKEY_FLOAT) && ((dq.sort_flags & mrk::SORT_DESC) != 0) == (o.parts[0].desc != 0),
                    "first locator");
            if (o.n_parts == 2)
              CHECK(dq.ord_item == (uint32_t)o.parts[1].bit_offset / 32 && dq.ord_shift == (uint32_t)o.parts[1].bit_offset % 32 && dq.ord_bits == (uint32_t)o.parts[1].bit_count &&
                        ((dq.ord_flags & mrk::SORT_FLOAT) != 0) == (o.parts[1].kind == MRK_SORTKEY_FLOAT) && ((dq.ord_flags & mrk::SORT_DESC) != 0) == (o.parts[1].desc != 0),
                    "second locator");
            else
              CHECK(dq.ord_bits == 0 && dq.ord_item == 0 && dq.ord_flags == 0, "a second part that is not there");
          }
          // the bins are the relevance bins of the weight (bins_by_weight): those of the same query without an order
          if (rk != MRK_RANK_NONE) { // (relevance under NONE bins by rowid; weight-first keeps the weight's bins: every match in one of them)
            const int rr = mrk::plan_query(seg, qr.q, 128 << 10, true, dr, 1, 0, plan_r);
            CHECK(rr == MRK_OK && dr.bin_mode == mrk::BIN_WEIGHT && dq.bin_mode == mrk::BIN_WEIGHT && dq.bin_lo == dr.bin_lo && dq.bin_shift == dr.bin_shift, "the relevance bins: %d/%u against %d/%u",
                  dq.bin_lo, dq.bin_shift, dr.bin_lo, dr.bin_shift);
          } else
            CHECK(dq.bin_mode == mrk::BIN_WEIGHT, "NONE: the weight's bins");
        }
  const size_t want_acc = 5 * 4 * (orders.size() + 1);
  CHECK((size_t)n_acc == want_acc, "accepted %d of %zu", n_acc, want_acc);

  auto plan_one = [&](const mrk_order& o, bool packed, int cutoff, const mrk_segment* seg, DevQuery* out = nullptr) {
    Q q;
    make_query(q, t2, 2, MRK_OP_AND, MRK_RANK_BM25);
    q.q.order = &o;
    q.q.cutoff = cutoff;
    mrk::BatchPlan plan;
    DevQuery dq;
    g_err[0] = 0;
    const int rc = mrk::plan_query(seg, q.q, 128 << 10, packed, dq, 1, 0, plan, cutoff ? 5000u : 0xFFFFFFFFu);
    if (out) *out = dq;
    return rc;
  };
  // ---- MRK_E_INVAL, before anything is read (the sanitizers watch the rows' vector)
  std::vector<mrk_order> bad;
  bad.push_back(order_of(3, 1, TS));
  bad.push_back(order_of(-1, 1, TS));
  bad.push_back(order_of(INT32_MAX, 2, TS, F5));
  bad.push_back(order_of(INT32_MIN, 0));
  bad.push_back(order_of(4, 1, TS));                      // 0x104, and the flag without a direction
  bad.push_back(order_of(0, 1, TS, mrk_order_part{}, MRK_ORDER_WEIGHT_FIRST));
  bad.push_back(order_of(0, 0, mrk_order_part{}, mrk_order_part{}, MRK_ORDER_WEIGHT_FIRST));
  bad.push_back(order_of(1, 0));                          // relevance: the caller leaves order NULL
  bad.push_back(order_of(0, 0));                          // no parts and no weight
  bad.push_back(order_of(2, -1));
  bad.push_back(order_of(1, 3, TS, F5));
  bad.push_back(order_of(2, 3, TS, F5));
  bad.push_back(order_of(1, 2, I64D, TS));                // INT64 as one of two parts
  bad.push_back(order_of(1, 1, mrk_order_part{MRK_SORTKEY_INT, 30, 5, 1}));        // straddles two dwords
  bad.push_back(order_of(2, 1, mrk_order_part{MRK_SORTKEY_INT, 7 * 32, 32, 1}));    // past the row
  bad.push_back(order_of(1, 1, mrk_order_part{MRK_SORTKEY_FLOAT, 32, 5, 1}));
  bad.push_back(order_of(1, 1, mrk_order_part{MRK_SORTKEY_INT64, 4 * 32 + 16, 64, 1}));
  bad.push_back(order_of(1, 1, mrk_order_part{7, 0, 32, 1}));
  for (const mrk_order& b : bad) {
    const int rc = plan_one(b, true, 0, &S);
    CHECK(rc == MRK_E_INVAL && g_err[0], "hostile order parts %d then_weight %d: rc %d", b.n_parts, b.then_weight, rc);
  }
  // ---- MRK_E_UNSUPPORTED: what mrk_order declines per query, with the weight in front too
  const mrk_order_part BLOB{MRK_SORTKEY_INT, -1, 0, 1}, NANCOL{MRK_SORTKEY_FLOAT, 96, 32, 1};
  struct Dec { mrk_order o; bool packed; int cutoff; const mrk_segment* seg; const char* what; };
  const Dec decs[] = {{order_of(1, 1, BLOB), true, 0, &S, "blob-stored single part"},
                      {order_of(2, 2, TS, BLOB), true, 0, &S, "blob-stored second part"},
                      {order_of(1, 1, mrk_order_part{MRK_SORTKEY_INT64, -1, 64, 1}), true, 0, &S, "blob-stored 64-bit part"},
                      {order_of(1, 1, NANCOL), true, 0, &S, "NaN column"},
                      {order_of(2, 2, TS, NANCOL), true, 0, &S, "NaN column second"},
                      {order_of(1, 1, TS), true, 10, &S, "cutoff"},
                      {order_of(2, 0), true, 10, &S, "cutoff without parts"},
                      {order_of(1, 1, TS), false, 0, &S, "VLB path"},
                      {order_of(2, 0), false, 0, &S, "VLB path without parts"},
                      {order_of(1, 1, TS), true, 0, &bare, "no attribute rows"},
                      {order_of(1, 1, I64D), true, 0, &bare, "no attribute rows (64-bit)"}};
  for (const Dec& d : decs) {
    const int rc = plan_one(d.o, d.packed, d.cutoff, d.seg);
    CHECK(rc == MRK_E_UNSUPPORTED && g_err[0], "%s: rc %d '%s'", d.what, rc, g_err);
  }
  // ---- the weight behind the parts plans what it planned before: one part is mrk_query.sort's plan word for word (the new
  // words zero), a 64-bit key keeps its layout
  const mrk_sort locs[] = {{MRK_SORTKEY_INT, 0, 32, 1, 1}, {MRK_SORTKEY_INT, 32 + 3, 5, 0, 0}, {MRK_SORTKEY_FLOAT, 64, 32, 0, 2}};
  for (const Shape& sh : shapes)
    for (const mrk_sort& so : locs) {
      Q qa, qb;
      make_query(qa, sh.t, sh.n, sh.op, MRK_RANK_PROXIMITY_BM25);
      make_query(qb, sh.t, sh.n, sh.op, MRK_RANK_PROXIMITY_BM25);
      const mrk_order o = order_of(0, 1, mrk_order_part{so.kind, so.bit_offset, so.bit_count, so.desc}, mrk_order_part{}, so.then_weight);
      qa.q.sort = &so, qb.q.order = &o;
      mrk::BatchPlan pa, pb;
      DevQuery da, db;
      const int ra = mrk::plan_query(&S, qa.q, 128 << 10, true, da, 1, 0, pa), rb = mrk::plan_query(&S, qb.q, 128 << 10, true, db, 1, 0, pb);
      CHECK(ra == MRK_OK && rb == MRK_OK, "one part: rc %d / %d", ra, rb);
      CHECK(!memcmp(&da, &db, sizeof da) && db.wf_parts == 0 && db.wf_pad == 0, "one part through order: another head pass than through sort");
      CHECK(pa.extra.size() == pb.extra.size() && (pa.extra.empty() || !memcmp(pa.extra.data(), pb.extra.data(), pa.extra.size() * sizeof(DevQuery))), "passes differ");
      CHECK(pa.sort_total == pb.sort_total && pa.cand_total == pb.cand_total, "arenas differ");
    }
  for (const mrk_order& o : {order_of(0, 1, I64D, mrk_order_part{}, 1), order_of(0, 2, TS, F5, 2)}) {
    DevQuery dq;
    CHECK(plan_one(o, true, 0, &S, &dq) == MRK_OK, "64-bit key: %s", g_err);
    CHECK(dq.sort_on == mrk::SORT_ON_ORDER && (dq.sort_flags & mrk::SORT_WIDE) && !(dq.sort_flags & mrk::SORT_WFIRST) && dq.wf_parts == 0 && dq.wf_pad == 0 && dq.sort_tie == (uint32_t)o.then_weight, "a 64-bit key with the weight behind it");
  }
  if (g_bad) return printf("%d checks failed\n", g_bad), 1;
  printf("ok accepted %d declined %zu hostile %zu\n", n_acc, sizeof decs / sizeof decs[0], bad.size());
  return 0;
}
