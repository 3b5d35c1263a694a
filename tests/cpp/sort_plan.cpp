// sort_plan.cpp -- sorted queries (mrk_query.sort) on the host, under AddressSanitizer + UBSan: the order-preserving key map
// (csrc/mrk_sortkey.h) over edge values, and the planner's answers (csrc/mrk_plan.cpp) -- every covered shape accepted and kept
// off the bitmap-driven kernels, every declined shape declined with a message, hostile sort specs refused before a row is read.
// Built and run by tests/test_sort_cpu.py; no GPU, no libmrk.so (the segment is a host-side stand-in as in fuzz_plan.cpp).
#include <math.h>
#include <stdarg.h>
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
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);            \
      printf("\n");                   \
      ++g_bad;                        \
    }                                 \
  } while (0)

static uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

static void test_map() {
  using namespace mrk;
  // integers: unsigned order, both directions
  const uint32_t iv[] = {0u, 1u, 2u, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  const int ni = sizeof iv / sizeof iv[0];
  for (int i = 0; i < ni; ++i)
    for (int j = 0; j < ni; ++j) {
      CHECK((iv[i] < iv[j]) == (sort_map_key(iv[i], SORT_DESC) < sort_map_key(iv[j], SORT_DESC)), "int desc %u %u", iv[i], iv[j]);
      CHECK((iv[i] < iv[j]) == (sort_map_key(iv[i], 0) > sort_map_key(iv[j], 0)), "int asc %u %u", iv[i], iv[j]);
    }
  // floats, ascending by value: -inf, -max, -1, -min normal, -denormals, zeros, +denormals ... +inf
  const float fv[] = {-INFINITY, -3.4028234664e38f, -1.0f, -1.17549435e-38f, -1.0e-40f, -1.4e-45f, 0.0f, 1.4e-45f, 1.0e-40f, 1.17549435e-38f, 1.0f, 3.4028234664e38f, INFINITY};
  const int nf = sizeof fv / sizeof fv[0];
  for (int i = 0; i < nf; ++i)
    for (int j = 0; j < nf; ++j) {
      const uint32_t a = sort_map_key(fbits(fv[i]), SORT_FLOAT | SORT_DESC), b = sort_map_key(fbits(fv[j]), SORT_FLOAT | SORT_DESC);
      CHECK((fv[i] < fv[j]) == (a < b) && (fv[i] == fv[j]) == (a == b), "float desc %g %g", fv[i], fv[j]);
      const uint32_t c = sort_map_key(fbits(fv[i]), SORT_FLOAT), d = sort_map_key(fbits(fv[j]), SORT_FLOAT);
      CHECK((fv[i] < fv[j]) == (c > d), "float asc %g %g", fv[i], fv[j]);
    }
  CHECK(sort_map_key(0x80000000u, SORT_FLOAT | SORT_DESC) == sort_map_key(0u, SORT_FLOAT | SORT_DESC), "-0.0 must fold onto +0.0");
  CHECK(sort_map_key(0x80000000u, SORT_FLOAT) == sort_map_key(0u, SORT_FLOAT), "-0.0 must fold onto +0.0 (asc)");
  CHECK(sort_is_nan(0x7FC00000u) && sort_is_nan(0xFFC00001u) && sort_is_nan(0x7F800001u) && !sort_is_nan(0x7F800000u) && !sort_is_nan(0xFF800000u), "NaN test");
  CHECK(sort_extract(0xABCD1234u, 4, 5) == ((0xABCD1234u >> 4) & 31u) && sort_extract(0xABCD1234u, 0, 32) == 0xABCD1234u && sort_extract(0x80000000u, 31, 1) == 1u, "extract");
  // bins are monotone in the mapped key and stay inside the histogram
  uint32_t prev = 0;
  for (uint64_t m = 0; m <= 0xFFFFFFFFull; m += 0x00FFFFFFull) {
    const uint32_t b = sort_bin(0x10000000u, 22, (uint32_t)m);
    CHECK(b >= prev && b < 1024u, "bin of %llx", (unsigned long long)m);
    prev = b;
  }
  CHECK(sort_weight_part(1, 5) > sort_weight_part(1, -5) && sort_weight_part(2, 5) < sort_weight_part(2, -5) && sort_weight_part(0, 5) == sort_weight_part(0, 9), "tie rules");
}

struct Q {
  std::vector<mrk_node> nodes;
  std::vector<int32_t> children;
  mrk_query q;
};
// AND (or `op`) of keywords terms[0..n)
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

int main() {
  test_map();
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
    h.bm_off = (uint64_t)t * 4096, h.dir_off = (uint64_t)t * 64; // every keyword is dense: unsorted ANDs go to the bitmap kernels
    S.terms.push_back(h);
  }
  S.dev.n_windows = (uint32_t)((S.total_docs + 2047) / 2048);
  S.dev.pk_attr = dummy, S.dev.pk_hit = dummy, S.dev.bm = dummy, S.dev.attrs = dummy;
  // rows: [0] timestamps in a narrow band, [1] bit-fields, [2] floats, [3] floats with one NaN, [4..5] a 64-bit attribute
  const uint32_t stride = 6;
  S.dev.attr_stride = stride;
  S.attr_rows = S.total_docs;
  S.h_attrs.resize((size_t)S.total_docs * stride);
  for (uint64_t r = 0; r < S.total_docs; ++r) {
    uint32_t* row = &S.h_attrs[r * stride];
    row[0] = 1700000000u + (uint32_t)((r * 2654435761ull) % 5000000ull);
    row[1] = (uint32_t)(r * 40503ull);
    row[2] = fbits((float)((int64_t)(r % 2001) - 1000) * 0.25f);
    row[3] = r == 777 ? 0x7FC00000u : row[2];
    row[4] = (uint32_t)r, row[5] = 1;
  }
  const int t1[] = {3}, t2[] = {0, 1}, t8[] = {0, 1, 2, 3, 4, 5, 6, 7}, tor[] = {2, 5};
  const int rankers[] = {MRK_RANK_NONE, MRK_RANK_BM25, MRK_RANK_PROXIMITY_BM25, MRK_RANK_SPH04};
  struct Shape { const int* t; int n, op; };
  const Shape shapes[] = {{t1, 1, MRK_OP_AND}, {t2, 2, MRK_OP_AND}, {t8, 8, MRK_OP_AND}, {tor, 2, MRK_OP_OR}, {t2, 2, MRK_OP_PHRASE}};
  const mrk_sort locs[] = {{MRK_SORTKEY_INT, 0, 32, 1, 1}, {MRK_SORTKEY_INT, 32 + 3, 5, 0, 0}, {MRK_SORTKEY_INT, 32 + 31, 1, 1, 2}, {MRK_SORTKEY_FLOAT, 64, 32, 0, 1}};
  int n_acc = 0;
  for (const Shape& sh : shapes)
    for (int rk : rankers)
      for (const mrk_sort& so : locs) {
        Q q;
        make_query(q, sh.t, sh.n, sh.op, rk);
        // the same query by relevance first: the dense AND goes to a bitmap kernel (so the check below means something)
        mrk::BatchPlan p0;
        DevQuery d0;
        int rc = mrk::plan_query(&S, q.q, 128 << 10, true, d0, 1, 0, p0);
        CHECK(rc == MRK_OK && !d0.sort_on && d0.cand_cap > 0 && p0.sort_total == 0, "relevance plan rc %d", rc);
        q.q.sort = &so;
        mrk::BatchPlan plan;
        DevQuery dq;
        rc = mrk::plan_query(&S, q.q, 128 << 10, true, dq, 1, 0, plan);
        CHECK(rc == MRK_OK, "covered shape declined: n %d op %d ranker %d loc %d/%d: %s", sh.n, sh.op, rk, so.bit_offset, so.bit_count, g_err);
        if (rc != MRK_OK) continue;
        ++n_acc;
        CHECK(dq.sort_on == 1 && dq.cand_cap == 0 && dq.sort_cap > 0 && plan.sort_total == dq.sort_cap && plan.cand_total == 0, "sort arena");
        CHECK(dq.sort_item == (uint32_t)so.bit_offset / 32 && dq.sort_shift == (uint32_t)so.bit_offset % 32 && dq.sort_bits == (uint32_t)so.bit_count && dq.sort_tie == (uint32_t)so.then_weight, "locator");
        CHECK(!(dq.tree_flags & (mrk::TF_BITMAP | mrk::TF_BTREE)), "a sorted query on a bitmap kernel");
        for (const DevQuery& P : plan.extra) CHECK(P.sort_on == 1 && !(P.tree_flags & (mrk::TF_BITMAP | mrk::TF_BTREE)), "pass without the sort");
        for (const DevItem& it : plan.items_bm) CHECK(it.kind == 2, "a sorted query laid out as a scan_bm / scan_bt item");
        // the bins cover the column: every row's mapped key lands inside [0, NBINS), the extremes in different bins for the wide columns
        uint32_t bmin = 0xFFFFFFFFu, bmax = 0;
        for (uint64_t r = 0; r < S.total_docs; r += 97) {
          const uint32_t m = mrk::sort_map_key(mrk::sort_extract(S.h_attrs[r * stride + dq.sort_item], dq.sort_shift, dq.sort_bits), dq.sort_flags);
          const uint32_t b = mrk::sort_bin((uint32_t)dq.bin_lo, dq.bin_shift, m);
          bmin = b < bmin ? b : bmin, bmax = b > bmax ? b : bmax;
        }
        CHECK(bmax < 1024u, "bin out of range");
        if (so.bit_count == 32) CHECK(bmax - bmin >= 256u, "column range not used: bins %u..%u", bmin, bmax);
      }
  CHECK(n_acc == 5 * 4 * 4, "accepted %d", n_acc);
  CHECK(S.sort_ranges.size() == 4, "column ranges cached per locator: %zu", S.sort_ranges.size());

  auto plan_one = [&](const mrk_sort& so, bool packed, int cutoff, const mrk_segment* seg) {
    Q q;
    make_query(q, t2, 2, MRK_OP_AND, MRK_RANK_BM25);
    q.q.sort = &so;
    q.q.cutoff = cutoff;
    mrk::BatchPlan plan;
    DevQuery dq;
    g_err[0] = 0;
    return mrk::plan_query(seg, q.q, 128 << 10, packed, dq, 1, 0, plan, cutoff ? 5000u : 0xFFFFFFFFu);
  };
  const mrk_sort ok{MRK_SORTKEY_INT, 0, 32, 1, 1};
  // declined, each with a message
  mrk_segment bare = S;
  bare.dev.attrs = nullptr, bare.h_attrs.clear(), bare.sort_ranges.clear();
  struct Dec { mrk_sort so; bool packed; int cutoff; const mrk_segment* seg; const char* what; };
  const Dec decs[] = {{{MRK_SORTKEY_INT, 128, 64, 1, 1}, true, 0, &S, "64-bit attribute"},
                      {{MRK_SORTKEY_INT, -1, 0, 1, 1}, true, 0, &S, "blob-stored attribute"},
                      {{MRK_SORTKEY_FLOAT, 96, 32, 1, 1}, true, 0, &S, "NaN column"},
                      {ok, true, 10, &S, "cutoff"},
                      {ok, false, 0, &S, "VLB path"},
                      {ok, true, 0, &bare, "no attribute rows"}};
  for (const Dec& d : decs) {
    const int rc = plan_one(d.so, d.packed, d.cutoff, d.seg);
    CHECK(rc == MRK_E_UNSUPPORTED && g_err[0], "%s: rc %d '%s'", d.what, rc, g_err);
  }
  {
    Q q;
    make_query(q, t2, 2, MRK_OP_AND, MRK_RANK_BM25);
    q.q.sort = &ok, q.q.max_matches = MRK_MAX_K + 1;
    mrk::BatchPlan plan;
    DevQuery dq;
    CHECK(mrk::plan_query(&S, q.q, 128 << 10, true, dq, 1, 0, plan) == MRK_E_UNSUPPORTED, "K > MRK_MAX_K");
  }
  // hostile: refused before a row is read (the sanitizers watch the rows' vector)
  const mrk_sort bad[] = {{MRK_SORTKEY_INT, 0, 0, 1, 1},    {MRK_SORTKEY_INT, 0, 33, 1, 1},  {MRK_SORTKEY_INT, 0, 63, 1, 1},   {MRK_SORTKEY_INT, 160, 64, 1, 1} /* runs off the row */,
                          {MRK_SORTKEY_INT, 16, 64, 1, 1},  {MRK_SORTKEY_INT, 0, 65, 1, 1},  {MRK_SORTKEY_INT, 0, -5, 1, 1},   {MRK_SORTKEY_INT, 6 * 32, 32, 1, 1},
                          {MRK_SORTKEY_INT, INT32_MAX - 7, 8, 1, 1}, {MRK_SORTKEY_INT, 30, 5, 1, 1} /* straddles two dwords */, {2, 0, 32, 1, 1}, {-1, 0, 32, 1, 1},
                          {MRK_SORTKEY_INT, 0, 32, 1, 3},   {MRK_SORTKEY_INT, 0, 32, 1, -1}, {MRK_SORTKEY_FLOAT, 32, 5, 1, 1}, {MRK_SORTKEY_INT, INT32_MAX, INT32_MAX, 1, 1}};
  for (const mrk_sort& b : bad) {
    const int rc = plan_one(b, true, 0, &S);
    CHECK(rc == MRK_E_INVAL && g_err[0], "hostile spec kind %d loc %d/%d tie %d: rc %d", b.kind, b.bit_offset, b.bit_count, b.then_weight, rc);
  }
  if (g_bad) return 1;
  printf("ok accepted %d declined %zu hostile %zu\n", n_acc, sizeof decs / sizeof decs[0] + 1, sizeof bad / sizeof bad[0]);
  return 0;
}
