// fuzz_plan.cpp -- the query planner (csrc/mrk_plan.cpp, host code only) under AddressSanitizer + UBSan on the CPU.
// A caller hands mrk_batch_submit a flattened tree it built itself; whatever it holds -- child indices out of range, cycles, shared
// subtrees, unknown operators, keywords outside the dictionary, absurd operator arguments, filters with impossible locators -- the
// planner must answer MRK_OK, MRK_E_UNSUPPORTED or MRK_E_INVAL and touch nothing it does not own.  The segment is a host-side
// stand-in (term table + flags; its device pointers are never followed by the planner).  Built and run by
// tests/test_plan_fuzz.py; no GPU, no libmrk.so: the three library symbols the planner calls are stubbed here.
#include <math.h>
#include <stdarg.h>
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
extern "C" float mrk_idf(int64_t docs, int64_t total, int plain, int normalized, int n_qwords, float boost) { // (values do not matter here)
  if (docs <= 0 || total <= 0) return 0.0f;
  float v = plain ? logf((float)total / (float)docs) : logf((float)(total - docs + 1) / (float)docs);
  v /= 2.0f * logf((float)(1 + total));
  if (normalized && n_qwords > 0) v /= (float)n_qwords;
  return v * boost;
}

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_s += 0x9E3779B97F4A7C15ull;
  uint64_t z = g_s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return n ? (uint32_t)(rnd() % n) : 0u; }
static bool chance(uint32_t pct) { return below(100) < pct; }
static int32_t wild_int() {
  switch (below(8)) {
    case 0: return 0;
    case 1: return -1;
    case 2: return INT32_MAX;
    case 3: return INT32_MIN;
    case 4: return (int32_t)rnd();
    default: return (int32_t)below(70);
  }
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  if (argc > 2) g_s = strtoull(argv[2], nullptr, 0);
  mrk_ctx ctx;
  // three stand-in segments: packed + bitmaps + attributes, packed without hit references, VLB only
  mrk_segment segs[3];
  static uint32_t dummy[16];
  for (int s = 0; s < 3; ++s) {
    mrk_segment& S = segs[s];
    S.ctx = &ctx;
    S.total_docs = s == 2 ? 5000 : 1000000;
    S.n_fields = s == 1 ? 12 : 3;
    S.has_packed = s != 2;
    uint32_t blk = 0;
    for (int t = 0; t < 40; ++t) {
      HostTerm h;
      h.docs = t == 7 ? 0 : (uint32_t)(S.total_docs / (uint64_t)(t + 2));
      h.hits = h.docs * 2;
      h.nblocks = (h.docs + 127) / 128;
      h.blk_first = blk;
      blk += h.nblocks;
      h.doclist_off = 1 + (uint64_t)t * 100000;
      h.doclist_len = h.docs * 3ull;
      h.packed_bytes = h.docs * 2ull;
      h.last_rowid = h.docs ? (uint32_t)S.total_docs - 1 - (uint32_t)t : 0;
      if (s == 0 && t < 12) h.bm_off = (uint64_t)t * 4096, h.dir_off = (uint64_t)t * 64;
      S.terms.push_back(h);
    }
    S.dev.n_windows = (uint32_t)((S.total_docs + 2047) / 2048);
    if (s != 2) S.dev.pk_attr = dummy;
    if (s == 0) {
      S.dev.pk_hit = dummy;
      S.dev.bm = dummy;
      S.dev.attrs = dummy;
      S.dev.attr_stride = 7;
      S.dev.blobs = (const uint8_t*)dummy;
      S.n_blob_attrs = 2;
      S.attr_rows = S.total_docs;
    }
  }
  int n_ok = 0, n_uns = 0, n_inval = 0;
  for (int it = 0; it < iters; ++it) {
    const bool hostile = chance(50); // the other half: well-formed trees of every operator, so that the deep paths run too
    const int n_nodes = 1 + (int)below(hostile ? 40 : 14);
    std::vector<mrk_node> nodes((size_t)n_nodes);
    std::vector<int32_t> children;
    std::vector<int64_t> local_docs;
    int pos = 1;
    for (int i = 0; i < n_nodes; ++i) {
      mrk_node& N = nodes[(size_t)i];
      memset(&N, 0, sizeof N);
      N.field_mask = chance(80) ? 0xFFFFFFFFu : (uint32_t)rnd();
      N.boost = chance(90) ? 1.0f : (float)wild_int();
      const bool leaf = hostile ? chance(50) : i < (n_nodes + 1) / 2;
      if (leaf) {
        N.op = MRK_OP_TERM;
        N.term_id = hostile && chance(15) ? wild_int() : (int32_t)below(40);
        N.atom_pos = hostile && chance(4) ? wild_int() : pos++;
        N.term_pos = hostile && chance(10) ? wild_int() : (chance(85) ? 0 : (int32_t)below(5));
        N.field_max_pos = chance(50) ? (int32_t)below(30) : wild_int();
        N.not_weighted = (int32_t)below(2);
      } else {
        N.op = hostile && chance(10) ? wild_int() : (int32_t)below(13);
        N.opt = hostile && chance(30) ? wild_int() : (int32_t)(1 + below(8));
        N.term_id = chance(70) ? (int32_t)below(40) : wild_int(); // (SENTENCE / PARAGRAPH: the boundary keyword)
        N.first_child = (int32_t)children.size();
        const int nk = hostile ? (int)below(12) : 2 + (int)below(N.op == MRK_OP_ANDNOT || N.op == MRK_OP_MAYBE || N.op == MRK_OP_NOTNEAR ? 1 : 4);
        N.n_children = nk;
        for (int k = 0; k < nk; ++k) {
          int32_t c;
          if (hostile)
            c = chance(10) ? wild_int() : (int32_t)below((uint32_t)n_nodes); // any node: cycles, self, shared
          else
            c = (int32_t)below((uint32_t)i ? (uint32_t)i : 1u); // an earlier node (post-order-like; may be shared between parents)
          children.push_back(c);
        }
        if (hostile && chance(5)) N.n_children = wild_int(); // (kept inside children[] below)
        if (hostile && chance(5)) N.first_child = wild_int();
      }
    }
    // the one contract the planner cannot check: [first_child, first_child + n_children) lies inside children[]
    children.resize(children.size() + 16, 0);
    for (mrk_node& N : nodes) {
      if (N.op == MRK_OP_TERM) continue;
      const int64_t room = (int64_t)children.size();
      if (N.first_child < 0 || N.first_child > room) N.first_child = 0;
      if (N.n_children < 0 && chance(50)) N.n_children = 0;
      if ((int64_t)N.first_child + (int64_t)(N.n_children > 0 ? N.n_children : 0) > room) N.n_children = (int32_t)(room - N.first_child);
    }
    mrk_query q;
    memset(&q, 0, sizeof q);
    q.nodes = nodes.data();
    q.n_nodes = hostile && chance(3) ? wild_int() % (n_nodes + 1) : n_nodes;
    if (q.n_nodes > n_nodes) q.n_nodes = n_nodes;
    q.children = children.data();
    q.root = hostile && chance(10) ? wild_int() : n_nodes - 1;
    q.ranker = hostile && chance(10) ? wild_int() : (int32_t)below(9);
    q.max_matches = hostile && chance(10) ? wild_int() : (chance(50) ? 1000 : 1 + (int32_t)below(1024));
    int32_t fw[40];
    for (int i = 0; i < 40; ++i) fw[i] = chance(80) ? 1 + (int32_t)below(5) : wild_int();
    if (chance(50)) q.field_weights = fw, q.n_weights = hostile && chance(20) ? wild_int() % 41 : (int32_t)below(9);
    if (q.n_weights < 0 && chance(50)) q.n_weights = 0;
    q.index_weight = chance(80) ? 0 : wild_int();
    q.plain_idf = (int32_t)below(2), q.normalized_tfidf = (int32_t)below(2);
    q.total_docs_override = chance(80) ? 0 : (int64_t)wild_int() * (chance(50) ? 1 : 1000003);
    if (chance(20)) {
      local_docs.resize((size_t)n_nodes);
      for (int64_t& v : local_docs) v = chance(50) ? -1 : (int64_t)wild_int();
      q.local_docs = local_docs.data();
    }
    q.cutoff = chance(85) ? 0 : wild_int();
    mrk_filter fl[4];
    int64_t vals[12];
    for (int i = 0; i < 12; ++i) vals[i] = (int64_t)i * 3 + (hostile ? wild_int() : 0);
    for (int i = 0; i < 4; ++i) {
      mrk_filter& F = fl[i];
      memset(&F, 0, sizeof F);
      F.kind = hostile && chance(10) ? wild_int() : (int32_t)below(3);
      F.bit_offset = hostile && chance(30) ? wild_int() : (int32_t)(32 * below(7));
      F.bit_count = hostile && chance(30) ? wild_int() : (chance(70) ? 32 : 64);
      F.exclude = (int32_t)below(2), F.has_equal_min = (int32_t)below(2), F.has_equal_max = (int32_t)below(2);
      F.open_left = chance(10), F.open_right = chance(10);
      F.min_value = wild_int(), F.max_value = wild_int();
      F.values = chance(90) ? vals : nullptr;
      F.n_values = hostile && chance(20) ? wild_int() : (int32_t)below(10);
      if (F.n_values > 12) F.n_values = 12; // (values[] is the caller's array: its length is the caller's word)
      F.fmin = (float)wild_int(), F.fmax = (float)wild_int();
      if (chance(15)) F.mva_bits = chance(80) ? (chance(50) ? 32 : 64) : wild_int(), F.mva_all = (int32_t)below(2), F.blob_attr_id = hostile ? wild_int() : (int32_t)below(2), F.n_blob_attrs = hostile ? wild_int() : 2;
    }
    if (chance(30)) q.filters = fl, q.n_filters = hostile && chance(20) ? wild_int() % 5 : (int32_t)below(3);
    if (chance(15)) q.weight_filters = fl + 1, q.n_weight_filters = hostile && chance(20) ? wild_int() % 4 : (int32_t)below(3);

    const mrk_segment* seg = &segs[below(3)];
    DevQuery dq;
    mrk::BatchPlan plan;
    const std::vector<DevQuery>& extra = plan.extra;
    const std::vector<DevItem>&items = plan.items, &items_bm = plan.items_bm;
    const std::vector<mrk::GenProg>& progs = plan.gen_progs;
    const uint32_t n_queries = 1 + below(4), qi = below(n_queries);
    const int rc = mrk::plan_query(seg, q, 128 << 10, seg->has_packed && chance(90), dq, n_queries, qi, plan, chance(90) ? 0xFFFFFFFFu : below(1000000));
    if (rc == MRK_OK) {
      ++n_ok;
      // what the launch code relies on
      auto check_pass = [&](const DevQuery& P) {
        if (P.n_terms > MRK_MAX_AND_TERMS || P.n_nodes > 16 || P.out_q != qi || P.n_filters > MRK_MAX_FILTERS || P.n_wfilters > MRK_MAX_FILTERS || P.k > MRK_MAX_K) {
          fprintf(stderr, "iteration %d: pass out of bounds (terms %u nodes %u out_q %u)\n", it, P.n_terms, P.n_nodes, P.out_q);
          exit(3);
        }
        for (uint32_t t = 0; t < P.n_terms; ++t)
          if ((uint64_t)P.t[t].blk_first + P.t[t].nblocks > (1ull << 32)) exit(4);
        if ((P.tree_flags & mrk::TF_GEN) && P.gen_prog >= progs.size()) {
          fprintf(stderr, "iteration %d: program index %u of %zu\n", it, P.gen_prog, progs.size());
          exit(5);
        }
      };
      check_pass(dq);
      for (const DevQuery& P : extra) check_pass(P);
      for (const DevItem& I : items)
        if (I.query != qi && (I.query < n_queries || I.query >= n_queries + extra.size())) exit(6);
      for (const DevItem& I : items_bm)
        if (I.query != qi && (I.query < n_queries || I.query >= n_queries + extra.size())) exit(7);
      for (const mrk::GenProg& G : progs)
        if (G.n_nodes > (uint32_t)mrk::GEN_MAX_NODES) exit(8);
    } else if (rc == MRK_E_UNSUPPORTED)
      ++n_uns;
    else if (rc == MRK_E_INVAL)
      ++n_inval;
    else {
      fprintf(stderr, "iteration %d: plan_query returned %d\n", it, rc);
      return 2;
    }
  }
  printf("ok %d unsupported %d invalid %d\n", n_ok, n_uns, n_inval);
  return 0;
}
