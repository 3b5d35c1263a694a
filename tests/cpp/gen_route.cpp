// gen_route.cpp -- which rank pass the planner (csrc/mrk_plan.cpp, host code only) gives a query: the witness behind
// tests/gen_edges_common.py's route().  Reads a text file, one record per line:
//   T <n> <docs of term 0> ... <docs of term n-1>          the dictionary of the queries that follow
//   Q <n_fields> <ranker> <n_nodes> { <op> <term_id> <atom_pos> <field_mask> <opt> <term_pos> <field_max_pos> <n_children> <first_child> } <n> { <child> }
// (the root is node 0, as api.py's _CQueries flattens a tree) and prints one line per query: "G" = tree_flags & TF_GEN, "GN" = ... with
// TF_GEN_NEARN, "S" = a specialised pass, "D <message>" = declined.  The segment is a host-side stand-in as in order_plan.cpp (packed
// arrays and hit references at hand, no bitmaps); no GPU, no libmrk.so.  Built and run by tests/test_gen_edges_cpu.py.
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
extern "C" float mrk_idf(int64_t docs, int64_t total, int, int normalized, int n_qwords, float boost) { // (a stand-in: no plan's shape depends on it)
  if (docs <= 0 || total <= 0) return 0.0f;
  float v = (float)(total - docs + 1) / (float)(total + docs);
  if (normalized && n_qwords > 0) v /= (float)n_qwords;
  return v * boost;
}

int main(int argc, char** argv) {
  if (argc < 2) return fprintf(stderr, "usage: gen_route FILE\n"), 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  static uint32_t dummy[16];
  mrk_ctx ctx;
  std::vector<long long> docs;
  char tag[8];
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "T")) {
      int n = 0;
      if (fscanf(f, "%d", &n) != 1 || n < 0 || n > 4096) return fprintf(stderr, "bad T record\n"), 2;
      docs.assign((size_t)n, 0);
      for (long long& d : docs)
        if (fscanf(f, "%lld", &d) != 1) return fprintf(stderr, "bad T record\n"), 2;
      continue;
    }
    if (strcmp(tag, "Q")) return fprintf(stderr, "unknown record %s\n", tag), 2;
    int n_fields = 0, ranker = 0, n_nodes = 0;
    if (fscanf(f, "%d %d %d", &n_fields, &ranker, &n_nodes) != 3 || n_nodes < 1 || n_nodes > 64) return fprintf(stderr, "bad Q record\n"), 2;
    std::vector<mrk_node> nodes((size_t)n_nodes);
    for (mrk_node& N : nodes) {
      memset(&N, 0, sizeof N);
      long long mask = 0;
      if (fscanf(f, "%d %d %d %lld %d %d %d %d %d", &N.op, &N.term_id, &N.atom_pos, &mask, &N.opt, &N.term_pos, &N.field_max_pos, &N.n_children, &N.first_child) != 9)
        return fprintf(stderr, "bad node\n"), 2;
      N.field_mask = (uint32_t)mask, N.boost = 1.0f;
    }
    int n_ch = 0;
    if (fscanf(f, "%d", &n_ch) != 1 || n_ch < 0 || n_ch > 1024) return fprintf(stderr, "bad child list\n"), 2;
    std::vector<int32_t> children((size_t)n_ch + 1, 0);
    for (int i = 0; i < n_ch; ++i)
      if (fscanf(f, "%d", &children[(size_t)i]) != 1) return fprintf(stderr, "bad child list\n"), 2;
    for (const mrk_node& N : nodes)
      if (N.n_children < 0 || N.first_child < 0 || N.first_child + N.n_children > n_ch) return fprintf(stderr, "children out of range\n"), 2;

    mrk_segment S;
    S.ctx = &ctx;
    S.total_docs = 4096;
    S.n_fields = (uint32_t)n_fields;
    S.has_packed = true;
    S.wide = n_fields > 8;
    uint32_t blk = 0;
    for (size_t t = 0; t < docs.size(); ++t) {
      HostTerm h;
      h.docs = (uint32_t)docs[t];
      h.hits = h.docs * 2, h.nblocks = (h.docs + 127) / 128, h.blk_first = blk, blk += h.nblocks;
      h.doclist_off = 1 + (uint64_t)t * 100000, h.doclist_len = h.docs * 3ull, h.packed_bytes = h.docs * 2ull;
      h.last_rowid = h.docs ? (uint32_t)S.total_docs - 1 - (uint32_t)t : 0;
      S.terms.push_back(h);
    }
    S.dev.n_windows = (uint32_t)((S.total_docs + 2047) / 2048);
    S.dev.pk_attr = dummy, S.dev.pk_hit = dummy;

    mrk_query q;
    memset(&q, 0, sizeof q);
    q.nodes = nodes.data(), q.n_nodes = n_nodes, q.children = children.data(), q.root = 0;
    q.ranker = ranker, q.max_matches = 1000, q.normalized_tfidf = 1;
    mrk::BatchPlan plan;
    DevQuery dq;
    g_err[0] = 0;
    const int rc = mrk::plan_query(&S, q, 128 << 10, true, dq, 1, 0, plan);
    if (rc != MRK_OK)
      printf("D %s\n", g_err);
    else
      printf("%s\n", (dq.tree_flags & mrk::TF_GEN_NEARN) ? "GN" : (dq.tree_flags & mrk::TF_GEN) ? "G" : "S");
  }
  fclose(f);
  return 0;
}
