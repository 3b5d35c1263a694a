// sortsel_geom.cpp -- the bin geometry the sorted selection's edge cases rest on (tests/sortsel_edges_common.py), on the host under
// AddressSanitizer + UBSan: the planner (csrc/mrk_plan.cpp) plans each named query over a stand-in segment that holds the test's own
// attribute rows, and the program prints what it set -- bin_lo, bin_shift, ord_geom -- and the bins of the named probe keys through
// cand_bin (csrc/mrk_sortkey.h: sort_bin / order_bin / wfirst_bin), with the candidate's high word built as the scan kernels build it.
// Built and run by tests/test_sortsel_edges_cpu.py, which asserts the premises on the output; no GPU, no libmrk.so.
//
//   sortsel_geom ROWS QUERY...
// ROWS: u32 n_rows, u32 stride, then the rows.  QUERY, fields separated by ':':
//   name : s|o : n_parts : kind0 : off0 : cnt0 : desc0 : kind1 : off1 : cnt1 : desc1 : then_weight : fw0 : fw1 : probe,probe,...
// s = through mrk_query.sort (part 0, then_weight 0..2), o = through mrk_query.order (then_weight as mrk_order takes it, 0x101 / 0x102
// included); fw0 / fw1 the two field weights (0 0 = none given).  A probe is a hex u64: the raw value of a sort, raw0 << 32 | raw1 of
// an order (an INT64: the value itself), the weight (int32, low dword) of a weight-first order.  Answer, one line per query:
//   q name sort_on S tie T bin_lo L bin_shift H geom A B N G bins b,b,...
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
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

static std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out(1);
  for (char c : s)
    if (c == sep)
      out.emplace_back();
    else
      out.back() += c;
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) return printf("usage: sortsel_geom ROWS QUERY...\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  uint32_t head[2] = {0, 0};
  if (!f || fread(head, 4, 2, f) != 2 || !head[0] || !head[1] || head[1] > 64u) return printf("FAIL %s: no rows header\n", argv[1]), 1;
  const uint32_t n_rows = head[0], stride = head[1];
  mrk_ctx ctx;
  mrk_segment S;
  static uint32_t dummy[16];
  S.ctx = &ctx;
  S.total_docs = n_rows;
  S.n_fields = 2;
  S.has_packed = true;
  uint32_t blk = 0;
  for (int t = 0; t < 2; ++t) { // the two keywords of corpus S: a quarter of the rowids each
    HostTerm h;
    h.docs = n_rows / 4;
    h.hits = h.docs * 2, h.nblocks = (h.docs + 127) / 128, h.blk_first = blk, blk += h.nblocks;
    h.doclist_off = 1 + (uint64_t)t * 1000000, h.doclist_len = h.docs * 3ull, h.packed_bytes = h.docs * 2ull;
    h.last_rowid = n_rows - 4;
    h.bm_off = (uint64_t)t * 4096, h.dir_off = (uint64_t)t * 64;
    S.terms.push_back(h);
  }
  S.dev.n_windows = (n_rows + 2047) / 2048;
  S.dev.pk_attr = dummy, S.dev.pk_hit = dummy, S.dev.bm = dummy, S.dev.attrs = dummy;
  S.dev.attr_stride = stride;
  S.attr_rows = n_rows;
  S.h_attrs.resize((size_t)n_rows * stride);
  if (fread(S.h_attrs.data(), 4, S.h_attrs.size(), f) != S.h_attrs.size() || fgetc(f) != EOF) return printf("FAIL %s: %u rows of %u dwords expected\n", argv[1], n_rows, stride), 1;
  fclose(f);

  for (int a = 2; a < argc; ++a) {
    const std::vector<std::string> w = split(argv[a], ':');
    if (w.size() != 15 || (w[1] != "s" && w[1] != "o")) return printf("FAIL query '%s': 15 fields expected\n", argv[a]), 1;
    auto num = [&](size_t i) { return (int32_t)strtol(w[i].c_str(), nullptr, 0); };
    mrk_order o;
    memset(&o, 0, sizeof o);
    o.n_parts = num(2), o.then_weight = num(11);
    for (int p = 0; p < 2; ++p) o.parts[p] = mrk_order_part{num(3 + 4 * (size_t)p), num(4 + 4 * (size_t)p), num(5 + 4 * (size_t)p), num(6 + 4 * (size_t)p)};
    const mrk_sort so{o.parts[0].kind, o.parts[0].bit_offset, o.parts[0].bit_count, o.parts[0].desc, o.then_weight};
    const int32_t fw[2] = {num(12), num(13)};
    mrk_node nodes[3];
    memset(nodes, 0, sizeof nodes);
    const int32_t children[2] = {0, 1};
    for (int i = 0; i < 2; ++i) nodes[i].op = MRK_OP_TERM, nodes[i].term_id = i, nodes[i].atom_pos = i + 1, nodes[i].field_mask = 0xFFFFFFFFu, nodes[i].boost = 1.0f;
    nodes[2].op = MRK_OP_AND, nodes[2].n_children = 2, nodes[2].first_child = 0, nodes[2].field_mask = 0xFFFFFFFFu, nodes[2].boost = 1.0f;
    mrk_query q;
    memset(&q, 0, sizeof q);
    q.nodes = nodes, q.n_nodes = 3, q.children = children, q.root = 2;
    q.ranker = MRK_RANK_BM25, q.max_matches = 1000, q.normalized_tfidf = 1;
    if (fw[0] || fw[1]) q.field_weights = fw, q.n_weights = 2;
    if (w[1] == "s")
      q.sort = &so;
    else
      q.order = &o;
    mrk::BatchPlan plan;
    DevQuery dq;
    g_err[0] = 0;
    const int rc = mrk::plan_query(&S, q, 128 << 10, true, dq, 1, 0, plan);
    if (rc != MRK_OK) return printf("FAIL query '%s': rc %d: %s\n", argv[a], rc, g_err), 1;
    printf("q %s sort_on %u tie %u bin_lo %d bin_shift %u geom %u %u %u %u bins ", w[0].c_str(), dq.sort_on, dq.sort_tie, dq.bin_lo, dq.bin_shift, dq.ord_geom.a_lo, dq.ord_geom.b_lo,
           dq.ord_geom.nb, dq.ord_geom.shift);
    bool first = true;
    for (const std::string& ps : split(w[14], ',')) {
      if (ps.empty()) continue;
      const uint64_t p = strtoull(ps.c_str(), nullptr, 16);
      uint64_t hi; // the candidate's high word: mrk_sortkey.h's three layouts
      if (dq.sort_on == mrk::SORT_ON_WEIGHT)
        hi = mrk::wfirst_hi(dq.sort_tie, (int32_t)(uint32_t)p, 0ull);
      else if (dq.sort_on == mrk::SORT_ON_ORDER)
        hi = mrk::order_key(mrk::order_map_part((uint32_t)(p >> 32), dq.sort_flags), mrk::order_map_part((uint32_t)p, dq.ord_flags));
      else if (dq.sort_on == mrk::SORT_ON_ATTR)
        hi = ((uint64_t)mrk::sort_map_key((uint32_t)p, dq.sort_flags) << 32) | mrk::sort_weight_part(dq.sort_tie, 1500);
      else
        return printf("\nFAIL query '%s': planned as a relevance query\n", argv[a]), 1;
      const uint32_t b = mrk::cand_bin(dq.sort_on, dq.sort_tie, dq.bin_lo, dq.bin_shift, dq.ord_geom, hi);
      if (b >= 1024u) return printf("\nFAIL query '%s': probe %s in bin %u\n", argv[a], ps.c_str(), b), 1;
      printf(first ? "%u" : ",%u", b);
      first = false;
    }
    printf("\n");
  }
  printf("ok %d queries\n", argc - 2);
  return 0;
}
