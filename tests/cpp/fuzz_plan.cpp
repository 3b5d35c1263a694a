// fuzz_plan.cpp -- the query planner (csrc/mrk_plan.cpp, host code only) under AddressSanitizer + UBSan on the CPU.
// A caller hands mrk_batch_submit a flattened tree it built itself; whatever it holds -- child indices out of range, cycles, shared
// subtrees, unknown operators, keywords outside the dictionary, absurd operator arguments, filters with impossible locators -- the
// planner must answer MRK_OK, MRK_E_UNSUPPORTED or MRK_E_INVAL and touch nothing it does not own.  The segment is a host-side
// stand-in (term table + flags; its device pointers are never followed by the planner).  Built and run by
// tests/test_plan_fuzz.py; no GPU, no libmrk.so: the three library symbols the planner calls are stubbed here.
//
// Three kinds of iterations: hostile trees, well-formed trees of every operator, and "typical" queries (1-4 keyword AND / OR /
// PHRASE / PROXIMITY / QUORUM / NEAR trees over the dense keywords with the common rankers -- the shapes that reach the bitmap-driven
// kernels, which the uniform generator almost never draws).  Every kind also draws mrk_query.sort / mrk_query.order (well-formed and
// hostile), filters, weight filters and a cutoff bound.
//
// `fuzz_plan ITERS SEED digest` also prints one FNV-1a digest per 1000 iterations over everything plan_query answered: the return
// code and message, and for an accepted query the head pass, every further pass, both item vectors, every GenProg and the BatchPlan's
// scalars -- hashed field by field (DevQuery and SortRange have padding).  Then the count of accepted plans per class and the digest of
// the segments' sort_ranges caches.  tests/golden/plan_digests.json holds these lines as recorded from plan_query while it was one
// 770-line function (before it was split into stages); the mrk_idf stub below is IEEE + - * / only, so that no digest depends on a libm.
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
extern "C" float mrk_idf(int64_t docs, int64_t total, int plain, int normalized, int n_qwords, float boost) { // (a stand-in: + - * / only)
  if (docs <= 0 || total <= 0) return 0.0f;
  const float r = plain ? (float)total / (float)docs : (float)(total - docs + 1) / (float)docs;
  float v = (r - 1.0f) / (r + 1.0f) * 0.5f;
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


struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void add(const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  }
  template <typename T>
  void val(const T& x) { add(&x, sizeof x); }
};
static_assert(sizeof(DevTerm) == 6 * 4 + 8 + 2 * 4 + 2 * 8 + 2 * 4, "DevTerm has no padding: hashed whole");
static_assert(sizeof(mrk::DevFilter) == 6 * 4 + 2 * 8 + 8 * MRK_MAX_FILTER_VALUES, "DevFilter has no padding: hashed whole");
static_assert(sizeof(mrk::GenNode) == 32 && sizeof(mrk::GenProg) == 32 + 32 * mrk::GEN_MAX_NODES, "GenProg has no padding: hashed whole");
static_assert(sizeof(DevItem) == 16 && sizeof(mrk::OrderGeom) == 16, "hashed whole");
static void hash_pass(Fnv& H, const DevQuery& P) { // member by member: the struct has padding (behind cand_cap, n_filters ...)
#define F(x) H.val(P.x)
  F(n_terms), F(ranker), F(k), F(n_weights), F(index_weight), F(item_first), F(n_items), F(bin_mode), F(bin_lo), F(bin_shift), F(cand_cap), F(cand_off);
  F(out_q), F(n_nodes), F(req_mask), F(excl_mask), F(tree_flags), F(prog), F(ph_atoms), F(n_filters), F(filters), F(ph_mask);
  F(qr_mask), F(qr_thr), F(qr_n), F(qr_row), F(qr_ord), F(px_dist), F(nn_a), F(nn_b), F(nn_dist), F(max_qpos), F(n_qwords), F(gen_prog), F(rowid_max);
  F(n_wfilters), F(wfilters), F(weights), F(t), F(sort_on), F(sort_item), F(sort_shift), F(sort_bits), F(sort_flags), F(sort_tie), F(sort_cap), F(sort_pad), F(sort_off);
  F(ord_item), F(ord_shift), F(ord_bits), F(ord_flags), F(ord_geom);
#undef F
}

enum { C_BLOCK1, C_BLOCKN, C_BM_PAIR, C_BT_TREE, C_BT_PHRASE, C_GEN, C_GEN_NEARN, C_QUORUM, C_FILTERED, C_WFILTERED, C_CUTOFF, C_SORT, C_ORDER_AS_SORT, C_ORDER_I64,
       C_ORDER_TWO, C_WIDE, C_VLB, C_EMPTY, N_CLASSES };
static const char* const CLASS_NAMES[N_CLASSES] = {"block_scan_1_pass", "block_scan_2plus_passes", "scan_bm_pair", "tree_on_bitmap_words", "phrase_on_bitmap_words", "generic",
                                                   "generic_near_3plus", "quorum", "filtered", "weight_filtered", "cutoff", "sort", "order_as_sort", "order_int64",
                                                   "order_two_parts", "wide_segment", "vlb_path", "empty_query"};

// a row-attribute column of segment 0's stand-in rows (7 dwords): what a well-formed sort / order / filter names
struct Column { int32_t kind, bit_offset, bit_count; };
static const Column COLUMNS[] = {{MRK_SORTKEY_INT, 0, 32},     {MRK_SORTKEY_FLOAT, 32, 32}, /* no NaN */ {MRK_SORTKEY_FLOAT, 64, 32}, /* holds a NaN */
                                 {MRK_SORTKEY_INT, 96, 32} /* constant */, {MRK_SORTKEY_INT64, 128, 64}, {MRK_SORTKEY_INT, 196, 8}, {MRK_SORTKEY_INT, 192, 4}};
static Column draw_column(bool narrow) {
  for (;;) {
    const Column c = COLUMNS[below(7)];
    if (!(narrow && c.kind == MRK_SORTKEY_INT64) && !(c.bit_offset == 64 && chance(70))) return c;
  }
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  if (argc > 2) g_s = strtoull(argv[2], nullptr, 0);
  const bool digest_mode = argc > 3 && !strcmp(argv[3], "digest");
  mrk_ctx ctx;
  // four stand-in segments: packed + bitmaps + attributes, packed without hit references, VLB only, packed in the wide (9-32 field) layout
  constexpr int N_SEGS = 4;
  mrk_segment segs[N_SEGS];
  static uint32_t dummy[16];
  for (int s = 0; s < N_SEGS; ++s) {
    mrk_segment& S = segs[s];
    S.ctx = &ctx;
    S.total_docs = s == 2 ? 5000 : 1000000;
    S.n_fields = s == 1 || s == 3 ? 12 : 3;
    S.has_packed = s != 2;
    S.wide = s == 3;
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
    if (s == 3) S.dev.pk_hit = dummy;
    if (s == 0) {
      S.dev.pk_hit = dummy;
      S.dev.bm = dummy;
      S.dev.attrs = dummy;
      S.dev.attr_stride = 7;
      S.dev.blobs = (const uint8_t*)dummy;
      S.n_blob_attrs = 2;
      S.attr_rows = S.total_docs;
      // real rows on the host (the planner takes a sort column's range from them; see COLUMNS): an integer, a float, a float with one
      // NaN, a constant, a signed 64-bit pair, bit fields
      const uint32_t rows = 3000;
      S.h_attrs.resize((size_t)rows * 7);
      uint64_t x = 0x1234567ull;
      auto lcg = [&]() { return x = x * 6364136223846793005ull + 1442695040888963407ull, (uint32_t)(x >> 32); };
      for (uint32_t r = 0; r < rows; ++r) {
        uint32_t* row = &S.h_attrs[(size_t)r * 7];
        row[0] = lcg() % 100000u + 17u;
        const float f1 = (float)((int32_t)(lcg() % 20001u) - 10000) * 0.25f, f2 = (float)(lcg() % 1000u);
        memcpy(&row[1], &f1, 4), memcpy(&row[2], &f2, 4);
        if (r == 1234) row[2] = 0x7FC00000u;
        row[3] = 42;
        const int64_t v = (int64_t)(((uint64_t)lcg() << 32) | lcg()) >> 20;
        row[4] = (uint32_t)(uint64_t)v, row[5] = (uint32_t)((uint64_t)v >> 32);
        row[6] = lcg();
      }
    }
  }
  int n_ok = 0, n_uns = 0, n_inval = 0;
  uint64_t n_class[N_CLASSES] = {};
  Fnv H;
  for (int it = 0; it < iters; ++it) {
    // a third typical queries; of the rest half hostile, half well-formed trees of every operator, so that the deep paths run too
    const bool typical = chance(34), hostile = !typical && chance(50);
    const int n_nodes = typical ? 8 : 1 + (int)below(hostile ? 40 : 14);
    std::vector<mrk_node> nodes((size_t)n_nodes);
    std::vector<int32_t> children;
    std::vector<int64_t> local_docs;
    int pos = 1;
    int root = n_nodes - 1;
    if (typical) {
      for (mrk_node& N : nodes) {
        memset(&N, 0, sizeof N);
        N.field_mask = 0xFFFFFFFFu, N.boost = 1.0f;
      }
      int used = 0;
      auto term = [&]() {
        mrk_node& N = nodes[(size_t)used];
        N.op = MRK_OP_TERM, N.term_id = chance(85) ? (int32_t)below(12) : (int32_t)below(40), N.atom_pos = pos++;
        return used++;
      };
      auto group = [&](int32_t op, int opt, std::initializer_list<int> kids) {
        mrk_node& N = nodes[(size_t)used];
        N.op = op, N.opt = opt, N.first_child = (int32_t)children.size(), N.n_children = (int32_t)kids.size();
        for (int k : kids) children.push_back(k);
        return used++;
      };
      auto flat = [&](int32_t op, int k) { // op over k keywords
        int kid[4];
        for (int i = 0; i < k; ++i) kid[i] = term();
        const int opt = op == MRK_OP_QUORUM ? 1 + (int)below((uint32_t)k) : 1 + (int)below(6);
        return k == 2 ? group(op, opt, {kid[0], kid[1]}) : k == 3 ? group(op, opt, {kid[0], kid[1], kid[2]}) : group(op, opt, {kid[0], kid[1], kid[2], kid[3]});
      };
      static const int32_t FLAT_OPS[] = {MRK_OP_AND, MRK_OP_AND, MRK_OP_OR, MRK_OP_PHRASE, MRK_OP_PROXIMITY, MRK_OP_QUORUM, MRK_OP_NEAR};
      static const int32_t JOIN_OPS[] = {MRK_OP_AND, MRK_OP_OR, MRK_OP_ANDNOT, MRK_OP_MAYBE};
      switch (below(10)) {
        case 0: root = term(); break;
        case 1: case 2: case 3: case 4: case 5: root = flat(FLAT_OPS[below(7)], chance(40) ? 2 : 2 + (int)below(3)); break;
        case 6: case 7: { // one group next to a keyword
          const int g = flat(FLAT_OPS[below(6)], 2 + (int)below(2)), t = term();
          root = group(JOIN_OPS[below(4)], 0, {g, t});
          break;
        }
        case 8: { // two phrases: a case for the generic evaluator
          const int a = flat(chance(50) ? MRK_OP_PHRASE : MRK_OP_PROXIMITY, 2), b = flat(MRK_OP_PHRASE, 2);
          root = group(chance(70) ? MRK_OP_AND : MRK_OP_OR, 0, {a, b});
          break;
        }
        default: root = flat(MRK_OP_NEAR, 3 + (int)below(2)); break;
      }
    } else
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
    q.root = hostile && chance(10) ? wild_int() : root;
    static const int32_t COMMON_RANKERS[] = {MRK_RANK_PROXIMITY_BM25, MRK_RANK_PROXIMITY_BM25, MRK_RANK_BM25, MRK_RANK_BM25, MRK_RANK_NONE, MRK_RANK_SPH04, MRK_RANK_PROXIMITY, MRK_RANK_MATCHANY, MRK_RANK_WORDCOUNT, MRK_RANK_FIELDMASK};
    q.ranker = hostile && chance(10) ? wild_int() : typical ? COMMON_RANKERS[below(10)] : (int32_t)below(9);
    q.max_matches = hostile && chance(10) ? wild_int() : (chance(50) ? 1000 : 1 + (int32_t)below(1024));
    int32_t fw[40];
    for (int i = 0; i < 40; ++i) fw[i] = chance(80) ? 1 + (int32_t)below(5) : wild_int();
    if (chance(50)) q.field_weights = fw, q.n_weights = hostile && chance(20) ? wild_int() % 41 : (int32_t)below(typical ? 14 : 9);
    if (q.n_weights < 0 && chance(50)) q.n_weights = 0;
    q.index_weight = chance(80) ? 0 : wild_int();
    q.plain_idf = (int32_t)below(2), q.normalized_tfidf = (int32_t)below(2);
    q.total_docs_override = chance(80) ? 0 : (int64_t)wild_int() * (chance(50) ? 1 : 1000003);
    if (chance(typical ? 5 : 20)) {
      local_docs.resize((size_t)n_nodes);
      for (int64_t& v : local_docs) v = chance(50) ? -1 : (int64_t)wild_int();
      q.local_docs = local_docs.data();
    }
    q.cutoff = chance(85) ? 0 : typical ? 1 + (int32_t)below(1024) : wild_int();
    mrk_filter fl[4];
    int64_t vals[12];
    for (int i = 0; i < 12; ++i) vals[i] = (int64_t)i * 3 + (hostile ? wild_int() : 0);
    for (int i = 0; i < 4; ++i) {
      mrk_filter& F = fl[i];
      memset(&F, 0, sizeof F);
      F.kind = hostile && chance(10) ? wild_int() : (int32_t)below(3);
      F.bit_offset = hostile && chance(30) ? wild_int() : (int32_t)(32 * below(7));
      F.bit_count = hostile && chance(30) ? wild_int() : (chance(70) ? 32 : 64);
      if (typical && (F.kind == MRK_FILTER_FLOATRANGE || F.bit_offset > 160)) F.bit_count = 32;
      F.exclude = (int32_t)below(2), F.has_equal_min = (int32_t)below(2), F.has_equal_max = (int32_t)below(2);
      F.open_left = chance(10), F.open_right = chance(10);
      F.min_value = wild_int(), F.max_value = wild_int();
      F.values = chance(typical ? 100 : 90) ? vals : nullptr;
      F.n_values = hostile && chance(20) ? wild_int() : typical ? 1 + (int32_t)below(8) : (int32_t)below(10);
      if (F.n_values > 12) F.n_values = 12; // (values[] is the caller's array: its length is the caller's word)
      F.fmin = (float)wild_int(), F.fmax = (float)wild_int();
      if (chance(15)) F.mva_bits = chance(80) ? (chance(50) ? 32 : 64) : wild_int(), F.mva_all = (int32_t)below(2), F.blob_attr_id = hostile ? wild_int() : (int32_t)below(2), F.n_blob_attrs = hostile ? wild_int() : 2;
      if (typical && F.mva_bits && F.kind == MRK_FILTER_FLOATRANGE) F.kind = MRK_FILTER_RANGE;
    }
    if (chance(typical ? 20 : 30)) q.filters = fl, q.n_filters = hostile && chance(20) ? wild_int() % 5 : typical ? 1 + (int32_t)below(2) : (int32_t)below(3);
    if (chance(15)) q.weight_filters = fl + 1, q.n_weight_filters = hostile && chance(20) ? wild_int() % 4 : typical ? 1 + (int32_t)below(2) : (int32_t)below(3);
    if (typical) // (a weight filter knows VALUES and RANGE)
      for (int i = 0; i < q.n_weight_filters; ++i)
        if (q.weight_filters[i].kind == MRK_FILTER_FLOATRANGE) fl[1 + i].kind = MRK_FILTER_RANGE;

    // the sorter's order: mrk_query.sort, mrk_query.order, now and then both
    mrk_sort srt;
    mrk_order ordr;
    memset(&srt, 0, sizeof srt), memset(&ordr, 0, sizeof ordr);
    const bool bad_order = hostile || chance(5); // (hostile specs reach the typical and the well-formed trees too)
    const uint32_t which = below(100);
    if (which < 12 || which == 99) {
      const Column c = draw_column(!chance(5));
      srt = mrk_sort{c.kind, c.bit_offset, c.bit_count, (int32_t)below(2), (int32_t)below(3)};
      if (bad_order) switch (below(8)) {
          case 0: srt.kind = wild_int(); break;
          case 1: srt.bit_offset = chance(50) ? -1 : wild_int(); break; // (-1: a blob-stored attribute)
          case 2: srt.bit_count = wild_int(); break;
          case 3: srt.then_weight = wild_int(); break;
          case 4: srt.bit_offset += 1 + (int32_t)below(31); break; // misaligned: may straddle a dword
          case 5: srt.kind = MRK_SORTKEY_FLOAT, srt.bit_count = 1 + (int32_t)below(31); break;
          case 6: srt.bit_offset = 32 * (int32_t)(7 + below(3)); break; // past the row
          default: break;
        }
      q.sort = &srt;
    }
    if ((which >= 12 && which < 32) || which >= 98) {
      ordr.n_parts = chance(45) ? 1 : 2;
      ordr.then_weight = (int32_t)below(3);
      for (int p = 0; p < 2; ++p) {
        const Column c = draw_column(ordr.n_parts == 2 || chance(30));
        ordr.parts[p] = mrk_order_part{c.kind, c.bit_offset, c.bit_count, (int32_t)below(2)};
      }
      if (bad_order) switch (below(10)) {
          case 0: ordr.n_parts = chance(50) ? 0 : 3; break;
          case 1: ordr.n_parts = wild_int(); break;
          case 2: ordr.n_parts = 2, ordr.parts[below(2)] = mrk_order_part{MRK_SORTKEY_INT64, 128, 64, 1}; break; // INT64 next to a second part
          case 3: ordr.parts[below(2)].bit_offset = chance(50) ? -1 : wild_int(); break;                                // a blob locator
          case 4: ordr.parts[below(2)].bit_offset += 1 + (int32_t)below(31); break;                                    // misaligned
          case 5: { mrk_order_part& P = ordr.parts[below(2)]; P.kind = MRK_SORTKEY_FLOAT, P.bit_count = 1 + (int32_t)below(31); break; }
          case 6: ordr.then_weight = chance(50) ? 3 : wild_int(); break;
          case 7: ordr.parts[below(2)].kind = wild_int(); break;
          case 8: ordr.parts[below(2)].bit_count = wild_int(); break;
          default: ordr.parts[below(2)].bit_offset = 32 * (int32_t)(6 + below(3)); break; // the last dword / past the row
        }
      q.order = &ordr;
    }

    // typical queries go to the segment with bitmaps and attribute rows most of the time
    const uint32_t seg_draw = below(100);
    const int seg_i = typical ? (seg_draw < 60 ? 0 : seg_draw < 75 ? 3 : seg_draw < 87 ? 1 : 2) : (int)below(N_SEGS);
    const mrk_segment* seg = &segs[seg_i];
    const bool use_packed = seg->has_packed && chance(typical ? 97 : 90);
    const uint32_t rowid_max = chance(typical ? 92 : 90) ? 0xFFFFFFFFu : below(1000000);
    DevQuery dq;
    mrk::BatchPlan plan;
    const uint32_t n_queries = 1 + below(4), qi = below(n_queries);
    // (a batch in progress: earlier queries' items and arena slots are there already)
    plan.cand_total = below(5000), plan.sort_total = chance(50) ? below(5000) : 0;
    plan.items.resize(below(3), DevItem{0, 0, 1, 0}), plan.items_bm.resize(below(3), DevItem{0, 0, 1, 0});
    const size_t items0 = plan.items.size(), items_bm0 = plan.items_bm.size();
    const std::vector<DevQuery>& extra = plan.extra;
    const std::vector<DevItem>&items = plan.items, &items_bm = plan.items_bm;
    const std::vector<mrk::GenProg>& progs = plan.gen_progs;
    g_err[0] = 0;
    const int rc = mrk::plan_query(seg, q, 128 << 10, use_packed, dq, n_queries, qi, plan, rowid_max);
    H.val(rc);
    if (rc != MRK_OK) H.add(g_err, strlen(g_err) + 1);
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
      for (size_t i = items0; i < items.size(); ++i)
        if (items[i].query != qi && (items[i].query < n_queries || items[i].query >= n_queries + extra.size())) exit(6);
      for (size_t i = items_bm0; i < items_bm.size(); ++i)
        if (items_bm[i].query != qi && (items_bm[i].query < n_queries || items_bm[i].query >= n_queries + extra.size())) exit(7);
      for (const mrk::GenProg& G : progs)
        if (G.n_nodes > (uint32_t)mrk::GEN_MAX_NODES) exit(8);

      hash_pass(H, dq);
      H.val(extra.size()), H.val(items.size()), H.val(items_bm.size()), H.val(progs.size());
      for (const DevQuery& P : extra) hash_pass(H, P);
      H.add(items.data(), items.size() * sizeof(DevItem)), H.add(items_bm.data(), items_bm.size() * sizeof(DevItem));
      H.add(progs.data(), progs.size() * sizeof(mrk::GenProg));
      H.val(plan.algo_bytes), H.val(plan.dev_bytes), H.val(plan.cand_total), H.val(plan.sort_total), H.val(plan.any_prox), H.val(plan.any_tree);

      const uint32_t tf = dq.tree_flags;
      const bool nothing = extra.empty() && items.size() == items0 && items_bm.size() == items_bm0 && dq.n_items == 0; // a required keyword without postings
      bool cls[N_CLASSES] = {};
      cls[C_EMPTY] = nothing;
      cls[C_BLOCK1] = !nothing && extra.empty() && !(tf & (mrk::TF_BITMAP | mrk::TF_BTREE | mrk::TF_GEN));
      cls[C_BLOCKN] = !extra.empty() && !(tf & mrk::TF_GEN);
      cls[C_BM_PAIR] = (tf & mrk::TF_BITMAP) != 0;
      cls[C_BT_TREE] = (tf & mrk::TF_BTREE) && !(tf & mrk::TF_PHRASE);
      cls[C_BT_PHRASE] = (tf & mrk::TF_BTREE) && (tf & mrk::TF_PHRASE);
      cls[C_GEN] = !nothing && (tf & mrk::TF_GEN);
      cls[C_GEN_NEARN] = !nothing && (tf & mrk::TF_GEN_NEARN);
      cls[C_QUORUM] = !nothing && dq.qr_thr > 0;
      cls[C_FILTERED] = dq.n_filters > 0;
      cls[C_WFILTERED] = dq.n_wfilters > 0;
      cls[C_CUTOFF] = dq.rowid_max != 0xFFFFFFFFu;
      cls[C_SORT] = q.sort != nullptr;
      cls[C_ORDER_AS_SORT] = q.order && dq.sort_on == 1;
      cls[C_ORDER_I64] = q.order && dq.sort_on == mrk::SORT_ON_ORDER && ordr.parts[0].kind == MRK_SORTKEY_INT64;
      cls[C_ORDER_TWO] = q.order && dq.sort_on == mrk::SORT_ON_ORDER && ordr.n_parts == 2;
      cls[C_WIDE] = seg->wide;
      cls[C_VLB] = !use_packed;
      for (int c = 0; c < N_CLASSES; ++c) n_class[c] += cls[c];
    } else if (rc == MRK_E_UNSUPPORTED)
      ++n_uns;
    else if (rc == MRK_E_INVAL)
      ++n_inval;
    else {
      fprintf(stderr, "iteration %d: plan_query returned %d\n", it, rc);
      return 2;
    }
    if (digest_mode && (it + 1) % 1000 == 0) {
      printf("chunk %d %016llx\n", it / 1000, (unsigned long long)H.h);
      H = Fnv();
    }
  }
  if (digest_mode) {
    printf("classes");
    for (int c = 0; c < N_CLASSES; ++c) printf(" %s %llu", CLASS_NAMES[c], (unsigned long long)n_class[c]);
    printf("\n");
    Fnv R; // the per-segment caches of column ranges: entries in the order the queries asked for them
    for (const mrk_segment& S : segs) {
      R.val(S.sort_ranges.size());
      for (const mrk_segment::SortRange& r : S.sort_ranges)
        R.val(r.bit_offset), R.val(r.bit_count), R.val(r.is_float), R.val(r.lo), R.val(r.hi), R.val(r.has_nan), R.val(r.lo64), R.val(r.hi64);
    }
    printf("sort_ranges %016llx\n", (unsigned long long)R.h);
  }
  printf("ok %d unsupported %d invalid %d\n", n_ok, n_uns, n_inval);
  return 0;
}
