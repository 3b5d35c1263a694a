// select_subkey.cpp -- the arithmetic of the relevance top-K selection (csrc/mrk_select.hip) that a CPU can call, held against the
// DEFINITION of the sorter's order (weight descending, then global rowid ascending; make_key's order) on the host, under
// AddressSanitizer + UBSan:
//   * weight_bin and rowid_bin (csrc/mrk_sortkey.h; bin_of of mrk_kprune.h is these two) are monotone non-decreasing in that order;
//   * wherever sub_guard accepts a (geometry, threshold bin), SubKey::sub is monotone non-decreasing in it over the keys of that bin
//     and stays below 2048 -- and the geometries it must decline are declined;
//   * the planner (csrc/mrk_plan.cpp) gives the bin geometry each case of tests/test_gpu_select_edges.py relies on.
// Built and run by tests/test_select_edges_cpu.py; no GPU, no libmrk.so (the segment is a host-side stand-in as in
// weight_first_plan.cpp).  Arguments, any number of them: DOCS:DF0[:DF1]:W[,W...] -- on a segment of DOCS rowids the BM25 query over
// one keyword of DF0 docs (or the AND of two, of DF0 and DF1) must put each weight W into an interior bin.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <random>
#include <set>
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
  if (total < docs) total = docs;
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

using mrk::BIN_ROWID;
using mrk::BIN_WEIGHT;
using mrk::SubKey;

static const int32_t LOS[] = {INT32_MIN, -5000, 0, 1, 123457};
static const uint32_t SHIFTS[] = {0, 1, 5, 10, 11, 12, 15, 22, 31};
static const uint32_t RBITS[] = {1, 11, 12, 16, 20, 25, 32};
static const uint32_t EDGE_BINS[] = {0, 1, 2, 511, 1022, 1023, 1024};

static uint32_t bin_of_key(uint32_t mode, int32_t lo, uint32_t shift, uint64_t key) {
  return mode == BIN_WEIGHT ? mrk::weight_bin(lo, shift, mrk::key_weight(key)) : mrk::rowid_bin(shift, mrk::key_rowid(key));
}

// ---- the bins along the order: keys sorted best-first must walk the bins downwards
static uint64_t g_bin_keys = 0;
static void bin_monotone() {
  const uint32_t few_rows[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  for (int32_t lo : LOS)
    for (uint32_t sh : SHIFTS) {
      std::set<int32_t> ws = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX};
      for (uint32_t b : EDGE_BINS)
        for (int d = -1; d <= 1; ++d) {
          const int64_t w = (int64_t)lo + ((int64_t)b << sh) + d;
          if (w >= INT32_MIN && w <= INT32_MAX) ws.insert((int32_t)w);
        }
      std::vector<uint64_t> keys;
      for (int32_t w : ws)
        for (uint32_t r : few_rows) {
          keys.push_back(mrk::make_key(w, r));
          CHECK(mrk::key_weight(keys.back()) == w && mrk::key_rowid(keys.back()) == r, "key round trip %d %u", w, r);
        }
      std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
      uint32_t prev = 1023;
      for (size_t i = 0; i < keys.size(); ++i) {
        const uint32_t b = bin_of_key(BIN_WEIGHT, lo, sh, keys[i]);
        CHECK(b < 1024u && b <= prev, "weight_bin lo %d shift %u: bin %u behind bin %u at weight %d", lo, sh, b, prev, mrk::key_weight(keys[i]));
        if (i && mrk::key_weight(keys[i]) == mrk::key_weight(keys[i - 1])) CHECK(b == prev, "weight_bin depends on the rowid");
        prev = b;
      }
      g_bin_keys += keys.size();
    }
  for (uint32_t sh : SHIFTS) {
    std::set<uint32_t> rs = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t b : EDGE_BINS)
      for (int d = -1; d <= 1; ++d) {
        const int64_t r = ((int64_t)b << sh) + d;
        if (r >= 0 && r <= 0xFFFFFFFFll) rs.insert((uint32_t)r);
      }
    std::vector<uint64_t> keys;
    for (uint32_t r : rs) keys.push_back(mrk::make_key(1, r)); // (the planner bins by rowid only where every weight is the same)
    std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
    uint32_t prev = 1023;
    for (uint64_t k : keys) {
      const uint32_t b = bin_of_key(BIN_ROWID, 0, sh, k);
      CHECK(b < 1024u && b <= prev, "rowid_bin shift %u: bin %u behind bin %u at rowid %u", sh, b, prev, mrk::key_rowid(k));
      prev = b;
    }
    CHECK(mrk::rowid_bin(sh, 0u) == 1023u, "rowid 0 is in the best bin");
    g_bin_keys += keys.size();
  }
}

// ---- the sub-bins of one (geometry, bin): the keys of weights [w0, w1] x global rowids [r0, r1], every one of them in `bin`
static uint64_t g_sub_keys = 0, g_exhaustive = 0, g_sampled = 0;
static std::mt19937_64 g_rng(0x5EED5E1Eull);
static void sub_monotone(const SubKey& sk, uint32_t bin, int64_t w0, int64_t w1, uint64_t r0, uint64_t r1) {
  const uint64_t nw = (uint64_t)(w1 - w0) + 1, nr = r1 - r0 + 1;
  std::vector<uint64_t> keys;
  if (nw <= 4096 && nr <= 4096 && nw * nr <= 4096) {
    for (int64_t w = w0; w <= w1; ++w)
      for (uint64_t r = r0; r <= r1; ++r) keys.push_back(mrk::make_key((int32_t)w, (uint32_t)r));
    ++g_exhaustive;
  } else {
    for (int64_t w : {w0, w1})
      for (uint64_t r : {r0, r1}) keys.push_back(mrk::make_key((int32_t)w, (uint32_t)r));
    for (int i = 0; i < 10000; ++i) keys.push_back(mrk::make_key((int32_t)(w0 + (int64_t)(g_rng() % nw)), (uint32_t)(r0 + g_rng() % nr)));
    ++g_sampled;
  }
  std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
  uint32_t prev = 0xFFFFFFFFu;
  for (uint64_t k : keys) {
    CHECK(bin_of_key(sk.mode, sk.lo, sk.shift, k) == bin, "mode %u lo %d shift %u: weight %d rowid %u is not in bin %u", sk.mode, sk.lo, sk.shift, mrk::key_weight(k), mrk::key_rowid(k), bin);
    const uint32_t s = sk.sub(k);
    CHECK(s < 2048u, "mode %u lo %d shift %u rbits %u rhi %u: sub %u", sk.mode, sk.lo, sk.shift, sk.rbits, sk.rhi, s);
    CHECK(s <= prev, "mode %u lo %d shift %u rbits %u rhi %u bin %u: sub %u behind sub %u at weight %d rowid %u", sk.mode, sk.lo, sk.shift, sk.rbits, sk.rhi, bin, s, prev,
          mrk::key_weight(k), mrk::key_rowid(k));
    prev = s;
  }
  g_sub_keys += keys.size();
}

static int g_geoms = 0, g_accepted = 0, g_dec_bin0 = 0, g_dec_top = 0, g_dec_nobits = 0, g_dec_wide = 0, g_empty = 0;
static bool g_tot_le11 = false, g_tot_gt11 = false, g_tot_56 = false;
static void sub_bins() {
  for (uint32_t rbits : RBITS) {
    const uint64_t docs = 1ull << rbits;
    std::set<uint64_t> bases = {0ull, 1ull << 24, (1ull << 32) - docs};
    for (uint64_t base : bases) {
      if (base + docs > (1ull << 32)) continue; // (no such segment: mrk_segment_create refuses it)
      const uint32_t rhi = (uint32_t)(base + docs - 1);
      for (uint32_t sh : SHIFTS) {
        // -- by weight
        for (int32_t lo : LOS) {
          const SubKey sk = mrk::sub_key(BIN_WEIGHT, lo, sh, rbits, rhi);
          CHECK(sk.totbits == sh + rbits && sk.rhi == rhi && sk.rbits == rbits && sk.shift == sh && sk.lo == lo, "sub_key");
          ++g_geoms;
          for (uint32_t bin : {0u, 1u, 2u, 511u, 1022u, 1023u}) {
            const bool want = bin > 0 && bin < 1023 && sk.totbits <= 56;
            CHECK(mrk::sub_guard(sk, bin) == want, "weight mode shift %u rbits %u bin %u: guard %d", sh, rbits, bin, (int)mrk::sub_guard(sk, bin));
            if (!want) {
              ++(bin == 0 ? g_dec_bin0 : bin == 1023 ? g_dec_top : g_dec_wide);
              continue;
            }
            const int64_t w0 = (int64_t)lo + ((int64_t)bin << sh), w1 = std::min<int64_t>(w0 + (1ll << sh) - 1, INT32_MAX);
            if (w0 > INT32_MAX) {
              ++g_empty;
              continue;
            }
            ++g_accepted;
            (sk.totbits <= 11 ? g_tot_le11 : g_tot_gt11) = true;
            if (sk.totbits == 56) g_tot_56 = true;
            sub_monotone(sk, bin, w0, w1, base, rhi);
          }
        }
        // -- by rowid: the bins the segment's own rowids fall into, and the two edges
        const SubKey sk = mrk::sub_key(BIN_ROWID, 0, sh, rbits, rhi);
        CHECK(sk.totbits == sh, "sub_key by rowid");
        ++g_geoms;
        std::set<uint32_t> bins = {0u, 1023u, mrk::rowid_bin(sh, (uint32_t)base), mrk::rowid_bin(sh, rhi), mrk::rowid_bin(sh, (uint32_t)(base + docs / 2))};
        for (uint32_t bin : bins) {
          const bool want = bin > 0 && sh > 0;
          CHECK(mrk::sub_guard(sk, bin) == want, "rowid mode shift %u bin %u: guard %d", sh, bin, (int)mrk::sub_guard(sk, bin));
          if (!want) {
            ++(bin == 0 ? g_dec_bin0 : g_dec_nobits);
            continue;
          }
          const uint64_t top = 1023u - bin, r0 = std::max<uint64_t>(top << sh, base), r1 = std::min<uint64_t>(((top + 1) << sh) - 1, rhi);
          if (r0 > r1) {
            ++g_empty;
            continue;
          }
          ++g_accepted;
          (sk.totbits <= 11 ? g_tot_le11 : g_tot_gt11) = true;
          sub_monotone(sk, bin, 1, 1, r0, r1);
        }
      }
    }
  }
  // more than 56 bits: declined whatever the bin (the widest the grid above reaches is 31 + 32)
  for (uint32_t bin : {1u, 511u, 1022u}) {
    CHECK(mrk::sub_guard(mrk::sub_key(BIN_WEIGHT, 0, 31, 25, 0xFFFFFFu), bin), "56 bits are accepted");
    CHECK(!mrk::sub_guard(mrk::sub_key(BIN_WEIGHT, 0, 31, 26, 0xFFFFFFu), bin), "57 bits are declined");
    CHECK(!mrk::sub_guard(mrk::sub_key(BIN_ROWID, 0, 0, 20, 0xFFFFFu), bin), "no bits are declined");
  }
  CHECK(g_tot_le11 && g_tot_gt11 && g_tot_56, "totbits on both sides of 11 and at 56");
  CHECK(g_dec_bin0 && g_dec_top && g_dec_nobits && g_dec_wide, "every kind of decline met");
}

// ---- the planner's geometry for the GPU cases
struct Q {
  std::vector<mrk_node> nodes;
  std::vector<int32_t> children;
  mrk_query q;
};
static void make_query(Q& out, int n, int ranker) {
  out.nodes.assign((size_t)n + (n > 1 ? 1 : 0), mrk_node{});
  out.children.clear();
  for (int i = 0; i < n; ++i) {
    mrk_node& N = out.nodes[(size_t)i];
    N.op = MRK_OP_TERM, N.term_id = i, N.atom_pos = i + 1, N.field_mask = 0xFFFFFFFFu, N.boost = 1.0f;
    out.children.push_back(i);
  }
  if (n > 1) {
    mrk_node& N = out.nodes[(size_t)n];
    N.op = MRK_OP_AND, N.n_children = n, N.first_child = 0, N.field_mask = 0xFFFFFFFFu, N.boost = 1.0f;
  }
  memset(&out.q, 0, sizeof out.q);
  out.q.nodes = out.nodes.data(), out.q.n_nodes = (int32_t)out.nodes.size(), out.q.children = out.children.data(), out.q.root = (int32_t)out.nodes.size() - 1;
  out.q.ranker = ranker, out.q.max_matches = 1000, out.q.normalized_tfidf = 1;
}

static uint32_t g_dummy[16];
static void make_segment(mrk_segment& S, mrk_ctx* ctx, uint64_t total_docs, const std::vector<uint32_t>& df, uint32_t rowid_base) {
  S.ctx = ctx;
  S.total_docs = total_docs;
  S.n_fields = 2;
  S.has_packed = true;
  uint32_t blk = 0;
  for (size_t t = 0; t < df.size(); ++t) {
    HostTerm h;
    h.docs = df[t];
    h.hits = h.docs * 2, h.nblocks = (h.docs + 127) / 128, h.blk_first = blk, blk += h.nblocks;
    h.doclist_off = 1 + (uint64_t)t * 100000000ull, h.doclist_len = h.docs * 3ull, h.packed_bytes = h.docs * 2ull;
    h.last_rowid = (uint32_t)total_docs - 1 - (uint32_t)t;
    S.terms.push_back(h);
  }
  S.dev.n_windows = (uint32_t)((total_docs + 2047) / 2048);
  S.dev.pk_attr = g_dummy, S.dev.pk_hit = g_dummy, S.dev.bm = g_dummy;
  S.dev.rowid_base = rowid_base;
}

static int plan(const mrk_segment& S, Q& q, DevQuery& dq) {
  mrk::BatchPlan p;
  g_err[0] = 0;
  return mrk::plan_query(&S, q.q, 128 << 10, true, dq, 1, 0, p);
}

static int g_plans = 0, g_interior = 0;
static void planner(int argc, char** argv) {
  mrk_ctx ctx;
  const uint64_t docs = 240000;
  // case D: the shared corpus under SPH_RANK_NONE bins by rowid; the shift follows the segment's LAST global rowid
  const uint64_t bases[] = {0, 1ull << 24, (1ull << 32) - docs};
  const uint32_t want_shift[] = {8, 15, 22};
  for (int i = 0; i < 3; ++i) {
    mrk_segment S;
    make_segment(S, &ctx, docs, {60000, 60000}, (uint32_t)bases[i]);
    Q q;
    make_query(q, 2, MRK_RANK_NONE);
    DevQuery dq;
    const int rc = plan(S, q, dq);
    CHECK(rc == MRK_OK, "case D base %llu: %s", (unsigned long long)bases[i], g_err);
    if (rc != MRK_OK) continue;
    ++g_plans;
    CHECK(dq.bin_mode == BIN_ROWID && dq.bin_shift == want_shift[i] && dq.bin_lo == 0, "case D base %llu: mode %u shift %u", (unsigned long long)bases[i], dq.bin_mode, dq.bin_shift);
    const uint32_t r0 = (uint32_t)bases[i], r1 = (uint32_t)(bases[i] + docs - 1);
    const SubKey sk = mrk::sub_key(dq.bin_mode, dq.bin_lo, dq.bin_shift, 18, r1);
    const uint32_t b0 = mrk::rowid_bin(dq.bin_shift, r0), b1 = mrk::rowid_bin(dq.bin_shift, r1);
    if (i == 0) CHECK(b0 == 1023 && b1 > 0 && sk.totbits <= 11 && mrk::sub_guard(sk, b0) && mrk::sub_guard(sk, b1), "base 0: sub-bins of at most 11 bits");
    if (i == 1) CHECK(b0 > b1 && b1 > 0 && b0 < 1023 && sk.totbits > 11 && mrk::sub_guard(sk, b0) && mrk::sub_guard(sk, b1), "base 2^24: sub-bins over the top 11 of 15 rowid bits");
    if (i == 2) CHECK(b0 == 0 && b1 == 0 && r1 == 0xFFFFFFFFu && !mrk::sub_guard(sk, 0), "a range that ends at 2^32 - 1: every match in the clamped bin 0, no sub-bins");
  }
  // case E: field weights whose planned range leaves int32 -> the fallback geometry; every real weight lands in ONE sub-bin
  {
    mrk_segment S;
    make_segment(S, &ctx, docs, {60000, 60000}, 0);
    Q q;
    make_query(q, 2, MRK_RANK_BM25);
    const int32_t fw[2] = {2200000, 1};
    q.q.field_weights = fw, q.q.n_weights = 2;
    DevQuery dq;
    const int rc = plan(S, q, dq);
    CHECK(rc == MRK_OK, "case E: %s", g_err);
    if (rc == MRK_OK) {
      ++g_plans;
      CHECK(dq.bin_mode == BIN_WEIGHT && dq.bin_lo == INT32_MIN && dq.bin_shift == 31, "case E: lo %d shift %u", dq.bin_lo, dq.bin_shift);
      const SubKey sk = mrk::sub_key(dq.bin_mode, dq.bin_lo, dq.bin_shift, 18, (uint32_t)docs - 1);
      CHECK(mrk::weight_bin(dq.bin_lo, dq.bin_shift, 1) == 1 && mrk::weight_bin(dq.bin_lo, dq.bin_shift, 1 << 20) == 1 && mrk::sub_guard(sk, 1), "case E: the positive weights share bin 1, with sub-bins");
      CHECK(sk.sub(mrk::make_key(1, 0)) == 0 && sk.sub(mrk::make_key((1 << 20) - 1, (uint32_t)docs - 1)) == 0 && sk.sub(mrk::make_key(1 << 20, 0)) == 1, "case E: weights below 2^20 share sub-bin 0");
    }
  }
  // cases A-C (and F, G): the rank-K classes' weights, as the oracle gives them, lie in interior bins of the query's geometry
  for (int i = 1; i < argc; ++i) {
    unsigned long long n = 0, d0 = 0, d1 = 0;
    char ws[400] = "";
    const int two = sscanf(argv[i], "%llu:%llu:%llu:%399s", &n, &d0, &d1, ws) == 4;
    if (!two && sscanf(argv[i], "%llu:%llu:%399s", &n, &d0, ws) != 3) {
      CHECK(false, "argument '%s'", argv[i]);
      continue;
    }
    mrk_segment S;
    std::vector<uint32_t> df = {(uint32_t)d0};
    if (two) df.push_back((uint32_t)d1);
    make_segment(S, &ctx, n, df, 0);
    Q q;
    make_query(q, two ? 2 : 1, MRK_RANK_BM25);
    DevQuery dq;
    const int rc = plan(S, q, dq);
    CHECK(rc == MRK_OK, "'%s': %s", argv[i], g_err);
    if (rc != MRK_OK) continue;
    ++g_plans;
    CHECK(dq.bin_mode == BIN_WEIGHT && dq.bin_shift < 31, "'%s': lo %d shift %u", argv[i], dq.bin_lo, dq.bin_shift);
    for (char* tok = strtok(ws, ","); tok; tok = strtok(nullptr, ",")) {
      const int32_t w = (int32_t)atol(tok);
      const uint32_t b = mrk::weight_bin(dq.bin_lo, dq.bin_shift, w);
      CHECK(b > 0 && b < 1023, "'%s': weight %d in edge bin %u (lo %d shift %u)", argv[i], w, b, dq.bin_lo, dq.bin_shift);
      ++g_interior;
    }
  }
}

int main(int argc, char** argv) {
  bin_monotone();
  sub_bins();
  planner(argc, argv);
  if (g_bad) return printf("%d checks failed\n", g_bad), 1;
  printf("ok bins %llu keys; sub-bins %d geometries %d accepted (%llu exhaustive %llu sampled, %llu keys) declined %d bin0 %d top %d nobits %d wide, %d empty; plans %d interior %d\n",
         (unsigned long long)g_bin_keys, g_geoms, g_accepted, (unsigned long long)g_exhaustive, (unsigned long long)g_sampled, (unsigned long long)g_sub_keys, g_dec_bin0, g_dec_top,
         g_dec_nobits, g_dec_wide, g_empty, g_plans, g_interior);
  return 0;
}
