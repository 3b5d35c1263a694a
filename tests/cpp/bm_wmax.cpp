// bm_wmax.cpp -- the per-word tf-class plane of the two-bitmap AND kernel (ctx key bm_wmax) on the CPU, under AddressSanitizer + UBSan.
//   1. mrk::pack_term's plane (PackedTerm::wmax, csrc/mrk_pack.cpp) against the per-word maximum recomputed from the postings the index
//      was written from: words whose only posting has tf 14, 15, 254, 255 or 300, an empty word, a word whose largest tf sits between
//      tf-1 postings, the last partial window of a doc count that is no multiple of 2048, groups of four windows that end early, both hit
//      formats; no plane without the flag, none for a term that gets no bitmap.  (The packer sees segment-local rowids only: a segment's
//      rowid_base never reaches it, the GPU test covers it.)
//   2. mrk::bm_wmax_bound (csrc/mrk_kcommon.h, the function the kernel calls) against mrk::term_tfidf, as floats: for every tf in 1..300
//      and every class a word holding that posting can have, for idf > 0, = 0 and < 0.
// Built and run by tests/test_bm_wmax_cpu.py; no GPU, no libmrk.so.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_kcommon.h"
#include "../../manticoresearch_amd/csrc/mrk_pack.h"

int mrk_fail(int code, const char* fmt, ...) { return code; }

static int g_bad = 0;
#define CHECK(c, ...)                        \
  do {                                       \
    if (!(c)) {                              \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);          \
      fprintf(stderr, "\n");                 \
      if (++g_bad > 20) exit(1);             \
    }                                        \
  } while (0)

static uint64_t g_s = 99;
static uint64_t rnd() {
  g_s += 0x9E3779B97F4A7C15ull;
  uint64_t z = g_s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// rowid -> tf of one term
typedef std::map<uint32_t, uint32_t> Postings;

static Postings make_term(uint32_t n_docs, bool planted, uint32_t dense_pct) {
  Postings p;
  const uint32_t first_random = planted ? 32 * 8 : 0;
  for (uint32_t r = first_random; r < n_docs; ++r)
    if (rnd() % 100 < dense_pct) {
      uint32_t tf = 1;
      while (tf < 40 && (rnd() & 1)) ++tf;
      p[r] = tf;
    }
  if (planted) {
    p[5] = 14, p[40] = 15, p[70] = 254, p[100] = 255, p[130] = 300; // words 0..4: one posting each
    // word 5 (rowids 160..191) stays empty
    for (uint32_t r = 192; r < 224; ++r) p[r] = 1; // word 6: the largest tf between tf-1 postings
    p[200] = 7;
    p[n_docs - 1] = 9; // the segment's last row
  }
  return p;
}

static int check_corpus(uint32_t n_docs, uint32_t hit_format) {
  std::vector<Postings> terms;
  terms.push_back(make_term(n_docs, true, 30));
  terms.push_back(make_term(n_docs, false, 10));
  terms.push_back(make_term(n_docs, false, 60));
  std::vector<uint64_t> W;
  std::vector<uint32_t> R, H;
  for (size_t t = 0; t < terms.size(); ++t)
    for (const auto& kv : terms[t])
      for (uint32_t h = 1; h <= kv.second; ++h) { // (sorted by hit position: the field is the high byte)
        W.push_back(t + 1), R.push_back(kv.first);
        H.push_back(((h > (kv.second + 1) / 2 ? 1u : 0u) << 24) | h);
      }
  mrk_host_index* hi = nullptr;
  if (mrk_index_from_hits(W.data(), R.data(), H.data(), W.size(), (uint32_t)terms.size(), 128, hit_format, &hi) != MRK_OK) return 2;
  uint64_t spd_len = 0;
  const uint8_t* spd = mrk_host_index_spd(hi, &spd_len);
  uint32_t nt = 0;
  const mrk_dict_entry* dict = mrk_host_index_dict(hi, &nt);
  const bool inl = hit_format == MRK_HITFMT_INLINE;
  const uint64_t windows = (n_docs + 2047) / 2048;
  for (uint32_t t = 0; t < nt; ++t) {
    std::string err;
    mrk::PackedTerm pt;
    CHECK(mrk::pack_term(spd, spd_len, dict[t], inl, n_docs, pt, err, n_docs, 0, false, true), "term %u: %s", t, err.c_str());
    CHECK(pt.bm.size() == windows * 64, "term %u: %zu bitmap words", t, pt.bm.size());
    CHECK(pt.wmax.size() == mrk::bm_wmax_words(windows) && pt.wmax.size() == (windows + 3) / 4 * 64, "term %u: %zu plane words for %llu windows", t,
          pt.wmax.size(), (unsigned long long)windows);
    if (pt.wmax.size() != mrk::bm_wmax_words(windows)) continue;
    std::vector<uint32_t> want((size_t)(windows + 3) / 4 * 4 * 64, 0u); // per word, the padding windows of the last group too
    for (const auto& kv : terms[t]) {
      uint32_t& x = want[kv.first >> 5];
      const uint32_t c = kv.second < 15u ? kv.second : 15u;
      if (c > x) x = c;
    }
    for (size_t w = 0; w < want.size(); ++w) {
      const uint32_t got = mrk::bm_wmax_class(pt.wmax.data(), w);
      CHECK(got == want[w], "docs %u term %u word %zu: class %u, postings say %u", n_docs, t, w, got, want[w]);
      if (w < pt.bm.size()) CHECK((pt.bm[w] != 0) == (got != 0), "docs %u term %u word %zu: bitmap %08x, class %u", n_docs, t, w, pt.bm[w], got);
    }
    if (t == 0) {
      const uint32_t planted[7] = {14, 15, 15, 15, 15, 0, 7};
      for (uint32_t w = 0; w < 7; ++w) CHECK(mrk::bm_wmax_class(pt.wmax.data(), w) == planted[w], "planted word %u", w);
      CHECK(mrk::bm_wmax_class(pt.wmax.data(), (n_docs - 1) >> 5) >= 9u, "the last row's word");
    }
    // the layout itself: lane l's 16-bit word of group g holds windows 4g .. 4g + 3 in nibbles 0 .. 3
    for (uint64_t w = 0; w < windows; ++w)
      for (uint32_t l = 0; l < 64; ++l)
        CHECK(((pt.wmax[(w >> 2) * 64 + l] >> ((w & 3) * 4)) & 15u) == want[w * 64 + l], "layout: window %llu lane %u", (unsigned long long)w, l);
    mrk::PackedTerm off;
    CHECK(mrk::pack_term(spd, spd_len, dict[t], inl, n_docs, off, err, n_docs) && off.wmax.empty() && off.bm == pt.bm && off.attr2 == pt.attr2,
          "term %u: without the flag", t);
    mrk::PackedTerm none;
    CHECK(mrk::pack_term(spd, spd_len, dict[t], inl, 0, none, err, n_docs, 0, false, true) && none.wmax.empty() && none.bm.empty(), "term %u: no bitmap, no plane", t);
    mrk::PackedTerm cut; // a rowid past the rows the bitmap covers (term 0 holds the last row): the term loses its bitmap, and the plane with it
    if (t == 0) CHECK(mrk::pack_term(spd, spd_len, dict[t], inl, n_docs / 2, cut, err, 0, 0, false, true) && cut.wmax.empty() && cut.bm.empty(), "term %u: cut bitmap", t);
  }
  mrk_host_index_free(hi);
  return 0;
}

// a posting with a hit count of 0 (malformed, but pack_term packs it): score() would add a tfidf of 0, above every bound of a negative
// idf -- the term keeps its bitmap and gets no plane
static void check_hitless_posting() {
  // plain format, per doc: rowid delta, hitlist offset delta, fields, hits; a 0 ends the list (byte 0 pads: offsets start at 1)
  const uint8_t spd[] = {0, 1, 1, 1, 2, 5, 1, 1, 0, 3, 1, 1, 1, 0};
  mrk_dict_entry e;
  memset(&e, 0, sizeof e);
  e.wordid = 1, e.doclist_off = 1, e.doclist_len = sizeof spd - 1, e.docs = 3, e.hits = 3;
  std::string err;
  mrk::PackedTerm pt, ok;
  CHECK(mrk::pack_term(spd, sizeof spd, e, false, 100, pt, err, 100, 0, false, true), "hitless posting: %s", err.c_str());
  CHECK(pt.bm.size() == 64 && pt.bm[0] == ((1u << 0) | (1u << 5) | (1u << 8)) && pt.wmax.empty(), "hitless posting: bitmap %zu words, plane %zu", pt.bm.size(), pt.wmax.size());
  const uint8_t good[] = {0, 1, 1, 1, 2, 5, 1, 1, 1, 3, 1, 1, 1, 0};
  CHECK(mrk::pack_term(good, sizeof good, e, false, 100, ok, err, 100, 0, false, true) && ok.wmax.size() == 64 && mrk::bm_wmax_class(ok.wmax.data(), 0) == 2u,
        "the same list with a hit: plane %zu", ok.wmax.size());
}

static void check_bounds() {
  const float idfs[] = {0.0f, 1e-30f, 0.0123f, 0.19f, 0.25f, 0.333333f, 0.5f, 0.731f, 1.0f, 3.7f, -1e-30f, -0.004f, -0.0461f, -0.25f, -0.5f, -1.0f};
  std::vector<float> more(idfs, idfs + sizeof idfs / sizeof idfs[0]);
  for (int i = 0; i < 400; ++i) { // idfs as the planner makes them: any fraction of 0.5, either sign
    const float f = (float)(rnd() % 1000001) / 1000000.0f * 0.5f;
    more.push_back(i & 1 ? -f : f);
  }
  size_t n = 0;
  for (float idf : more) {
    float tab[256];
    for (uint32_t t = 0; t < 256; ++t) tab[t] = mrk::term_tfidf(t, idf);
    for (uint32_t tf = 1; tf <= 300; ++tf) {
      const float real = tf < 255u ? tab[tf] : mrk::term_tfidf(tf, idf); // (what score() adds: the table's entry below 255, the escape's lookup from there)
      const uint32_t own = tf < 15u ? tf : 15u;
      for (uint32_t cls = own; cls <= 15u; ++cls) { // the word's class is its largest: this posting's or a higher one
        const float b = mrk::bm_wmax_bound(cls, idf);
        CHECK(b >= real, "idf %.9g tf %u class %u: bound %.9g < %.9g", (double)idf, tf, cls, (double)b, (double)real);
        ++n;
      }
    }
  }
  printf("bounds %zu\n", n);
}

int main() {
  for (uint32_t fmt = 0; fmt < 2; ++fmt) {
    const uint32_t docs[] = {2048 * 2 + 777, 2048 * 8 + 100, 2048 * 4, 300};
    for (uint32_t nd : docs)
      if (int rc = check_corpus(nd, fmt)) return rc;
  }
  check_hitless_posting();
  check_bounds();
  if (g_bad) return 1;
  printf("ok\n");
  return 0;
}
