// pk_probe.cpp -- one doc of a packed block read on its own (mrk::pk_doc_off, mrk::pk_lower_bound, csrc/mrk_kpk.h: what the
// lean block scan's probe of a sparse second keyword runs per lane) against the plain decode, on the CPU.
// Doclists are written in the reference's VLB format and packed by mrk::pack_term (csrc/mrk_pack.cpp): for every width 0 .. 16
// and for PK_WIDE, at the smallest and the largest last offset of that width, with 1, 2, 63, 64, 65, 127 and 128 docs in the
// block under test -- as a term's only block and behind a full block (a base other than 0).  Checked: the offset of every doc,
// and the lower bound and the hit test for every rowid from base - 1 to last + 1 (blocks that span more than 4096 rowids: the
// block's docs and their neighbours).  The packed words are vectors of exactly the packed size: a read past a block's spare word
// is AddressSanitizer's to report.
// Built and run by tests/test_pk_probe_cpu.py; no GPU, no libmrk.so.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../manticoresearch_amd/csrc/mrk_kpk.h"
#include "../../manticoresearch_amd/csrc/mrk_pack.h"

static uint64_t g_s = 0x5EEDull;
static uint64_t rnd() {
  g_s += 0x9E3779B97F4A7C15ull;
  uint64_t z = g_s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(c, ...)                                       \
  do {                                                      \
    if (!(c)) {                                             \
      fprintf(stderr, "FAIL %s:%d: %s ", __FILE__, __LINE__, #c); \
      fprintf(stderr, __VA_ARGS__);                         \
      fprintf(stderr, "\n");                                \
      exit(1);                                              \
    }                                                       \
  } while (0)

static void vlb(std::vector<uint8_t>& out, uint64_t v) {
  uint8_t tmp[10];
  int n = 0;
  do tmp[n++] = (uint8_t)(v & 0x7f), v >>= 7;
  while (v);
  while (n--) out.push_back((uint8_t)(tmp[n] | (n ? 0x80 : 0)));
}

// n distinct offsets in [0, dmax], ascending, the last one dmax
static std::vector<uint32_t> offsets(uint32_t n, uint32_t dmax) {
  std::vector<uint32_t> o;
  if ((uint64_t)n - 1 > dmax / 2) { // dense: draw what to leave out
    std::vector<uint32_t> all(dmax);
    for (uint32_t i = 0; i < dmax; ++i) all[i] = i;
    for (uint32_t i = 0; i + 1 < n; ++i) std::swap(all[i], all[i + (uint32_t)(rnd() % (dmax - i))]);
    o.assign(all.begin(), all.begin() + (n - 1));
  } else
    while (o.size() + 1 < n) {
      const uint32_t v = (uint32_t)(rnd() % dmax);
      if (std::find(o.begin(), o.end(), v) == o.end()) o.push_back(v);
    }
  o.push_back(dmax);
  std::sort(o.begin(), o.end());
  return o;
}

static uint64_t g_blocks = 0, g_probes = 0;

// every doc and every rowid around them of block b of the packed term P, whose docs are rows[first .. first + nd)
static void check_block(const mrk::PackedTerm& P, uint32_t b, const std::vector<uint32_t>& rows, uint32_t first, uint32_t nd) {
  const uint32_t* dp = P.delta.data() + P.doff[b];
  const uint32_t w = P.w[b], base = P.base[b];
  std::vector<uint32_t> off(nd);
  for (uint32_t i = 0; i < nd; ++i) {
    off[i] = rows[first + i] - base;
    CHECK(mrk::pk_doc_off(dp, w, i) == off[i], "w %u nd %u doc %u: offset %u, packed from %u", w, nd, i, mrk::pk_doc_off(dp, w, i), off[i]);
  }
  auto probe = [&](uint64_t row64) {
    if (row64 > 0xFFFFFFFEull) return;
    const uint32_t row = (uint32_t)row64;
    ++g_probes;
    // (a row below the base belongs to an earlier block: the kernel never asks this block for it)
    const int64_t want_hit = row >= base && std::binary_search(off.begin(), off.end(), row - base) ? (int64_t)(std::lower_bound(off.begin(), off.end(), row - base) - off.begin()) : -1;
    if (row < base) return;
    const uint32_t want = row - base;
    const uint32_t lb = (uint32_t)(std::lower_bound(off.begin(), off.end(), want) - off.begin());
    const uint32_t pos = mrk::pk_lower_bound(dp, w, nd, want);
    CHECK(pos == std::min(lb, 127u), "w %u nd %u row %u: lower bound %u, %u docs lie below", w, nd, row, pos, lb);
    const bool hit = pos < nd && mrk::pk_doc_off(dp, w, pos) == want;
    CHECK((hit ? (int64_t)pos : -1) == want_hit, "w %u nd %u row %u: hit at %lld, doc %lld holds it", w, nd, row, hit ? (long long)pos : -1ll, (long long)want_hit);
  };
  const uint64_t last = rows[first + nd - 1];
  if (last - base <= 4096)
    for (uint64_t r = base ? base - 1 : 0; r <= last + 1; ++r) probe(r);
  else
    for (uint32_t i = 0; i < nd; ++i)
      for (int d = -1; d <= 1; ++d) probe((uint64_t)((int64_t)rows[first + i] + d));
  probe(base ? base - 1 : 0), probe(base), probe(last + 1), probe(last + 70000), probe(0xFFFFFFFEull);
  ++g_blocks;
}

// a term of `lead` full blocks and one block of nd docs whose last offset is dmax; returns false where no such block exists
static bool run_case(uint32_t lead, uint32_t nd, uint32_t dmax, uint32_t want_w) {
  if ((uint64_t)nd - 1 > dmax) return false;
  std::vector<uint32_t> rows;
  uint32_t next = 0;
  for (uint32_t l = 0; l < lead; ++l) {
    const uint32_t lead_max = 127u + (uint32_t)(rnd() % 3000);
    for (uint32_t o : offsets(128, lead_max)) rows.push_back(next + o);
    next = rows.back() + 1;
  }
  const uint32_t first = (uint32_t)rows.size();
  for (uint32_t o : offsets(nd, dmax)) rows.push_back(next + o);
  std::vector<uint8_t> spd(1, 0); // (a doclist never starts at offset 0)
  uint32_t prev = 0xFFFFFFFFu;
  for (uint32_t r : rows) {
    vlb(spd, r - prev), prev = r; // rowid delta from INVALID_ROWID
    vlb(spd, 1 + rnd() % 50);     // hitlist offset delta
    vlb(spd, 1 + rnd() % 255);    // field mask
    vlb(spd, 1 + rnd() % 300);    // hits
  }
  spd.push_back(0);
  mrk_dict_entry e{};
  e.doclist_off = 1, e.doclist_len = spd.size() - 1, e.docs = (uint32_t)rows.size();
  mrk::PackedTerm P;
  std::string err;
  CHECK(mrk::pack_term(spd.data(), spd.size(), e, false, 0, P, err), "pack_term: %s", err.c_str());
  CHECK(P.w.size() == lead + 1 && P.w[lead] == want_w, "the block under test has width %u, %u wanted (nd %u dmax %u)", P.w.empty() ? 0u : P.w[lead], want_w, nd, dmax);
  CHECK(P.delta.size() == (size_t)P.doff[lead] + (want_w == mrk::PK_WIDE ? 128u : 4u * want_w + 1u), "the packed words end where the last block does");
  for (uint32_t b = 0; b <= lead; ++b) check_block(P, b, rows, b * 128, b < lead ? 128u : nd);
  return true;
}

int main() {
  static const uint32_t nds[7] = {1, 2, 63, 64, 65, 127, 128};
  uint32_t cases = 0, widths_seen = 0;
  for (uint32_t w = 0; w <= 17; ++w) { // 17: PK_WIDE
    const uint32_t lo = w == 0 ? 0u : 1u << (w - 1), hi = w == 17 ? 1u << 30 : (1u << w) - 1u;
    bool any = false;
    for (uint32_t nd : nds)
      for (uint32_t lead = 0; lead < 2; ++lead)
        for (uint32_t dmax : {std::max(lo, nd - 1), hi}) {
          if (dmax > hi) continue;
          if (run_case(lead, nd, dmax, w == 17 ? mrk::PK_WIDE : w)) ++cases, any = true;
        }
    CHECK(any, "no block of width %u was built", w);
    ++widths_seen;
  }
  printf("ok %u widths %u cases %llu blocks %llu probes\n", widths_seen, cases, (unsigned long long)g_blocks, (unsigned long long)g_probes);
  return 0;
}
