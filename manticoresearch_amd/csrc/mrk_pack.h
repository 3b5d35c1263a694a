// mrk_pack.h -- load-time transcode of one term's VLB doclist into packed 128-doc blocks.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mrk.h"

namespace mrk {

struct PackedTerm {
  std::vector<uint32_t> base;  // per block
  std::vector<uint32_t> doff;  // per block, word offset relative to this term's delta run
  std::vector<uint8_t> w;      // per block
  std::vector<uint32_t> delta; // this term's delta run
  std::vector<uint32_t> attr;  // 64 words per block
  std::vector<uint64_t> exc;   // rowid<<32 | tf for tf >= 255
  // one byte per doc slot for the bitmap kernel's gathers (half the bytes of the attr words): tf in the low nibble
  // (15 = look at the attr word), fields in the high one; attr1_ok = false when a doc has a field bit >= 4
  std::vector<uint8_t> attr1;
  // dense terms only (bitmap_rows != 0): tf | fields << 8 per doc slot IN SLOT ORDER (the attr words above interleave slots l and l + 64
  // for the block decoder; the bitmap kernel gathers by rank, and a line whose docs are scored rounds apart is fetched twice)
  std::vector<uint16_t> attr2;
  bool attr1_ok = true;
  uint32_t last_rowid = 0; // rowid of the term's last doc
  std::vector<uint32_t> hit;   // 128 per block: the inlined Hitpos_t (inline format, tf == 1) or the doc's
                               // hitlist offset in .spp relative to hbase[block]
  std::vector<uint64_t> hbase; // per block: .spp position of the block's first hitlist
  std::vector<uint32_t> fmask; // wide layout only (9-32 fields): 128 per block, the doc's field mask per slot (indexed like hit);
                               // the attr words' field bytes stay zero
  uint64_t packed_bytes = 0;   // bytes a scan of the whole term reads (deltas + attrs + block index)
  // dense terms only (bitmap_rows != 0): the doc set as a bitmap over [0, bitmap_rows), one 2048-rowid
  // window = 64 words, plus a rank directory (docs before each group of 8 words = 256 rowids).
  // A doc's rank is its slot in the packed arrays above (block = rank >> 7, slot = rank & 127).
  std::vector<uint32_t> bm;
  std::vector<uint32_t> bm_dir;
  // ... and, with bm_wmax, one nibble per bitmap word: min(15, the largest hit count among the term's postings whose rowid
  // falls in that word), 0 for an empty word.  Four windows share 64 16-bit words: word wmax[(w >> 2) * 64 + l] holds in nibble
  // w & 3 the class of word l of window w, so a wave reads its lanes' classes for four aligned windows with one 128-byte load.
  // The last group is padded with empty windows.  Empty for a term with a posting of no hits (malformed: no bound holds for it).
  std::vector<uint16_t> wmax;
};

constexpr uint32_t BM_WINDOW = 2048; // rowids per bitmap window (64 lanes x 32 bits)
constexpr uint32_t BM_GROUP = 256;   // rowids per rank-directory entry
constexpr uint32_t BM_WMAX_WINDOWS = 4; // windows per group of the wmax plane (64 16-bit words)

// 16-bit words of a term's wmax plane, and the class of bitmap word `word` (term-local: window * 64 + lane) in it
inline size_t bm_wmax_words(uint64_t windows) { return (size_t)((windows + BM_WMAX_WINDOWS - 1) / BM_WMAX_WINDOWS) * 64; }
inline uint32_t bm_wmax_class(const uint16_t* wmax, uint64_t word) {
  const uint64_t w = word >> 6;
  return (wmax[(w >> 2) * 64 + (word & 63u)] >> ((w & 3u) * 4u)) & 15u;
}

// returns false and sets err on input it cannot pack; err starts with "corrupt:" when the bytes are malformed (truncated
// entries, descending rowids, rowids >= total_rows, hitlist offsets >= spp_len; the last two only when the limit is
// given) -- as opposed to well-formed input beyond the packed format (field masks wider than 8 bits in the narrow layout)
// bitmap_rows: 0 = no bitmap; else the segment's row count (every rowid of the term must be below it)
// bm_wmax: with a bitmap, also build the per-word tf-class plane (PackedTerm::wmax)
// wide: the layout of a segment with 9-32 fields -- every mask fits, it goes to out.fmask
bool pack_term(const uint8_t* spd, uint64_t spd_len, const mrk_dict_entry& e, bool inline_hits, uint64_t bitmap_rows,
               PackedTerm& out, std::string& err, uint64_t total_rows = 0, uint64_t spp_len = 0, bool wide = false, bool bm_wmax = false);

// Validate-only walk of one term's doclist: every entry decodes, rowids ascend and stay below total_rows, hitlist
// offsets stay below spp_len, the terminator sits where the dictionary's doc count says.  false + err ("corrupt: ...")
// otherwise.  mrk_segment_create runs it on every doclist pack_term did not walk to the end (pack = 0, a packing decline half way): nothing unvalidated reaches a kernel.
bool validate_term(const uint8_t* spd, uint64_t spd_len, const mrk_dict_entry& e, bool inline_hits, uint64_t total_rows,
                   uint64_t spp_len, std::string& err);

} // namespace mrk
