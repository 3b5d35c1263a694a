// mrk_sortkey.h -- the order-preserving 32-bit map of a sorter's primary attribute (mrk_query.sort), one definition for the
// planner, the kernels and the CPU unit test.  "Larger mapped key = better" always holds: unsigned integers as they are,
// floats by the usual sign flip with -0.0 folded onto +0.0 (SPH_KEYPART_FLOAT compares floats: the two zeros are equal and
// the comparison falls through to the next key part), ascending orders complemented.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRK_HD __host__ __device__
#else
#define MRK_HD
#endif

namespace mrk {

// candidate key of the relevance order, and the format every result row leaves in: bigger = better under MatchRelevanceLt_fn
// (weight desc, rowid asc)
MRK_HD inline uint64_t make_key(int32_t weight, uint32_t rowid) { return ((uint64_t)((uint32_t)weight ^ 0x80000000u) << 32) | (uint32_t)(~rowid); }
MRK_HD inline int32_t key_weight(uint64_t k) { return (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u); }
MRK_HD inline uint32_t key_rowid(uint64_t k) { return ~(uint32_t)k; }

constexpr uint32_t SORT_FLOAT = 1, SORT_DESC = 2; // DevQuery::sort_flags

// the attribute's bits out of its dword (sphGetRowAttr, sphinx.h:993-1014, for locators of <= 32 bits)
MRK_HD inline uint32_t sort_extract(uint32_t dword, uint32_t shift, uint32_t bits) { return bits >= 32u ? dword : (dword >> shift) & ((1u << bits) - 1u); }

MRK_HD inline bool sort_is_nan(uint32_t v) { return (v & 0x7FFFFFFFu) > 0x7F800000u; }

MRK_HD inline uint32_t sort_map_key(uint32_t v, uint32_t flags) {
  uint32_t m = v;
  if (flags & SORT_FLOAT) {
    if ((v << 1) == 0u) v = 0u; // -0.0 == +0.0
    m = (v & 0x80000000u) ? ~v : (v | 0x80000000u);
  }
  return (flags & SORT_DESC) ? m : ~m;
}

// The sort spec word of a wide exchange row (MRK_SROW_WORDS, include/mrk.h): everything that decides whether two shards' mapped
// keys and tie rules compare, and nothing of where a segment stores the column.  0 = a relevance query.
//   bit 0 sorted | bit 1 float | bit 2 desc | bits 4-5 then_weight | bits 8-13 bit_count
constexpr uint64_t SPEC_SORTED = 1, SPEC_FLOAT = 2, SPEC_DESC = 4;
MRK_HD inline uint64_t sort_spec_word(uint32_t flags, uint32_t tie, uint32_t bits) {
  return SPEC_SORTED | ((flags & SORT_FLOAT) ? SPEC_FLOAT : 0u) | ((flags & SORT_DESC) ? SPEC_DESC : 0u) | ((uint64_t)(tie & 3u) << 4) | ((uint64_t)(bits & 63u) << 8);
}
MRK_HD inline uint32_t sort_spec_tie(uint64_t spec) { return spec ? (uint32_t)(spec >> 4) & 3u : 1u; } // relevance = weight desc

// the inverse of sort_map_key under a spec word: the attribute's raw value (a float's -0.0 was folded onto +0.0 and reads +0.0)
MRK_HD inline uint32_t sort_unmap_key(uint64_t spec, uint32_t mapped) {
  const uint32_t m = (spec & SPEC_DESC) ? mapped : ~mapped;
  if (!(spec & SPEC_FLOAT)) return m;
  return (m & 0x80000000u) ? (m ^ 0x80000000u) : ~m;
}

// pruning bin of a mapped key: monotone non-decreasing in it; lo / shift come from the column's range (mrk_plan.cpp)
MRK_HD inline uint32_t sort_bin(uint32_t lo, uint32_t shift, uint32_t mapped) {
  if (mapped < lo) return 0u;
  const uint32_t b = (mapped - lo) >> shift;
  return b < 1023u ? b : 1023u;
}

// pruning bin of a weight (the relevance order's BIN_WEIGHT bins: bin_of of mrk_kprune.h calls this): monotone non-decreasing in it,
// 1024 bins; lo / shift = DevQuery::bin_lo / bin_shift as bins_by_weight (mrk_plan.cpp) sets them
MRK_HD inline uint32_t weight_bin(int32_t lo, uint32_t shift, int32_t weight) {
  if (weight < lo) return 0u;
  const uint32_t b = ((uint32_t)weight - (uint32_t)lo) >> shift; // (== (uint32_t)(weight - lo), without the signed overflow)
  return b < 1024u ? b : 1023u;
}

constexpr uint32_t BIN_WEIGHT = 0, BIN_ROWID = 1; // DevQuery::bin_mode: what the relevance order's pruning histogram is keyed on

// pruning bin of a GLOBAL rowid (the BIN_ROWID bins of a query whose weights are all equal: the order is rowid ascending, so lower
// rowids sit in higher bins): monotone non-decreasing in the order, 1024 bins; shift as bins_by_rowid (mrk_plan.cpp) sets it.
// Rowids of 1023 << shift and beyond share the clamped bin 0
MRK_HD inline uint32_t rowid_bin(uint32_t shift, uint32_t grow) {
  const uint32_t b = grow >> shift;
  return 1023u - (b < 1024u ? b : 1023u);
}

// Order of a relevance key INSIDE its pruning bin, bigger = better, as a number of `totbits` bits of which sub() hands out the top
// SUB_BITS (all of them where there are fewer): the sub-bins of the selection's sort pass (sel_sort_kernel, mrk_select.hip).
//   BIN_WEIGHT  (weight offset inside the bin) << rbits | rhi - global rowid      rhi / rbits: the segment's largest global rowid and
//   BIN_ROWID   2^shift - 1 - (global rowid mod 2^shift)                          the bits of its rowid count - 1
// Only where sub_guard() holds is this an order of the bin's keys.
constexpr uint32_t SUB_BITS = 11;
struct SubKey {
  uint32_t mode, shift, rbits, rhi, totbits;
  int32_t lo;
  MRK_HD inline uint32_t sub(uint64_t key) const {
    const uint32_t grow = key_rowid(key);
    uint64_t ok;
    if (mode == BIN_WEIGHT) {
      const uint32_t woff = shift ? (((uint32_t)key_weight(key) - (uint32_t)lo) & ((1u << shift) - 1u)) : 0u; // (unsigned: no signed overflow, as in weight_bin)
      ok = ((uint64_t)woff << rbits) | (uint64_t)(rhi - grow);
    } else
      ok = (uint64_t)(((1u << shift) - 1u) - (grow & ((1u << shift) - 1u)));
    return totbits > SUB_BITS ? (uint32_t)(ok >> (totbits - SUB_BITS)) : (uint32_t)ok;
  }
};
// mode / lo / shift = DevQuery::bin_mode / bin_lo / bin_shift; rowid_bits / rowid_hi = SelectArgs' (mrk_dev.h)
MRK_HD inline SubKey sub_key(uint32_t mode, int32_t lo, uint32_t shift, uint32_t rowid_bits, uint32_t rowid_hi) {
  return SubKey{mode, shift, rowid_bits, rowid_hi, mode == BIN_WEIGHT ? shift + rowid_bits : shift, lo};
}
// May the keys of threshold bin tau_bin be told apart by sub()?  Not in the edge bins, which are open-ended (bin 0 of either mode holds
// everything below the range or beyond the clamp, bin 1023 of the weight's everything above: no finite sub-order), not without a bit
// to tell by, and not where the order would not fit the 64-bit arithmetic of sub() with room to spare
MRK_HD inline bool sub_guard(const SubKey& sk, uint32_t tau_bin) {
  return tau_bin > 0u && sk.totbits > 0u && sk.totbits <= 56u && (sk.mode == BIN_ROWID || tau_bin < 1023u);
}

// A candidate of a sorted query is 128 bits, compared as (hi, lo), larger = better:
//   hi = mapped key << 32 | the weight as the tie rule orders it (0 where the weight is no part of the order)
//   lo = ~global rowid << 32 | the true weight
MRK_HD inline uint32_t sort_weight_part(uint32_t tie, int32_t weight) {
  const uint32_t w = (uint32_t)weight ^ 0x80000000u;
  return tie == 1u ? w : tie == 2u ? ~w : 0u;
}

// ---------------------------------------------------------------------------------------
// The wider order (mrk_query.order): ONE signed 64-bit attribute, or TWO attributes of <= 32 bits.  Both are two dwords to the
// device: a 64-bit attribute is its high dword compared as a signed integer, then its low dword as an unsigned one, both in the
// attribute's direction.  The mapped key is 64 bits, larger = better: map32(first) << 32 | map32(second).
//   hi = the 64-bit mapped key
//   lo = weight as the tie rule orders it << 32 | ~global rowid      then_weight 1 / 2 (the true weight comes back out of the part)
//   lo = ~global rowid << 32 | the true weight                       then_weight 0
// ---------------------------------------------------------------------------------------
constexpr uint32_t SORT_SIGNED = 4;                // a part's flags: the dword is a signed integer (the high dword of an int64)
constexpr uint32_t SORT_WIDE = 8;                  // DevQuery::sort_flags of a query with sort_on == SORT_ON_ORDER (the kernels test this bit of a word they hold anyway)
constexpr uint32_t SORT_ON_ATTR = 1, SORT_ON_ORDER = 2; // DevQuery::sort_on

MRK_HD inline uint32_t order_map_part(uint32_t v, uint32_t flags) { return sort_map_key((flags & SORT_SIGNED) ? v ^ 0x80000000u : v, flags); }
// the part's raw value (a float's -0.0 reads +0.0)
MRK_HD inline uint32_t order_unmap_part(uint32_t mapped, uint32_t flags) {
  const uint32_t v = sort_unmap_key(((flags & SORT_FLOAT) ? SPEC_FLOAT : 0u) | ((flags & SORT_DESC) ? SPEC_DESC : 0u), mapped);
  return (flags & SORT_SIGNED) ? v ^ 0x80000000u : v;
}
MRK_HD inline uint64_t order_key(uint32_t a, uint32_t b) { return ((uint64_t)a << 32) | b; }
// where a part lives in the row and how it compares: dword, bit offset inside it, width, SORT_FLOAT | SORT_DESC | SORT_SIGNED
struct OrderPart {
  uint32_t item, shift, bits, flags;
};
// the 64-bit mapped key of an attribute row
MRK_HD inline uint64_t order_row_key(const uint32_t* row, const OrderPart& p0, const OrderPart& p1) {
  return order_key(order_map_part(sort_extract(row[p0.item], p0.shift, p0.bits), p0.flags), order_map_part(sort_extract(row[p1.item], p1.shift, p1.bits), p1.flags));
}
// a signed 64-bit attribute as one mapped key, and back (== order_key over its dwords: high SORT_SIGNED, low plain)
MRK_HD inline uint64_t order_map_i64(int64_t v, bool desc) {
  const uint64_t m = (uint64_t)v ^ 0x8000000000000000ull;
  return desc ? m : ~m;
}
MRK_HD inline int64_t order_unmap_i64(uint64_t mapped, bool desc) { return (int64_t)((desc ? mapped : ~mapped) ^ 0x8000000000000000ull); }

MRK_HD inline uint32_t order_unweight_part(uint32_t tie, uint32_t part) { return (tie == 2u ? ~part : part) ^ 0x80000000u; }
MRK_HD inline uint64_t order_lo(uint32_t tie, int32_t weight, uint32_t grow) {
  return tie ? ((uint64_t)sort_weight_part(tie, weight) << 32) | (uint32_t)~grow : ((uint64_t)(uint32_t)~grow << 32) | (uint32_t)weight;
}
MRK_HD inline int32_t order_lo_weight(uint32_t tie, uint64_t lo) { return (int32_t)(tie ? order_unweight_part(tie, (uint32_t)(lo >> 32)) : (uint32_t)lo); }
MRK_HD inline uint32_t order_lo_rowid(uint32_t tie, uint64_t lo) { return ~(tie ? (uint32_t)lo : (uint32_t)(lo >> 32)); }

// Pruning bin of a 64-bit mapped key.  Uniform bins over the raw 64 bits would put every row of one first value into one bin (the
// second part's 2^32 span per first value dwarfs its real range), so the key is compressed first: with the parts' least mapped keys
// a_lo / b_lo in the column and nb = the bits of the second part's range,
//   c = (a - a_lo) << nb  +  (b - b_lo)        bin = c >> shift, clamped to 1023
// monotone non-decreasing in the key as long as b stays inside its range.  A 64-bit attribute takes nb = 32 and a_lo : b_lo = the
// least key of the column: the sum, in wrapping 64-bit arithmetic, is then exactly key - least key.  Keys below the range (no row of
// the column the planner saw holds one) land in bin 0.
struct OrderGeom {
  uint32_t a_lo, b_lo, nb, shift;
};
MRK_HD inline uint32_t order_bin(const OrderGeom& g, uint64_t key) {
  const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
  if (a < g.a_lo || (a == g.a_lo && b < g.b_lo)) return 0u;
  const uint64_t c = (((uint64_t)(a - g.a_lo) << g.nb) + (uint64_t)b - (uint64_t)g.b_lo) >> g.shift;
  return c < 1023u ? (uint32_t)c : 1023u;
}
// the geometry from the parts' ranges of mapped keys (in the query's directions); a 64-bit attribute: a = high, b = low dwords of
// its least / largest key and i64 = true
MRK_HD inline OrderGeom order_geom(uint32_t a_lo, uint32_t a_hi, uint32_t b_lo, uint32_t b_hi, bool i64) {
  OrderGeom g{a_lo, b_lo, 32u, 0u};
  uint64_t top; // the largest compressed key
  if (i64)
    top = order_key(a_hi, b_hi) - order_key(a_lo, b_lo);
  else {
    g.nb = 0;
    while (g.nb < 32u && ((uint64_t)(b_hi - b_lo) >> g.nb) != 0u) ++g.nb;
    top = ((uint64_t)(a_hi - a_lo) << g.nb) + (b_hi - b_lo);
  }
  while (g.shift < 63u && (top >> g.shift) >= 1024u) ++g.shift;
  return g;
}

// ---------------------------------------------------------------------------------------
// The weight in FRONT of the parts (MRK_ORDER_WEIGHT_FIRST_*; SPH_KEYPART_WEIGHT as key part 0 of MatchGeneric2_fn / 3_fn): one
// layout for every shape of parts, wf = 1 weight DESC / 2 weight ASC (sort_weight_part's tie values; DevQuery::sort_tie holds it),
//   hi = the weight as wf orders it << 32 | d1
//   lo = d2 << 32 | ~global rowid
// d1 : d2 = the parts' 64-bit mapped key exactly as above -- map32(first) : map32(second), the second 0 for a single part of <= 32
// bits, both 0 without parts (weight ASC alone), the high : low dwords of an INT64's mapped key.  The true weight comes back out of
// the weight part through order_unweight_part.  The pruning bin is the WEIGHT's: the relevance bins (weight_bin above, which
// bin_of(BIN_WEIGHT, ..) of mrk_kprune.h is) for weight DESC, 1023 - that bin for weight ASC.
// ---------------------------------------------------------------------------------------
constexpr uint32_t SORT_WFIRST = 16;  // DevQuery::sort_flags of a query with sort_on == SORT_ON_WEIGHT (scan_pk_kernel tests this bit, as it does SORT_WIDE)
constexpr uint32_t SORT_ON_WEIGHT = 3; // DevQuery::sort_on
MRK_HD inline uint64_t wfirst_hi(uint32_t wf, int32_t weight, uint64_t parts_key) { return ((uint64_t)sort_weight_part(wf, weight) << 32) | (uint32_t)(parts_key >> 32); }
MRK_HD inline uint64_t wfirst_lo(uint64_t parts_key, uint32_t grow) { return (parts_key << 32) | (uint32_t)~grow; }
MRK_HD inline int32_t wfirst_weight(uint32_t wf, uint64_t hi) { return (int32_t)order_unweight_part(wf, (uint32_t)(hi >> 32)); }
MRK_HD inline uint32_t wfirst_rowid(uint64_t lo) { return ~(uint32_t)lo; }
MRK_HD inline uint64_t wfirst_parts_key(uint64_t hi, uint64_t lo) { return (hi << 32) | (lo >> 32); } // d1 : d2
// d1 : d2 of an attribute row; n_parts 0..2 (an INT64 counts as its two dwords).  Without parts the row is not read (it may not exist)
MRK_HD inline uint64_t wfirst_row_key(const uint32_t* row, uint32_t n_parts, const OrderPart& p0, const OrderPart& p1) {
  if (!n_parts) return 0ull;
  return order_key(order_map_part(sort_extract(row[p0.item], p0.shift, p0.bits), p0.flags), n_parts > 1u ? order_map_part(sort_extract(row[p1.item], p1.shift, p1.bits), p1.flags) : 0u);
}
// lo / shift: DevQuery::bin_lo / bin_shift as bins_by_weight (mrk_plan.cpp) sets them for the relevance order
MRK_HD inline uint32_t wfirst_bin(uint32_t wf, int32_t lo, uint32_t shift, int32_t weight) {
  const uint32_t b = weight_bin(lo, shift, weight);
  return wf == 2u ? 1023u - b : b;
}

// ---------------------------------------------------------------------------------------
// A candidate (hi, lo) under whichever of the three layouts above DevQuery::sort_on names (SORT_ON_ATTR: the sort's; SORT_ON_ORDER:
// the 64-bit order's; SORT_ON_WEIGHT: weight-first), tie = DevQuery::sort_tie: its pruning bin (lo / shift = DevQuery::bin_lo /
// bin_shift, g = ord_geom), the key it leaves the device with -- make_key(true weight, global rowid) -- and its 64-bit mapped key (a
// sort's 32 bits in the high dword; weight-first: the parts' key d1 : d2)
// ---------------------------------------------------------------------------------------
MRK_HD inline uint32_t cand_bin(uint32_t sort_on, uint32_t tie, int32_t lo, uint32_t shift, const OrderGeom& g, uint64_t hi) {
  return sort_on == SORT_ON_WEIGHT ? wfirst_bin(tie, lo, shift, wfirst_weight(tie, hi)) : sort_on == SORT_ON_ORDER ? order_bin(g, hi) : sort_bin((uint32_t)lo, shift, (uint32_t)(hi >> 32));
}
MRK_HD inline uint64_t cand_out_key(uint32_t sort_on, uint32_t tie, uint64_t hi, uint64_t lo) {
  return sort_on == SORT_ON_WEIGHT  ? make_key(wfirst_weight(tie, hi), wfirst_rowid(lo))
         : sort_on == SORT_ON_ORDER ? make_key(order_lo_weight(tie, lo), order_lo_rowid(tie, lo))
                                    : make_key((int32_t)(uint32_t)lo, ~(uint32_t)(lo >> 32));
}
MRK_HD inline uint64_t cand_mkey(uint32_t sort_on, uint64_t hi, uint64_t lo) {
  return sort_on == SORT_ON_WEIGHT ? wfirst_parts_key(hi, lo) : sort_on == SORT_ON_ORDER ? hi : hi & 0xFFFFFFFF00000000ull;
}

// ---------------------------------------------------------------------------------------
// The order spec word of an ORDER row (MRK_OROW_WORDS, include/mrk.h), whose entries carry a 64-bit mapped key: everything that
// decides whether two shards' mapped keys and tie rules compare and how a mapped key turns back into a raw value, and nothing of
// where a segment stores the columns.  0 = a relevance query.
//   bit 0 ordered | bit 1 wide (a 64-bit key; clear = a sort: the 32-bit mapped key in the high dword, the low dword zero) |
//   bit 2 INT64 (one signed 64-bit attribute) | bit 3 weight-first | bits 4-5 then_weight | part p in the 16 bits from bit 8 + 16 p:
//   bit 0 float | bit 1 desc | bit 2 signed (the high dword of an INT64) | bits 4-9 bit_count
// Weight-first (bit 3; MRK_ORDER_WEIGHT_FIRST_*): the weight leads the order and bits 4-5 hold ITS direction, 1 DESC / 2 ASC (0 and 3
// are no valid spec); every other field reads as without the bit -- one part of <= 32 bits (wide clear, the key in the high dword),
// two parts (wide), one INT64 (wide | INT64), or no part at all (weight ASC alone: both part fields zero, the mapped plane all zero).
// ---------------------------------------------------------------------------------------
constexpr uint64_t OSPEC_ORDERED = 1, OSPEC_WIDE = 2, OSPEC_INT64 = 4, OSPEC_WFIRST = 8;
constexpr uint32_t OSPEC_PART_FLOAT = 1, OSPEC_PART_DESC = 2, OSPEC_PART_SIGNED = 4;
MRK_HD inline uint64_t order_spec_part(uint32_t flags, uint32_t bits) {
  return ((flags & SORT_FLOAT) ? OSPEC_PART_FLOAT : 0u) | ((flags & SORT_DESC) ? OSPEC_PART_DESC : 0u) | ((flags & SORT_SIGNED) ? OSPEC_PART_SIGNED : 0u) | ((uint64_t)(bits & 63u) << 4);
}
// from a DevQuery's own words: sort_on (SORT_ON_ATTR / SORT_ON_ORDER), the first part's sort_flags / sort_bits, the second's ord_flags /
// ord_bits (read for SORT_ON_ORDER only), sort_tie
MRK_HD inline uint64_t order_spec_word(uint32_t sort_on, uint32_t flags0, uint32_t bits0, uint32_t flags1, uint32_t bits1, uint32_t tie) {
  if (!sort_on) return 0ull;
  uint64_t w = OSPEC_ORDERED | ((uint64_t)(tie & 3u) << 4) | (order_spec_part(flags0, bits0) << 8);
  if (sort_on == SORT_ON_ORDER) w |= OSPEC_WIDE | ((flags0 & SORT_SIGNED) ? OSPEC_INT64 : 0u) | (order_spec_part(flags1, bits1) << 24);
  return w;
}
// from a weight-first DevQuery's words (sort_on == SORT_ON_WEIGHT): sort_flags / sort_bits of the first dword behind the weight, ord_flags /
// ord_bits of the second, sort_tie = the weight's direction, wf_parts = 0..2 dwords (an INT64 counts as its two; part 0 is SORT_SIGNED then)
MRK_HD inline uint64_t order_spec_word_wfirst(uint32_t flags0, uint32_t bits0, uint32_t flags1, uint32_t bits1, uint32_t wf, uint32_t wf_parts) {
  uint64_t w = OSPEC_ORDERED | OSPEC_WFIRST | ((uint64_t)(wf & 3u) << 4);
  if (wf_parts) w |= order_spec_part(flags0, bits0) << 8;
  if (wf_parts > 1u) w |= OSPEC_WIDE | ((flags0 & SORT_SIGNED) ? OSPEC_INT64 : 0u) | (order_spec_part(flags1, bits1) << 24);
  return w;
}
// a weight-first spec word's direction of the weight is 1 or 2
MRK_HD inline bool order_spec_wfirst_valid(uint64_t spec) { const uint32_t d = (uint32_t)(spec >> 4) & 3u; return d == 1u || d == 2u; }
MRK_HD inline uint32_t order_spec_tie(uint64_t spec) { return spec ? (uint32_t)(spec >> 4) & 3u : 1u; } // relevance = weight desc
// part p's SORT_FLOAT | SORT_DESC | SORT_SIGNED out of a spec word
MRK_HD inline uint32_t order_spec_flags(uint64_t spec, uint32_t p) {
  const uint32_t f = (uint32_t)(spec >> (8u + 16u * p));
  return ((f & OSPEC_PART_FLOAT) ? SORT_FLOAT : 0u) | ((f & OSPEC_PART_DESC) ? SORT_DESC : 0u) | ((f & OSPEC_PART_SIGNED) ? SORT_SIGNED : 0u);
}
// the inverse of the 64-bit map under a spec word, in mrk_result.order_key's format: the raw int64, or raw0 << 32 | raw1 (a sort
// spec: raw0 << 32); a float's -0.0 reads +0.0.  A weight-first spec unmaps its parts as the same spec without bit 3 does; one
// without parts (part 0's bit count 0) unmaps to 0
MRK_HD inline uint64_t order_unmap_key(uint64_t spec, uint64_t mapped) {
  if (!spec) return 0ull;
  if ((spec & OSPEC_WFIRST) && !((spec >> 12) & 63u)) return 0ull;
  const uint32_t r0 = order_unmap_part((uint32_t)(mapped >> 32), order_spec_flags(spec, 0));
  if (!(spec & OSPEC_WIDE)) return (uint64_t)r0 << 32;
  return ((uint64_t)r0 << 32) | order_unmap_part((uint32_t)mapped, order_spec_flags(spec, 1));
}

#undef MRK_HD
} // namespace mrk
