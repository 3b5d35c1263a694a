// mrk_kgroup.h -- GROUP BY one integer row attribute, or one 32-bit multi-value attribute (a group per value: blob_mva_span and
// group_flush_wave_mva below): the per-query group table and its update.
//
// Stands in for CSphKBufferGroupSorter (sphinxsort.cpp:2961-3310) while it has not cut: PushEx (:3148-3205) finds the match's group
// in a hash of group keys; a new group gets the match as its head and a count of 1 (++m_iTotal), an existing one
// (PushIntoExistingGroup, :3112-3145) a count + 1 and the match as its new head when it beats the old one under the within-group
// order -- MatchRelevanceLt_fn: weight DESC, rowid ASC, i.e. the larger make_key(weight, global rowid).  Up to max_matches *
// GROUPBY_FACTOR (:2767) groups none of this depends on the order the matches arrive in, so a group here is one slot claim, one
// 32-bit add and one 64-bit max; beyond that limit the reference starts CutWorst (:3176) and the device declines the query.
//
// Table of S slots (a power of two >= 2 * (4 K + 1), so that a query inside the limit never fills it), in the batch's arena of
// u64 words at DevQuery::grp_off:   [0] claimed slots (low dword)   [1 .. S] tag | group value   [S+1 .. 2S] head key
// [2S+1 ..] S counts (u32).  An empty slot's key word is 0; a claimed one holds GRP_TAG | value, so values 0 and 0xFFFFFFFF are
// ordinary keys.  Linear probing from group_hash(value); nothing is ever removed.
//
// Aggregates (mrk_aggrs, include/mrk.h: SUM / MIN / MAX of an integer row attribute, m_dAggregates, sphinxsort.cpp:2608-2693 with
// AggrSum_t / AggrMin_t / AggrMax_t, :1902-1979): a table with n_aggr of them has n_aggr planes of S u64 accumulators BEHIND the
// counts, [2S+1+S/2 + a S ..], so whoever reads the first three planes reads them where they were.  Every accumulator is an ADD or an
// UNSIGNED MAX over a word that starts at zero -- the arena's one memset stays the table's only initialisation: SUM adds the value
// (a DWORD sum is the low dword of the 64-bit one: it wraps modulo 2^32 as AggrSum_t<DWORD> does, :2623), MAX takes the value, MIN
// the value's complement, and a signed (INT64) value has its top bit flipped first (aggr_map).  A group's slot sees at least one
// update of every accumulator, so zero is a safe identity; group_select_kernel undoes the mapping (aggr_unmap).
// Where the flush gets the values: it READS THE ROWS AGAIN.  A buffered match's key holds its global rowid, and rowid - rowid_base is
// the row, so group_flush_wave_aggr needs no LDS beyond the two buffers (cbuf2's spare upper half could carry one 32-bit value, not
// four of 64), and the rows are in cache: the scan read the group attribute from them when it buffered the match.
//
// The probe, the claim and the hash are written over an "atomic ops" policy: GroupDevOps on the device (relaxed, agent scope --
// nothing reads the table before the selection launch), GroupSeqOps sequentially on the host (tests/cpp/group_table.cpp).
#pragma once
#include <stdint.h>

#include "../../include/mrk.h"
#include "mrk_sortkey.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRK_GHD __host__ __device__ inline
#else
#define MRK_GHD inline
#endif

namespace mrk {

constexpr uint32_t GROUPBY_FACTOR = 4; // sphinxsort.cpp:2767
constexpr uint64_t GRP_TAG = 1ull << 63;
constexpr uint32_t GRP_MAX_GROUPS = GROUPBY_FACTOR * MRK_MAX_K; // what group_select_kernel sorts in LDS

MRK_GHD uint32_t group_limit(uint32_t k) { return GROUPBY_FACTOR * k; }
MRK_GHD uint32_t group_slots_for(uint32_t k) {
  const uint32_t need = 2u * (group_limit(k) + 1u);
  uint32_t s = 8;
  while (s < need) s <<= 1;
  return s;
}
MRK_GHD uint64_t group_table_words(uint32_t slots, uint32_t n_aggr = 0) { return 1ull + 2ull * slots + slots / 2u + (uint64_t)n_aggr * slots; }

struct GroupTable {
  uint32_t* claimed;
  uint64_t* keys;
  uint64_t* heads;
  uint32_t* counts;
  uint32_t slots;
  uint64_t* aggr; // accumulator a of slot i: aggr[a * slots + i] (there for a table sized with n_aggr > a only)
};
MRK_GHD GroupTable group_table_at(uint64_t* base, uint32_t slots) {
  return GroupTable{reinterpret_cast<uint32_t*>(base), base + 1, base + 1 + slots, reinterpret_cast<uint32_t*>(base + 1 + 2ull * slots), slots, base + 1 + 2ull * slots + slots / 2u};
}

// An aggregate's op word (DevQuery::grp_aggr_op): bits 0-4 shift | bits 5-10 bit_count | bits 11-12 func (MRK_AGGR_*) |
// bit 13 the source is an aligned signed 64 (dwords item, item + 1) | bit 14 an INT source widened to 64 bits
constexpr uint32_t AGGR_SRC64 = 1u << 13, AGGR_WIDEN = 1u << 14;
constexpr uint64_t AGGR_SIGN = 1ull << 63;
MRK_GHD uint32_t aggr_op_word(uint32_t func, uint32_t shift, uint32_t bits, bool src64, bool widen) {
  return (shift & 31u) | ((bits & 63u) << 5) | ((func & 3u) << 11) | (src64 ? AGGR_SRC64 : 0u) | (widen ? AGGR_WIDEN : 0u);
}
MRK_GHD uint32_t aggr_func(uint32_t op) { return (op >> 11) & 3u; }
MRK_GHD bool aggr_is_add(uint32_t op) { return aggr_func(op) == (uint32_t)MRK_AGGR_SUM; }
MRK_GHD bool aggr_result64(uint32_t op) { return (op & (AGGR_SRC64 | AGGR_WIDEN)) != 0u; }
// the source's value in a row: the locator's raw bits zero-extended, or the 64's bits
MRK_GHD uint64_t aggr_source(const uint32_t* row, uint32_t item, uint32_t op) {
  return (op & AGGR_SRC64) ? ((uint64_t)row[item + 1u] << 32) | row[item] : (uint64_t)sort_extract(row[item], op & 31u, (op >> 5) & 63u);
}
// what goes into the accumulator (an add for SUM, an unsigned max for MIN / MAX) ...
MRK_GHD uint64_t aggr_map(uint32_t op, uint64_t v) {
  const uint32_t f = aggr_func(op);
  if (f == (uint32_t)MRK_AGGR_SUM) return v;
  const uint64_t x = (op & AGGR_SRC64) ? v ^ AGGR_SIGN : v;
  return f == (uint32_t)MRK_AGGR_MAX ? x : ~x;
}
// ... and the aggregate's value from it: a 32-bit result zero-extended, a 64-bit one the integer's bits
MRK_GHD uint64_t aggr_unmap(uint32_t op, uint64_t acc) {
  const uint32_t f = aggr_func(op);
  uint64_t x = f == (uint32_t)MRK_AGGR_MIN ? ~acc : acc;
  if (f != (uint32_t)MRK_AGGR_SUM && (op & AGGR_SRC64)) x ^= AGGR_SIGN;
  return aggr_result64(op) ? x : (uint64_t)(uint32_t)x;
}

MRK_GHD uint32_t group_hash(uint32_t value, uint32_t slots) {
  uint32_t h = value * 0x9E3779B1u;
  h ^= h >> 15;
  return h & (slots - 1u);
}

struct GroupSeqOps {
  static uint64_t load64(const uint64_t* p) { return *p; }
  static uint64_t cas64(uint64_t* p, uint64_t expected, uint64_t desired) {
    const uint64_t old = *p;
    if (old == expected) *p = desired;
    return old;
  }
  static void add32(uint32_t* p, uint32_t v) { *p += v; }
  static void add64(uint64_t* p, uint64_t v) { *p += v; }
  static void max64(uint64_t* p, uint64_t v) {
    if (v > *p) *p = v;
  }
};

// `count` matches of group `value`, the best of them `head`.  false: neither the value nor an empty slot within `slots` probes --
// the table is full of other groups, the query is past its limit (the caller sets QF_GROUPS) and the matches are dropped.
// A slot is counted (claimed) by the one caller that won its compare-and-swap, so the counter is the number of distinct values in
// the table whatever races the claims ran.
template <class Ops>
MRK_GHD bool group_update(const GroupTable& T, uint32_t value, uint32_t count, uint64_t head) {
  const uint64_t word = GRP_TAG | value;
  uint32_t i = group_hash(value, T.slots);
  for (uint32_t step = 0; step < T.slots; ++step, i = (i + 1u) & (T.slots - 1u)) {
    uint64_t cur = Ops::load64(T.keys + i);
    if (cur == 0ull) {
      cur = Ops::cas64(T.keys + i, 0ull, word);
      if (cur == 0ull) {
        Ops::add32(T.claimed, 1u);
        cur = word;
      }
    }
    if (cur == word) {
      Ops::add32(T.counts + i, count);
      Ops::max64(T.heads + i, head);
      return true;
    }
  }
  return false;
}

// group_update that also tells the slot (0xFFFFFFFF: the table is full), for the callers that go on to the slot's accumulators ...
template <class Ops>
MRK_GHD uint32_t group_update_slot(const GroupTable& T, uint32_t value, uint32_t count, uint64_t head) {
  const uint64_t word = GRP_TAG | value;
  uint32_t i = group_hash(value, T.slots);
  for (uint32_t step = 0; step < T.slots; ++step, i = (i + 1u) & (T.slots - 1u)) {
    uint64_t cur = Ops::load64(T.keys + i);
    if (cur == 0ull) {
      cur = Ops::cas64(T.keys + i, 0ull, word);
      if (cur == 0ull) {
        Ops::add32(T.claimed, 1u);
        cur = word;
      }
    }
    if (cur == word) {
      Ops::add32(T.counts + i, count);
      Ops::max64(T.heads + i, head);
      return i;
    }
  }
  return 0xFFFFFFFFu;
}
// ... one accumulator's update with a MAPPED value (aggr_map), or with the sum / the maximum of several
template <class Ops>
MRK_GHD void group_aggr_update(const GroupTable& T, uint32_t slot, uint32_t a, uint32_t op, uint64_t mapped) {
  uint64_t* p = T.aggr + (uint64_t)a * T.slots + slot;
  if (aggr_is_add(op))
    Ops::add64(p, mapped);
  else
    Ops::max64(p, mapped);
}
// ... and the whole: `count` matches of group `value` whose aggregates' mapped values combine to mapped[0 .. n_aggr)
template <class Ops>
MRK_GHD bool group_update(const GroupTable& T, uint32_t value, uint32_t count, uint64_t head, uint32_t n_aggr, const uint32_t* ops, const uint64_t* mapped) {
  const uint32_t slot = group_update_slot<Ops>(T, value, count, head);
  if (slot == 0xFFFFFFFFu) return false;
  for (uint32_t a = 0; a < n_aggr; ++a) group_aggr_update<Ops>(T, slot, a, ops[a], mapped[a]);
  return true;
}

// ---- GROUP BY a multi-value attribute (mrk_group_mva, include/mrk.h; MVAGroupSorter_T::Push, sphinxsort.cpp:4113-4156): a match is
// pushed once per STORED value of its MVA, in the stored order and with every duplicate.  The MVA word (DevQuery::grp_pad) is coded as
// DevFilter::mva is: width in bits | blob attribute id << 16 | blob attributes of the row << 24.
// blob_mva_span: where the values of a row's MVA lie in the pool, with row_passes_filters' arithmetic (mrk_dev.h; the blob row of
// attribute.cpp:495-513: length-size byte, n_blob cumulative lengths, data).  Every blob row was bounds-checked at load
// (mrk_blobrow.h), so nothing here is checked again.  The data is not aligned: the header and the values are read byte-wise.
struct MvaSpan {
  const uint8_t* data;
  uint32_t n; // values of the MVA's width
};
MRK_GHD uint32_t group_mva_word(uint32_t bits, uint32_t blob_attr_id, uint32_t n_blob_attrs) { return (bits & 0xffu) | ((blob_attr_id & 0xffu) << 16) | (n_blob_attrs << 24); }
MRK_GHD uint64_t blob_read_le(const uint8_t* p, uint32_t nb) {
  uint64_t x = 0;
  for (uint32_t i = 0; i < nb; ++i) x |= (uint64_t)p[i] << (8u * i);
  return x;
}
MRK_GHD MvaSpan blob_mva_span(const uint8_t* blobs, const uint32_t* row, uint32_t mva) {
  const uint32_t w = (mva & 0xffu) >> 3, id = (mva >> 16) & 0xffu, nblob = mva >> 24;
  const uint8_t* br = blobs + ((uint64_t)row[2] | ((uint64_t)row[3] << 32)); // sphGetBlobRowOffset: the 2nd attribute
  const uint32_t sz = br[0] == 0 ? 1u : br[0] == 1 ? 2u : 4u;
  const uint64_t l1 = blob_read_le(br + 1 + id * sz, sz), l0 = id ? blob_read_le(br + 1 + (id - 1u) * sz, sz) : 0ull;
  return MvaSpan{br + 1 + (uint64_t)nblob * sz + l0, w ? (uint32_t)((l1 - l0) / w) : 0u};
}
MRK_GHD uint32_t blob_mva_value32(const MvaSpan& s, uint32_t i) { return (uint32_t)blob_read_le(s.data + 4ull * i, 4u); }

// The groups' order (MatchGeneric1_fn, sphinxsort.cpp:4708-4720): one of group value / count / head weight, ascending or
// descending, then the head's global rowid ascending.  Larger = better.  Heads of a row attribute's groups are distinct rows, so no
// two of them tie; one doc may head several groups of a multi-value attribute, and groups whose keys are equal leave with the
// smaller group value first (group_sort_desc, mrk_groupsel.hip; include/mrk.h has the why).
MRK_GHD uint64_t group_order_key(uint32_t sort_by, uint32_t desc, uint32_t value, uint32_t count, uint64_t head) {
  const uint32_t p = sort_by == MRK_GROUPSORT_COUNT ? count : sort_by == MRK_GROUPSORT_KEY ? value : (uint32_t)(head >> 32);
  return ((uint64_t)(desc ? p : ~p) << 32) | (uint32_t)head;
}
// ... or an aggregate's 32-bit value (mrk_aggrs::order_by), exactly as @count is taken
MRK_GHD uint64_t group_order_key_aggr(uint32_t desc, uint32_t aggr_value, uint64_t head) { return ((uint64_t)(desc ? aggr_value : ~aggr_value) << 32) | (uint32_t)head; }

// The group spec word of a GROUP row (MRK_GROW_WORDS, include/mrk.h): what every merger of a grouped query's rows must agree on --
// the groups' order, the key's width and the query's max_matches (the 4 k limit and the first k) -- and nothing of where a segment
// stores the column.  0 = a relevance query.
//   bit 0 grouped | bits 1-2 sort_by | bit 3 desc | bits 8-13 bit_count | bits 16-26 max_matches
struct GroupSpec {
  uint32_t sort_by, desc, bit_count, k;
};
MRK_GHD uint64_t group_spec_word(uint32_t sort_by, uint32_t desc, uint32_t bit_count, uint32_t k) {
  return 1ull | ((uint64_t)(sort_by & 3u) << 1) | ((uint64_t)(desc & 1u) << 3) | ((uint64_t)(bit_count & 63u) << 8) | ((uint64_t)(k & 2047u) << 16);
}
// false: not a word group_spec_word writes for a query this library answers (a stray bit, an unknown order, a width or a max_matches
// out of range); the merge reads such a list as declined
MRK_GHD bool group_spec_unpack(uint64_t w, GroupSpec& s) {
  s.sort_by = (uint32_t)(w >> 1) & 3u, s.desc = (uint32_t)(w >> 3) & 1u, s.bit_count = (uint32_t)(w >> 8) & 63u, s.k = (uint32_t)(w >> 16) & 2047u;
  return (w & 1ull) && w == group_spec_word(s.sort_by, s.desc, s.bit_count, s.k) && s.sort_by <= (uint32_t)MRK_GROUPSORT_WEIGHT && s.bit_count >= 1u &&
         s.bit_count <= 32u && s.k >= 1u && s.k <= (uint32_t)MRK_MAX_K;
}
// A group row's word offsets; an entry of its plane (the group value over its count); and its reader -- the one every merger goes
// through, on the device and in tests/cpp/group_merge.cpp: the entry count, the total word and the spec word of a list's row.  A
// hostile row (more entries than a row holds, a spec word that does not unpack) reads as MRK_ROW_DECLINED with no entries and spec
// word 0, so nothing behind it indexes past the row.  group_row_has_say: whether the list takes part in the election of the query's
// spec word -- every list but a declined one without a spec (a shard whose planner declined the query sends 0).  A list declined
// under its spec word (over the limit while it ran, or the merged row of such lists) keeps its say, so that a staged merge elects
// the spec a one-step merge elects.
constexpr int GROW_GROUPS = MRK_GROW_GROUPS, GROW_WORDS = MRK_GROW_WORDS;
constexpr int GROW_CNT = GROW_GROUPS, GROW_TOTAL = GROW_GROUPS + 1, GROW_PLANE = GROW_GROUPS + 2, GROW_SPEC = GROW_WORDS - 1;
MRK_GHD uint64_t group_plane_word(uint32_t value, uint32_t count) { return ((uint64_t)value << 32) | count; }
MRK_GHD uint32_t group_row_head(const uint64_t* row, uint64_t& tword, uint64_t& spec) {
  const uint64_t c = row[GROW_CNT], t = row[GROW_TOTAL], sp = row[GROW_SPEC];
  GroupSpec gs;
  const bool hostile = c > (uint64_t)GROW_GROUPS || (sp != 0ull && !group_spec_unpack(sp, gs));
  tword = hostile ? (t & MRK_ROW_RERUN) | MRK_ROW_DECLINED : t;
  spec = hostile ? 0ull : sp;
  return hostile ? 0u : (uint32_t)c;
}
MRK_GHD bool group_row_has_say(uint64_t tword, uint64_t spec) { return !(tword & MRK_ROW_DECLINED) || spec != 0ull; }

// The AGGREGATE row (MRK_AROW_WORDS, include/mrk.h): a GROUP row's first 2 G + 2 words, then MRK_MAX_AGGRS planes of G aggregate
// VALUES (what aggr_unmap gives: the accumulators' mapping does not travel), the group spec word and the aggregate spec word --
// what every merger of the query's aggregates must agree on and nothing of where a segment stores the column.  0 = no aggregates.
//   bit 0 set | bits 1-3 n | bits 4-6 1 + the ordering aggregate (0 = none) | per aggregate a, bits 8 + 4 a ..: func (2 bits) |
//   the source is a signed 64 | an INT source widened
constexpr int AROW_WORDS = MRK_AROW_WORDS;
constexpr int AROW_AGGR = GROW_PLANE + GROW_GROUPS, AROW_GSPEC = AROW_WORDS - 2, AROW_ASPEC = AROW_WORDS - 1; // (plane a: AROW_AGGR + a * GROW_GROUPS)
struct AggrSpec {
  uint32_t n, order; // order: 1 + the aggregate whose merged 32-bit value orders the groups, 0 = the group spec's sort_by does
};
MRK_GHD uint32_t aggr_spec_nibble(uint32_t op) { return aggr_func(op) | ((op & AGGR_SRC64) ? 4u : 0u) | ((op & AGGR_WIDEN) ? 8u : 0u); }
// aggregate a's op word from its nibble, shift and bits 0: all that aggr_map / aggr_unmap / group_aggr_update read of it
MRK_GHD uint32_t aggr_spec_op(uint64_t w, uint32_t a) {
  const uint32_t nib = (uint32_t)(w >> (8u + 4u * a)) & 15u;
  return aggr_op_word(nib & 3u, 0u, 0u, (nib & 4u) != 0u, (nib & 8u) != 0u);
}
MRK_GHD uint64_t aggr_spec_word(uint32_t n, uint32_t order, const uint32_t* ops) {
  uint64_t w = 1ull | ((uint64_t)(n & 7u) << 1) | ((uint64_t)(order & 7u) << 4);
  for (uint32_t a = 0; a < n && a < (uint32_t)MRK_MAX_AGGRS; ++a) w |= (uint64_t)aggr_spec_nibble(ops[a]) << (8u + 4u * a);
  return w;
}
// false: not a word aggr_spec_word writes for a query this library answers next to a group spec with this sort_by -- a stray bit, n out
// of range, func 0 inside n or a field beyond it, both width bits, an order that names a 64-bit result or no aggregate, an order next
// to another sort_by
MRK_GHD bool aggr_spec_unpack(uint64_t w, uint32_t group_sort_by, AggrSpec& s) {
  s.n = (uint32_t)(w >> 1) & 7u, s.order = (uint32_t)(w >> 4) & 7u;
  if (!(w & 1ull) || (w >> 24) != 0ull || (w & 0x80ull) || s.n < 1u || s.n > (uint32_t)MRK_MAX_AGGRS || s.order > s.n) return false;
  for (uint32_t a = 0; a < (uint32_t)MRK_MAX_AGGRS; ++a) {
    const uint32_t nib = (uint32_t)(w >> (8u + 4u * a)) & 15u;
    if (a < s.n ? (nib & 3u) == 0u || (nib & 12u) == 12u : nib != 0u) return false;
  }
  if (s.order && ((((uint32_t)(w >> (8u + 4u * (s.order - 1u))) & 12u) != 0u) || group_sort_by != (uint32_t)MRK_GROUPSORT_KEY)) return false;
  return true;
}
// The reader of an aggregate row, the only way into one for merge_arows_kernel and tests/cpp/aggr_merge.cpp: group_row_head's
// contract over both spec words.  Hostile -- more entries than a row holds, a group spec that does not unpack, an aggregate spec that
// does not unpack next to it or stands over group spec 0 -- reads as MRK_ROW_DECLINED with no entries and both spec words 0, so nothing
// behind it indexes by an unchecked field.  (group_row_has_say over the group spec word tells whether the list takes part in the election.)
MRK_GHD uint32_t aggr_row_head(const uint64_t* row, uint64_t& tword, uint64_t& gspec, uint64_t& aspec) {
  const uint64_t c = row[GROW_CNT], t = row[GROW_TOTAL], gsp = row[AROW_GSPEC], asp = row[AROW_ASPEC];
  GroupSpec gs;
  AggrSpec as;
  const bool hostile = c > (uint64_t)GROW_GROUPS || (gsp != 0ull && !group_spec_unpack(gsp, gs)) || (asp != 0ull && (gsp == 0ull || !aggr_spec_unpack(asp, gs.sort_by, as)));
  tword = hostile ? (t & MRK_ROW_RERUN) | MRK_ROW_DECLINED : t;
  gspec = hostile ? 0ull : gsp, aspec = hostile ? 0ull : asp;
  return hostile ? 0u : (uint32_t)c;
}

#if defined(__HIPCC__)
struct GroupDevOps {
  static __device__ uint64_t load64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ uint64_t cas64(uint64_t* p, uint64_t expected, uint64_t desired) {
    __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expected; // (the value found: `expected` itself when the exchange happened)
  }
  static __device__ void add32(uint32_t* p, uint32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ void add64(uint64_t* p, uint64_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ void max64(uint64_t* p, uint64_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t group_dpp_max64(uint64_t x) { // (keys are unsigned: the 0 a lane without a source reads is the identity)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, CTRL, ROW_MASK, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), CTRL, ROW_MASK, 0xf, false);
  const uint64_t y = ((uint64_t)hi << 32) | lo;
  return y > x ? y : x;
}
__device__ __forceinline__ uint64_t group_wave_max64(uint64_t v) {
  v = group_dpp_max64<0x111, 0xf>(v); // row_shr:1
  v = group_dpp_max64<0x112, 0xf>(v); // row_shr:2
  v = group_dpp_max64<0x114, 0xf>(v); // row_shr:4
  v = group_dpp_max64<0x118, 0xf>(v); // row_shr:8
  v = group_dpp_max64<0x142, 0xa>(v); // row_bcast:15 -> rows 1, 3
  v = group_dpp_max64<0x143, 0xc>(v); // row_bcast:31 -> rows 2, 3
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}

// A wave's buffered matches of ONE grouped query go to its table: cbuf[i] = make_key(weight, global rowid), cbuf2[i] = the group
// value, i < cn <= 128.  Equal values are combined first -- count = their number, head = their largest key -- and the distinct ones
// written back to the front of the two buffers (the lanes hold the entries in registers by then: no LDS beyond the buffers), so a
// column of four values costs four table updates per flush, not one same-address atomic per match.  Then one lane per distinct value
// runs group_update.  All 64 lanes call it; false (uniform) = some update found the table full.
__device__ __forceinline__ bool group_flush_wave(const GroupTable& T, uint64_t* cbuf, uint64_t* cbuf2, uint32_t cn, uint32_t lane) {
  const bool v0 = lane < cn, v1 = lane + 64u < cn;
  const uint64_t k0 = v0 ? cbuf[lane] : 0ull, k1 = v1 ? cbuf[lane + 64u] : 0ull;
  const uint32_t g0 = v0 ? (uint32_t)cbuf2[lane] : 0u, g1 = v1 ? (uint32_t)cbuf2[lane + 64u] : 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  uint64_t p0 = __ballot(v0), p1 = __ballot(v1);
  uint32_t nd = 0;
  while (p0 | p1) { // (uniform) one round per distinct value
    const uint32_t src = (uint32_t)__builtin_ctzll(p0 ? p0 : p1);
    const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)(p0 ? g0 : g1), (int)src);
    const bool m0 = v0 && g0 == v, m1 = v1 && g1 == v; // (entries of one value are pending together)
    const uint64_t b0 = __ballot(m0), b1 = __ballot(m1);
    const uint64_t a = m0 ? k0 : 0ull, b = m1 ? k1 : 0ull;
    const uint64_t h = group_wave_max64(a > b ? a : b);
    if (lane == 0) {
      cbuf[nd] = h;
      cbuf2[nd] = (uint64_t)v | ((uint64_t)(uint32_t)(__popcll(b0) + __popcll(b1)) << 32);
    }
    ++nd;
    p0 &= ~b0, p1 &= ~b1;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  bool ok = true;
  for (uint32_t j = lane; j < nd; j += 64u) {
    const uint64_t vc = cbuf2[j];
    ok = group_update<GroupDevOps>(T, (uint32_t)vc, (uint32_t)(vc >> 32), cbuf[j]) && ok;
  }
  const bool all_ok = __ballot(!ok) == 0ull;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return all_ok;
}

// ---- the flush of a query WITH aggregates.  A function of its own, chosen by a uniform branch on DevQuery::grp_naggr where the
// kernels publish, so that a grouped query without aggregates runs group_flush_wave as it stands -- and only in kernel INSTANCES of
// their own (the AGGR template flag of scan_pk_kernel / rank_kernel, launched for batches that hold a query with aggregates), so that
// the instances every other sorted or grouped batch launches report the registers they reported before (DESIGN section 4c'').
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t group_dpp_add64(uint64_t x) { // (a lane without a source reads 0)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, CTRL, ROW_MASK, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), CTRL, ROW_MASK, 0xf, false);
  return x + (((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t group_wave_add64(uint64_t v) { // (the ladder of group_wave_max64: lane 63 ends with the wave's sum, modulo 2^64)
  v = group_dpp_add64<0x111, 0xf>(v);
  v = group_dpp_add64<0x112, 0xf>(v);
  v = group_dpp_add64<0x114, 0xf>(v);
  v = group_dpp_add64<0x118, 0xf>(v);
  v = group_dpp_add64<0x142, 0xa>(v);
  v = group_dpp_add64<0x143, 0xc>(v);
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}

// group_flush_wave for a query with n_aggr aggregates (aggr_item / aggr_op: DevQuery::grp_aggr_item / grp_aggr_op).  Its three steps: the same combine per distinct value (count, head);
// one lane per distinct value claims or finds the slot and leaves it in cbuf2 (value | slot << 32); then, one aggregate at a time
// (two mapped values per lane, re-read from the rows attrs + (key_rowid(key) - rowid_base) * attr_stride: see the header), one round
// per distinct value reduces the aggregate across the wave -- a 64-bit add or max over the DPP ladder -- and lane 0 issues the
// slot's one atomic; a buffer of mostly distinct values (fewer than four entries to a value) skips the rounds and every entry updates
// its slot itself.  The locators are read from the descriptor here, on the rare branch.
__device__ __forceinline__ bool group_flush_wave_aggr(const GroupTable& T, uint64_t* cbuf, uint64_t* cbuf2, uint32_t cn, uint32_t lane, const uint32_t* __restrict__ attrs,
                                                      uint32_t attr_stride, uint32_t rowid_base, uint32_t n_aggr, const uint32_t* __restrict__ aggr_item, const uint32_t* __restrict__ aggr_op) {
  const bool v0 = lane < cn, v1 = lane + 64u < cn;
  const uint64_t k0 = v0 ? cbuf[lane] : 0ull, k1 = v1 ? cbuf[lane + 64u] : 0ull;
  const uint32_t g0 = v0 ? (uint32_t)cbuf2[lane] : 0u, g1 = v1 ? (uint32_t)cbuf2[lane + 64u] : 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  uint64_t p0 = __ballot(v0), p1 = __ballot(v1);
  uint32_t nd = 0, e0 = 0, e1 = 0; // (e0 / e1: which distinct value the lane's entries are)
  while (p0 | p1) { // (uniform) one round per distinct value
    const uint32_t src = (uint32_t)__builtin_ctzll(p0 ? p0 : p1);
    const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)(p0 ? g0 : g1), (int)src);
    const bool m0 = v0 && g0 == v, m1 = v1 && g1 == v;
    const uint64_t b0 = __ballot(m0), b1 = __ballot(m1);
    const uint64_t a = m0 ? k0 : 0ull, b = m1 ? k1 : 0ull;
    const uint64_t h = group_wave_max64(a > b ? a : b);
    if (lane == 0) {
      cbuf[nd] = h;
      cbuf2[nd] = (uint64_t)v | ((uint64_t)(uint32_t)(__popcll(b0) + __popcll(b1)) << 32);
    }
    e0 = m0 ? nd : e0, e1 = m1 ? nd : e1;
    ++nd;
    p0 &= ~b0, p1 &= ~b1;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  bool ok = true;
  for (uint32_t j = lane; j < nd; j += 64u) { // (nd <= cn <= 128: a lane's own entries only)
    const uint64_t vc = cbuf2[j];
    const uint32_t slot = group_update_slot<GroupDevOps>(T, (uint32_t)vc, (uint32_t)(vc >> 32), cbuf[j]);
    ok = ok && slot != 0xFFFFFFFFu;
    cbuf2[j] = (uint64_t)(uint32_t)vc | ((uint64_t)slot << 32);
  }
  const bool all_ok = __ballot(!ok) == 0ull;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const uint32_t* __restrict__ row0 = attrs + (uint64_t)(v0 ? key_rowid(k0) - rowid_base : 0u) * attr_stride;
  const uint32_t* __restrict__ row1 = attrs + (uint64_t)(v1 ? key_rowid(k1) - rowid_base : 0u) * attr_stride;
  // (uniform) mostly distinct values -- fewer than four entries to a value: a round per value would reduce next to nothing, so every
  // entry goes to its slot's accumulator itself (the few that share a slot meet in the atomic unit)
  const bool direct = nd * 4u > cn;
  const uint32_t s0 = direct && v0 ? (uint32_t)(cbuf2[e0] >> 32) : 0xFFFFFFFFu, s1 = direct && v1 ? (uint32_t)(cbuf2[e1] >> 32) : 0xFFFFFFFFu;
  for (uint32_t ai = 0; ai < n_aggr && ai < (uint32_t)MRK_MAX_AGGRS; ++ai) { // (uniform)
    const uint32_t item = aggr_item[ai], op = aggr_op[ai];
    const uint64_t x0 = v0 ? aggr_map(op, aggr_source(row0, item, op)) : 0ull, x1 = v1 ? aggr_map(op, aggr_source(row1, item, op)) : 0ull;
    uint64_t* __restrict__ plane = T.aggr + (uint64_t)ai * T.slots;
    const bool add = aggr_is_add(op);
    if (direct) {
      if (s0 != 0xFFFFFFFFu) {
        if (add)
          GroupDevOps::add64(plane + s0, x0);
        else
          GroupDevOps::max64(plane + s0, x0);
      }
      if (s1 != 0xFFFFFFFFu) {
        if (add)
          GroupDevOps::add64(plane + s1, x1);
        else
          GroupDevOps::max64(plane + s1, x1);
      }
      continue;
    }
    for (uint32_t j = 0; j < nd; ++j) { // (uniform) the entries of distinct value j
      const uint64_t vc = cbuf2[j]; // (one address: a broadcast read)
      const uint32_t v = (uint32_t)vc, slot = (uint32_t)(vc >> 32);
      const uint64_t a = v0 && g0 == v ? x0 : 0ull, b = v1 && g1 == v ? x1 : 0ull;
      const uint64_t r = add ? group_wave_add64(a + b) : group_wave_max64(a > b ? a : b);
      if (lane == 0 && slot != 0xFFFFFFFFu) {
        if (add)
          GroupDevOps::add64(plane + slot, r);
        else
          GroupDevOps::max64(plane + slot, r);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return all_ok;
}

// ---- the flush of a query grouped by a MULTI-VALUE attribute (the MVA word, DevQuery::grp_pad: see blob_mva_span).  Chosen by a
// uniform branch on that word where the kernels publish, in the AGGR instances only -- the flag means "the flush reads the rows
// again" -- so that every other instance stays as it is.  cbuf holds the matches' keys; what the scan buffered in cbuf2 is ignored.
// Steps: every lane takes the keys of its <= 2 entries into registers (from here on the two buffers are free: no key is read from
// LDS again, so nothing unread is ever overwritten) and finds their MVAs' spans in the pool, row = key_rowid(key) - rowid_base; a
// wave prefix sum of the value counts numbers the expanded (key, value) pairs, entries in buffer order and values in stored order;
// then, in rounds of up to 128 pairs, the lanes write their pairs of the round into the buffers and group_flush_wave takes the
// round to the table as it takes a row attribute's buffer -- equal values combined to one count and one head, one lane per distinct
// value in group_update, so a hot tag costs one atomic per round and not one per match.  A doc with more values than a round holds
// spreads over several rounds (the lane keeps key and span in registers); an entry without values writes nothing.  Offsets are 64-bit:
// 128 spans of one pool may add up to more than 2^32 values.  false (uniform) = some update found the table full.
__device__ __forceinline__ uint64_t group_wave_scan64(uint64_t v, uint64_t& total) { // inclusive prefix sum over the lanes; total = lane 63's
  v = group_dpp_add64<0x111, 0xf>(v);
  v = group_dpp_add64<0x112, 0xf>(v);
  v = group_dpp_add64<0x114, 0xf>(v);
  v = group_dpp_add64<0x118, 0xf>(v);
  v = group_dpp_add64<0x142, 0xa>(v);
  v = group_dpp_add64<0x143, 0xc>(v);
  total = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  return v;
}
constexpr uint32_t GRP_MVA_ROUND = 128; // pairs per round: what cbuf / cbuf2 hold (MRK_CBUF, RK_CBUF)

__device__ __forceinline__ bool group_flush_wave_mva(const GroupTable& T, uint64_t* cbuf, uint64_t* cbuf2, uint32_t cn, uint32_t lane, const uint32_t* __restrict__ attrs,
                                                     uint32_t attr_stride, uint32_t rowid_base, const uint8_t* __restrict__ blobs, uint32_t mva) {
  const bool v0 = lane < cn, v1 = lane + 64u < cn;
  const uint64_t k0 = v0 ? cbuf[lane] : 0ull, k1 = v1 ? cbuf[lane + 64u] : 0ull;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  MvaSpan s0{nullptr, 0u}, s1{nullptr, 0u};
  if (v0) s0 = blob_mva_span(blobs, attrs + (uint64_t)(key_rowid(k0) - rowid_base) * attr_stride, mva);
  if (v1) s1 = blob_mva_span(blobs, attrs + (uint64_t)(key_rowid(k1) - rowid_base) * attr_stride, mva);
  uint64_t t0, t1;
  const uint64_t o0 = group_wave_scan64(s0.n, t0) - s0.n;      // the lane's first entry: its first pair's number
  const uint64_t o1 = t0 + group_wave_scan64(s1.n, t1) - s1.n; // ... and its second entry's, behind all the first ones
  const uint64_t total = t0 + t1;
  bool ok = true;
  for (uint64_t base = 0; base < total; base += GRP_MVA_ROUND) { // (uniform)
    auto fill = [&](uint64_t o, const MvaSpan& s, uint64_t k) {  // the entry's pairs numbered [base, base + GRP_MVA_ROUND)
      const uint64_t lo = base > o ? base - o : 0ull;
      const uint64_t room = o >= base + GRP_MVA_ROUND ? 0ull : base + GRP_MVA_ROUND - o;
      const uint64_t hi = room < s.n ? room : s.n;
      for (uint64_t i = lo; i < hi; ++i) {
        const uint32_t at = (uint32_t)(o + i - base); // (< GRP_MVA_ROUND)
        cbuf[at] = k;
        cbuf2[at] = blob_mva_value32(s, (uint32_t)i);
      }
    };
    fill(o0, s0, k0);
    fill(o1, s1, k1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint64_t left = total - base;
    ok = group_flush_wave(T, cbuf, cbuf2, left < GRP_MVA_ROUND ? (uint32_t)left : GRP_MVA_ROUND, lane) && ok; // (ends behind a fence: the buffers are free again)
  }
  return ok;
}
#endif // __HIPCC__

} // namespace mrk
