// mrk_krows.h -- the three exchange-row formats (include/mrk.h: MRK_ROW_WORDS, MRK_SROW_WORDS, MRK_OROW_WORDS) as the kernels see
// them: what differs between them, and the one writer of a row.  Every row starts alike,
//   KCAP keys, zero past the count | count | total_found or a flag of ROW_FLAG_MASK
// a wide and an order row go on with a plane of KCAP mapped keys (zero past the count; all zero for a relevance query) and the
// query's spec word (mrk_sortkey.h; 0 = a relevance query).  pack_xrows_kernel, merge_xrows_kernel, sort_select_kernel
// (mrk_sortsel.hip) and sel_sort_kernel (mrk_select.hip) write rows through what is here.
#pragma once
#include "mrk_kcommon.h"

namespace mrk {

// how a merge elects the query's spec word out of its lists' (merge_xrows_kernel)
enum SpecElection {
  SPEC_NONE,         // the format has no spec word
  SPEC_OF_LIST0,     // list 0's; every list, a declined one included, must agree with it
  SPEC_OF_ANSWERING, // that of the first list not marked MRK_ROW_DECLINED; the other such lists must agree, a declined list has no say
};

// A format: KIND, its RowKind (the bit of a query's decline mask that pack_xrows_kernel tests); WORDS per row; MK, an entry of the mapped-key plane, MK_BYTES of it per entry in a row and in the merge's LDS (0: no plane);
// the word offsets MKEYS and SPEC; ELECT; WIDE_KEYS: the plane holds a whole 64-bit mapped key (else its high dword); spec_tie of a
// spec word; spec_of a query; mkey_of a 64-bit mapped key; load_mkey / store_plane of a row.
struct NarrowFmt {
  static constexpr RowKind KIND = ROWS_NARROW;
  static constexpr int WORDS = ROW_WORDS, MKEYS = 0, SPEC = 0, MK_BYTES = 0;
  static constexpr SpecElection ELECT = SPEC_NONE;
  static constexpr bool WIDE_KEYS = false;
  using MK = uint32_t; // (never read: every query merges as a relevance query)
  static __device__ __forceinline__ uint32_t spec_tie(uint64_t) { return 1u; }
  static __device__ __forceinline__ uint64_t spec_of(const DevQuery&) { return 0ull; }
  static __device__ __forceinline__ MK mkey_of(uint64_t) { return 0u; }
  static __device__ __forceinline__ MK load_mkey(const uint64_t*, uint32_t) { return 0u; }
  template <class F>
  static __device__ __forceinline__ void store_plane(uint64_t*, uint32_t, F) {}
};

struct WideFmt {
  static constexpr RowKind KIND = ROWS_WIDE;
  static constexpr int WORDS = SROW_WORDS, MKEYS = SROW_MKEYS, SPEC = SROW_SPEC, MK_BYTES = 4;
  static constexpr SpecElection ELECT = SPEC_OF_LIST0;
  static constexpr bool WIDE_KEYS = false;
  using MK = uint32_t;
  static __device__ __forceinline__ uint32_t spec_tie(uint64_t spec) { return sort_spec_tie(spec); }
  static __device__ __forceinline__ uint64_t spec_of(const DevQuery& Q) { return sort_spec_word(Q.sort_flags, Q.sort_tie, Q.sort_bits); }
  static __device__ __forceinline__ MK mkey_of(uint64_t mkey64) { return (uint32_t)(mkey64 >> 32); }
  static __device__ __forceinline__ MK load_mkey(const uint64_t* row, uint32_t i) { return reinterpret_cast<const uint32_t*>(row + MKEYS)[i]; }
  template <class F>
  static __device__ __forceinline__ void store_plane(uint64_t* __restrict__ row, uint32_t n, F mkey_at) { // two entries per word
    for (uint32_t i = threadIdx.x; i < (uint32_t)KCAP / 2; i += WG) {
      const uint64_t m0 = 2 * i < n ? mkey_at(2 * i) : 0u, m1 = 2 * i + 1 < n ? mkey_at(2 * i + 1) : 0u;
      row[MKEYS + i] = m0 | (m1 << 32);
    }
  }
};

struct OrderFmt {
  static constexpr RowKind KIND = ROWS_ORDER;
  static constexpr int WORDS = OROW_WORDS, MKEYS = OROW_MKEYS, SPEC = OROW_SPEC, MK_BYTES = 8;
  static constexpr SpecElection ELECT = SPEC_OF_ANSWERING;
  static constexpr bool WIDE_KEYS = true;
  using MK = uint64_t;
  static __device__ __forceinline__ uint32_t spec_tie(uint64_t spec) { return order_spec_tie(spec); }
  static __device__ __forceinline__ uint64_t spec_of(const DevQuery& Q) {
    if (Q.sort_on == SORT_ON_WEIGHT) return order_spec_word_wfirst(Q.sort_flags, Q.sort_bits, Q.ord_flags, Q.ord_bits, Q.sort_tie, Q.wf_parts);
    return order_spec_word(Q.sort_on, Q.sort_flags, Q.sort_bits, Q.ord_flags, Q.ord_bits, Q.sort_tie);
  }
  static __device__ __forceinline__ MK mkey_of(uint64_t mkey64) { return mkey64; }
  static __device__ __forceinline__ MK load_mkey(const uint64_t* row, uint32_t i) { return row[MKEYS + i]; }
  template <class F>
  static __device__ __forceinline__ void store_plane(uint64_t* __restrict__ row, uint32_t n, F mkey_at) {
    for (uint32_t i = threadIdx.x; i < (uint32_t)KCAP; i += WG) row[MKEYS + i] = i < n ? mkey_at(i) : 0ull;
  }
};

// ---- the row writer.  By the whole workgroup: the keys key_at(0 .. n) zero-padded to KCAP (Fmt::store_plane is its like for the plane)
template <class F>
__device__ __forceinline__ void write_row_keys(uint64_t* __restrict__ row, uint32_t n, F key_at) {
  for (uint32_t i = threadIdx.x; i < (uint32_t)KCAP; i += WG) row[i] = i < n ? key_at(i) : 0ull;
}
// By one thread: the count, the total_found word and, where the format has one, the spec word
template <class Fmt>
__device__ __forceinline__ void write_row_header(uint64_t* __restrict__ row, uint32_t n, uint64_t total_word, uint64_t spec) {
  row[KCAP] = n;
  row[KCAP + 1] = total_word;
  if (Fmt::ELECT != SPEC_NONE) row[Fmt::SPEC] = spec;
}
// The total_found word of a row that leaves a batch.  A query whose candidate list overflowed (QF_OVERFLOW) has no trustworthy list
// on the device until the host reran it: its row goes out empty with ROW_RERUN.  A query this shard declined (MRK_E_UNSUPPORTED) goes
// out empty with ROW_DECLINED: at submit by the planner (`declined`), or while it ran (QF_FSM, QF_ARENA: no rerun would help, and
// mrk_batch_wait reports MRK_E_UNSUPPORTED for it).  The merge ORs both bits through: the receiver reruns / fails the query, never a
// partial answer.  A row leaves with its keys only when row_unflagged(): the kernels' one test for that.
// (The fourth format, the GROUP row of mrk_groupsel.hip, has a header and a writer of its own and shares only what follows.)
constexpr uint32_t QF_DECLINES = QF_FSM | QF_ARENA | QF_GROUPS;
__device__ __forceinline__ bool row_unflagged(bool declined, uint32_t qflags) { return !declined && !(qflags & (QF_OVERFLOW | QF_DECLINES)); }
__device__ __forceinline__ uint64_t row_total_word(bool declined, uint32_t qflags, uint64_t total) {
  return declined || (qflags & QF_DECLINES) ? ROW_DECLINED : (qflags & QF_OVERFLOW) ? ROW_RERUN : (total & ~ROW_FLAG_MASK);
}

} // namespace mrk
