// mrk_sortsel.hip -- exact top-K of the SORTED queries' candidate lists (mrk_query.sort: MatchAttrLt_fn / MatchAttrGt_fn /
// MatchGeneric1_fn / 2_fn over one row attribute, sphinxsort.cpp:4552-4730), gfx950 / wave64.
//
// A sorted query's candidates are 128 bits (mrk_sortkey.h): hi = mapped attribute key | weight as the tie rule orders it,
// lo = ~rowid | true weight; larger (hi, lo) = better, which is the sorter's whole order -- attribute, then the weight where
// the tie rule names it, then rowid ascending.  The scan pruned by the bin of the mapped key alone, so everything at or above
// the final threshold bin of the query's histogram is in the list.  One workgroup per query streams the list, keeps what
// reaches the threshold bin and the running K-th best in an LDS buffer of 2 K candidates, and sorts that buffer (bitonic, on
// the full 128 bits) whenever it fills up: exact however many rows share the K-th row's attribute value -- a column with four
// distinct values puts a quarter of the matches into one bin, and all of them are compared by weight and rowid here.
// A weight-first order (MRK_ORDER_WEIGHT_FIRST_*) takes the same walk with the weight-first layout: the bin is the weight's, out of
// hi's high dword, and the parts' mapped key -- hi's low dword : lo's high dword -- decides inside a weight class.
//
// Below it: the WIDE exchange rows that carry a sorted query across segments and shards (pack_srows_kernel) and their merge
// (merge_srows_kernel), then the ORDER rows that carry a 64-bit mapped key per entry (pack_orows_kernel, merge_orows_kernel).
#include "mrk_kcommon.h"
#include "mrk_kprune.h"
#include "mrk_sortkey.h"

#include <atomic>

namespace mrk {

struct __align__(16) SortSelSmem {
  uint64_t hi[CAND];
  uint64_t lo[CAND];
  uint32_t cand_n, tau_bin, have_tau, pad;
  uint64_t tau_hi, tau_lo;
};

__device__ __forceinline__ bool sortkey_gt(uint64_t ah, uint64_t al, uint64_t bh, uint64_t bl) { return ah > bh || (ah == bh && al > bl); }

// sort the buffer's first `len` (a power of two) entries descending; entries past cand_n are zero padding
static __device__ void sortsel_sort(SortSelSmem& s, uint32_t len) {
  for (uint32_t k = 2; k <= len; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < len / 2; t += WG) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const bool desc = (i & k) == 0;
        const uint64_t ah = s.hi[i], al = s.lo[i], bh = s.hi[p], bl = s.lo[p];
        if (sortkey_gt(bh, bl, ah, al) == desc) s.hi[i] = bh, s.lo[i] = bl, s.hi[p] = ah, s.lo[p] = al;
      }
      __syncthreads();
    }
}

// keep the best K of the buffer, sorted; the K-th becomes the running threshold
static __device__ uint32_t sortsel_compact(SortSelSmem& s, uint32_t K) {
  __syncthreads();
  const uint32_t n = s.cand_n;
  uint32_t len = 64;
  while (len < n) len <<= 1;
  if (len > (uint32_t)CAND) len = (uint32_t)CAND;
  for (uint32_t i = n + threadIdx.x; i < len; i += WG) s.hi[i] = 0, s.lo[i] = 0;
  __syncthreads();
  sortsel_sort(s, len);
  const uint32_t keep = n < K ? n : K;
  if (threadIdx.x == 0) {
    s.cand_n = keep;
    if (keep == K) s.have_tau = 1, s.tau_hi = s.hi[K - 1], s.tau_lo = s.lo[K - 1];
  }
  __syncthreads();
  return keep;
}

// DST: the batch's standing destination.  DST_WIDE: a wide one (a.srows_dst) -- the kernel writes the query's wide exchange row
// itself; DST_ORDER: an order-row one (a.orows_dst) -- its order row; DST_NONE: neither
constexpr int DST_NONE = 0, DST_WIDE = 1, DST_ORDER = 2;
template <int DST>
__global__ __launch_bounds__(WG) void sort_select_kernel(SortSelArgs a) {
  __shared__ SortSelSmem s;
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
  if (q >= a.n_queries) return;
  const DevQuery* __restrict__ Q = a.queries + q;
  if (!Q->sort_on) return; // (uniform: the relevance selection answered this query)
  const uint32_t K = Q->k ? (Q->k < (uint32_t)KCAP ? Q->k : (uint32_t)KCAP) : 1u;
  uint32_t n = a.q_cand_n[(size_t)q * QSTRIDE];
  if (n > Q->sort_cap) n = Q->sort_cap;
  const uint32_t lo = (uint32_t)Q->bin_lo, shift = Q->bin_shift;
  // (uniform) mrk_query.order's 64-bit key: the bin of the whole high word, weight and rowid out of the low word by the tie layout
  const bool wide_ord = Q->sort_on == SORT_ON_ORDER;
  const OrderGeom og = Q->ord_geom;
  const uint32_t tie = Q->sort_tie;
  // (uniform) MRK_ORDER_WEIGHT_FIRST_*: the weight, in hi's high dword, takes the bin; the parts' mapped key is hi's low : lo's high dword
  const bool wfirst = Q->sort_on == SORT_ON_WEIGHT;
  const int32_t wlo = Q->bin_lo;
  const ulonglong2* __restrict__ src = reinterpret_cast<const ulonglong2*>(a.scand) + Q->sort_off;
  if (tid < 64) {
    const uint32_t tb = threshold_bin(a.q_hist + (uint64_t)q * NBINS, K);
    if (tid == 0) s.tau_bin = tb, s.cand_n = 0, s.have_tau = 0, s.tau_hi = 0, s.tau_lo = 0;
  }
  __syncthreads();
  const uint32_t tau_bin = s.tau_bin;
  for (uint32_t f0 = 0; f0 < n; f0 += WG) {
    if (s.cand_n > (uint32_t)(CAND - WG)) sortsel_compact(s, K); // (uniform: cand_n is read behind a barrier)
    const bool have_tau = s.have_tau != 0;
    const uint64_t th = s.tau_hi, tl = s.tau_lo;
    const uint32_t f = f0 + tid;
    bool push = false;
    ulonglong2 c = make_ulonglong2(0, 0);
    if (f < n) {
      c = src[f];
      const uint32_t bin = wfirst ? wfirst_bin(tie, wlo, shift, wfirst_weight(tie, c.x)) : wide_ord ? order_bin(og, c.x) : sort_bin(lo, shift, (uint32_t)(c.x >> 32));
      push = bin >= tau_bin && (!have_tau || sortkey_gt(c.x, c.y, th, tl));
    }
    const uint64_t bal = __ballot(push);
    if (bal) {
      uint32_t basep = 0;
      if (lane == 0) basep = atomicAdd(&s.cand_n, (uint32_t)__popcll(bal));
      basep = rdlane(basep, 0);
      if (push) {
        const uint32_t at = basep + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        s.hi[at] = c.x, s.lo[at] = c.y;
      }
    }
    __syncthreads();
  }
  const uint32_t m = sortsel_compact(s, K); // sorted best first
  // the rows leave in the relevance format: make_key(true weight, global rowid)
  for (uint32_t i = tid; i < m; i += WG) {
    const uint64_t h = s.hi[i], l = s.lo[i];
    const uint64_t key = wfirst     ? make_key(wfirst_weight(tie, h), wfirst_rowid(l))
                         : wide_ord ? make_key(order_lo_weight(tie, l), order_lo_rowid(tie, l))
                                    : make_key((int32_t)(uint32_t)l, ~(uint32_t)(l >> 32));
    const uint64_t mk = wfirst ? wfirst_parts_key(h, l) : wide_ord ? h : h & 0xFFFFFFFF00000000ull; // (weight-first: the parts' key d1 : d2)
    a.out_keys[(uint64_t)q * KCAP + i] = key;
    if (a.h_keys) a.h_keys[(uint64_t)q * KCAP + i] = key;
    a.out_mkeys[(uint64_t)q * KCAP + i] = (uint32_t)(mk >> 32); // the mapped key travels with the row (wide exchange rows)
    if (a.out_mkeys64) a.out_mkeys64[(uint64_t)q * KCAP + i] = mk; // ... all of it (order rows)
  }
  // (a 64-bit key does not fit a wide row: pack_srows_kernel marks that query's row MRK_ROW_DECLINED; no exchange row carries the
  // weight's position yet: pack_srows_kernel / pack_orows_kernel mark a weight-first query's row the same way)
  if (DST == DST_WIDE && !wide_ord && !wfirst) { // sel_sort_kernel's rule: a query whose candidate list overflowed leaves empty with MRK_ROW_RERUN
    const bool bad = (a.q_flags[q] & (QF_OVERFLOW | QF_FSM)) != 0;
    const uint32_t nr = bad ? 0u : m;
    uint64_t* __restrict__ row = a.srows_dst + (uint64_t)q * SROW_WORDS;
    for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) {
      const uint64_t l = s.lo[i];
      row[i] = i < nr ? make_key((int32_t)(uint32_t)l, ~(uint32_t)(l >> 32)) : 0ull;
    }
    for (uint32_t i = tid; i < (uint32_t)KCAP / 2; i += WG) {
      const uint64_t m0 = 2 * i < nr ? s.hi[2 * i] >> 32 : 0ull, m1 = 2 * i + 1 < nr ? s.hi[2 * i + 1] >> 32 : 0ull;
      row[SROW_MKEYS + i] = m0 | (m1 << 32);
    }
    if (tid == 0) {
      row[KCAP] = nr;
      row[KCAP + 1] = bad ? ROW_RERUN : (a.q_total[q] & ~ROW_FLAG_MASK);
      row[SROW_SPEC] = sort_spec_word(Q->sort_flags, Q->sort_tie, Q->sort_bits);
    }
  }
  if (DST == DST_ORDER && !wfirst) { // the same rule; sorts and 64-bit orders alike
    const bool bad = (a.q_flags[q] & (QF_OVERFLOW | QF_FSM)) != 0;
    const uint32_t nr = bad ? 0u : m;
    uint64_t* __restrict__ row = a.orows_dst + (uint64_t)q * OROW_WORDS;
    for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) {
      const uint64_t h = s.hi[i], l = s.lo[i];
      const uint64_t key = wide_ord ? make_key(order_lo_weight(tie, l), order_lo_rowid(tie, l)) : make_key((int32_t)(uint32_t)l, ~(uint32_t)(l >> 32));
      row[i] = i < nr ? key : 0ull;
      row[OROW_MKEYS + i] = i < nr ? (wide_ord ? h : h & 0xFFFFFFFF00000000ull) : 0ull;
    }
    if (tid == 0) {
      row[KCAP] = nr;
      row[KCAP + 1] = bad ? ROW_RERUN : (a.q_total[q] & ~ROW_FLAG_MASK);
      row[OROW_SPEC] = order_spec_word(Q->sort_on, Q->sort_flags, Q->sort_bits, Q->ord_flags, Q->ord_bits, Q->sort_tie);
    }
  }
  if (tid == 0) {
    a.out_cnt[q] = m;
    if (a.h_cnt) a.h_cnt[q] = m;
  }
}

void launch_sort_select(const SortSelArgs& a, void* stream) {
  if (!a.n_queries) return;
  if (a.orows_dst)
    hipLaunchKernelGGL(sort_select_kernel<DST_ORDER>, dim3(a.n_queries), dim3(WG), 0, (hipStream_t)stream, a);
  else if (a.srows_dst)
    hipLaunchKernelGGL(sort_select_kernel<DST_WIDE>, dim3(a.n_queries), dim3(WG), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(sort_select_kernel<DST_NONE>, dim3(a.n_queries), dim3(WG), 0, (hipStream_t)stream, a);
}

// ---------------------------------------------------------------------------------------
// a batch's results as WIDE exchange rows: KCAP keys | count | total_found | KCAP mapped keys (u32) | spec word
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void pack_srows_kernel(PackSRowsArgs a) {
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  if (q >= a.n) return;
  const DevQuery* __restrict__ Q = a.queries + q;
  // declined words: 1 = the planner declined the query on this segment; 2 = declined for NARROW rows only (a sorted query
  // of a batch with a narrow standing destination) -- a wide row answers it
  const bool declined = a.declined && a.declined[q] == 1u;
  const bool sorted = Q->sort_on != 0 && !declined;
  if (a.skip_sorted && sorted) return; // (uniform) sort_select_kernel<DST_WIDE> wrote this row
  const bool bad = declined || (a.flags && (a.flags[q] & (QF_OVERFLOW | QF_FSM)) != 0);
  const uint32_t n = bad ? 0u : a.cnt[q] < (uint32_t)KCAP ? a.cnt[q] : (uint32_t)KCAP;
  uint64_t* __restrict__ row = a.rows + (uint64_t)q * SROW_WORDS;
  const uint32_t nm = sorted && a.mkeys ? n : 0u; // a relevance row's u32 plane is zero
  for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) row[i] = i < n ? a.keys[(uint64_t)q * KCAP + i] : 0ull;
  for (uint32_t i = tid; i < (uint32_t)KCAP / 2; i += WG) {
    const uint64_t m0 = 2 * i < nm ? a.mkeys[(uint64_t)q * KCAP + 2 * i] : 0u, m1 = 2 * i + 1 < nm ? a.mkeys[(uint64_t)q * KCAP + 2 * i + 1] : 0u;
    row[SROW_MKEYS + i] = m0 | (m1 << 32);
  }
  if (tid == 0) {
    row[KCAP] = n;
    row[KCAP + 1] = declined ? ROW_DECLINED : bad ? ROW_RERUN : (a.total[q] & ~ROW_FLAG_MASK);
    row[SROW_SPEC] = sorted ? sort_spec_word(Q->sort_flags, Q->sort_tie, Q->sort_bits) : 0ull;
  }
}

void launch_pack_srows(const PackSRowsArgs& a, void* stream) {
  if (!a.n) return;
  hipLaunchKernelGGL(pack_srows_kernel, dim3(a.n), dim3(WG), 0, (hipStream_t)stream, a);
}

// ---------------------------------------------------------------------------------------
// merge of <= 8 sorted WIDE rows per query: merge_rows_kernel's pairwise bitonic merges (mrk_select.hip) over entries of
// 12 bytes -- the u64 key and, in a plane of its own, the u32 mapped key.  The weight and the docid come out of the u64 key,
// so a sorted query compares (mapped key, the key as the tie rule reads it); a relevance query (spec 0) compares the key alone:
// exactly merge_rows_kernel's order.  LDS: P lists x KCAP x 12 B = 96 KB for 8 lists (one workgroup per CU on gfx950's 160 KB;
// 48 KB and three workgroups for up to 4 lists).
// ---------------------------------------------------------------------------------------
// the u64 key as tie rule `tie` orders it, larger = better; the zero key is the lists' padding and stays the smallest
template <uint32_t TIE>
__device__ __forceinline__ uint64_t tie_key(uint64_t k) {
  if (TIE == 1u) return k;
  if (k == 0ull) return 0ull;
  return TIE == 2u ? k ^ 0xFFFFFFFF00000000ull : k & 0xFFFFFFFFull; // weight ascending / the weight is no part of the order
}

template <bool SORTED, uint32_t TIE>
static __device__ void merge_srows_rounds(uint64_t* mk, uint32_t* mm, uint32_t P) {
  const uint32_t tid = threadIdx.x;
  auto less = [](uint64_t xk, uint32_t xm, uint64_t yk, uint32_t ym) -> bool {
    if (SORTED && xm != ym) return xm < ym;
    return tie_key<TIE>(xk) < tie_key<TIE>(yk);
  };
  for (uint32_t step = 1; step < P; step <<= 1) { // this round merges list slot 2 p step with slot (2 p + 1) step
    const uint32_t pairs = P / (2 * step);
    for (uint32_t t = tid; t < pairs * KCAP; t += WG) { // top K of A and B as a bitonic sequence, in A's place
      const uint32_t p = t / KCAP, i = t % KCAP;
      const size_t ia = (size_t)(2 * p * step) * KCAP + i, ib = (size_t)((2 * p + 1) * step) * KCAP + (KCAP - 1 - i);
      const uint64_t xk = mk[ia], yk = mk[ib];
      const uint32_t xm = SORTED ? mm[ia] : 0u, ym = SORTED ? mm[ib] : 0u;
      if (less(xk, xm, yk, ym)) {
        mk[ia] = yk;
        if (SORTED) mm[ia] = ym;
      }
    }
    __syncthreads();
    for (uint32_t j = KCAP / 2; j > 0; j >>= 1) { // ... sorted descending by half-cleaners
      for (uint32_t t = tid; t < pairs * (KCAP / 2); t += WG) {
        const uint32_t p = t / (KCAP / 2), i0 = t % (KCAP / 2);
        const size_t base = (size_t)(2 * p * step) * KCAP;
        const size_t i = base + (((i0 & ~(j - 1)) << 1) | (i0 & (j - 1))), ij = i + j;
        const uint64_t xk = mk[i], yk = mk[ij];
        const uint32_t xm = SORTED ? mm[i] : 0u, ym = SORTED ? mm[ij] : 0u;
        if (less(xk, xm, yk, ym)) {
          mk[i] = yk, mk[ij] = xk;
          if (SORTED) mm[i] = ym, mm[ij] = xm;
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(WG) void merge_srows_kernel(MergeRowsArgs a, uint32_t P) { // P = power of two >= n_lists
  extern __shared__ uint64_t mk[];                            // [P][KCAP] keys ...
  uint32_t* mm = reinterpret_cast<uint32_t*>(mk + (size_t)P * KCAP); // ... then [P][KCAP] mapped keys
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  if (q >= a.n_queries) return;
  const uint64_t spec = a.in_rows[(uint64_t)q * SROW_WORDS + SROW_SPEC]; // list 0's; every list must agree
  uint64_t total = 0, flags = 0, have = 0;
  bool mismatch = false;
  for (uint32_t l = 0; l < P; ++l) {
    uint32_t cnt = 0;
    const uint64_t* __restrict__ row = nullptr;
    if (l < a.n_lists) {
      row = a.in_rows + ((uint64_t)l * a.list_stride + q) * SROW_WORDS;
      cnt = (uint32_t)row[KCAP];
      if (cnt > (uint32_t)KCAP) cnt = KCAP;
      const uint64_t t = row[KCAP + 1];
      total += t & ~ROW_FLAG_MASK, flags |= t & ROW_FLAG_MASK, have += cnt;
      mismatch = mismatch || row[SROW_SPEC] != spec;
    }
    for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) mk[l * KCAP + i] = i < cnt ? row[i] : 0ull;
    if (spec) {
      const uint32_t* __restrict__ rm = row ? reinterpret_cast<const uint32_t*>(row + SROW_MKEYS) : nullptr;
      for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) mm[l * KCAP + i] = i < cnt ? rm[i] : 0u;
    }
  }
  __syncthreads();
  // lists that do not compare (differing spec words: other kind / direction / tie rule / width, or a sorted row next to a relevance
  // row), and a sorted query some shard declined: the merged row is no answer -- MRK_ROW_DECLINED and no keys
  const bool none = mismatch || (spec != 0 && (flags & ROW_DECLINED) != 0);
  if (mismatch) flags |= ROW_DECLINED;
  if (!none) { // (uniform)
    const uint32_t tie = sort_spec_tie(spec);
    if (!spec)
      merge_srows_rounds<false, 1u>(mk, mm, P);
    else if (tie == 1u)
      merge_srows_rounds<true, 1u>(mk, mm, P);
    else if (tie == 2u)
      merge_srows_rounds<true, 2u>(mk, mm, P);
    else
      merge_srows_rounds<true, 0u>(mk, mm, P);
  }
  const uint32_t n = none ? 0u : have < a.k ? (uint32_t)have : a.k;
  uint64_t* __restrict__ out = a.out_rows + (uint64_t)(a.out_first + q) * SROW_WORDS;
  for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) out[i] = i < n ? mk[i] : 0ull;
  const uint32_t nm = spec ? n : 0u;
  for (uint32_t i = tid; i < (uint32_t)KCAP / 2; i += WG) {
    const uint64_t m0 = 2 * i < nm ? mm[2 * i] : 0u, m1 = 2 * i + 1 < nm ? mm[2 * i + 1] : 0u;
    out[SROW_MKEYS + i] = m0 | (m1 << 32);
  }
  if (tid == 0) {
    out[KCAP] = n;
    out[KCAP + 1] = (total & ~ROW_FLAG_MASK) | flags; // totals add up, the shards' flag bits are OR-ed through (merge_rows_kernel)
    out[SROW_SPEC] = spec;
    if (a.flags_any) {
      if (flags & ROW_RERUN) a.flags_any[0] = 1u;
      if (flags & ROW_DECLINED) a.flags_any[1] = 1u;
    }
  }
}

void launch_merge_srows(const MergeRowsArgs& a, void* stream) {
  if (!a.n_queries) return;
  uint32_t P = 1;
  while (P < a.n_lists) P <<= 1;
  const size_t lds = (size_t)P * KCAP * (sizeof(uint64_t) + sizeof(uint32_t));
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)merge_srows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * KCAP * (int)(sizeof(uint64_t) + sizeof(uint32_t)));
    attr_set = true;
  }
  hipLaunchKernelGGL(merge_srows_kernel, dim3(a.n_queries), dim3(WG), lds, (hipStream_t)stream, a, P);
}

// ---------------------------------------------------------------------------------------
// a batch's results as ORDER rows: KCAP keys | count | total_found | KCAP mapped keys (u64) | order spec word.  Sorts and 64-bit
// orders alike leave with their mapped keys; relevance queries with spec 0 and a zero plane.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void pack_orows_kernel(PackORowsArgs a) {
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  if (q >= a.n) return;
  const DevQuery* __restrict__ Q = a.queries + q;
  const bool declined = a.declined && a.declined[q] == 1u; // (2 = declined for narrow rows only)
  const bool sorted = Q->sort_on != 0 && !declined;
  if (a.skip_sorted && sorted) return; // (uniform) sort_select_kernel<DST_ORDER> wrote this row
  const bool bad = declined || (a.flags && (a.flags[q] & (QF_OVERFLOW | QF_FSM)) != 0);
  const uint32_t n = bad ? 0u : a.cnt[q] < (uint32_t)KCAP ? a.cnt[q] : (uint32_t)KCAP;
  uint64_t* __restrict__ row = a.rows + (uint64_t)q * OROW_WORDS;
  // a 64-bit key needs the 64-bit plane; a sort's key is whole in the u32 plane too (a batch that never saw a 64-bit key has no other)
  const bool wide_ord = Q->sort_on == SORT_ON_ORDER;
  const uint32_t nm = sorted && (a.mkeys64 || (a.mkeys && !wide_ord)) ? n : 0u;
  for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) {
    row[i] = i < n ? a.keys[(uint64_t)q * KCAP + i] : 0ull;
    row[OROW_MKEYS + i] = i >= nm ? 0ull : a.mkeys64 ? a.mkeys64[(uint64_t)q * KCAP + i] : (uint64_t)a.mkeys[(uint64_t)q * KCAP + i] << 32;
  }
  if (tid == 0) {
    row[KCAP] = n;
    row[KCAP + 1] = declined ? ROW_DECLINED : bad ? ROW_RERUN : (a.total[q] & ~ROW_FLAG_MASK);
    row[OROW_SPEC] = sorted ? order_spec_word(Q->sort_on, Q->sort_flags, Q->sort_bits, Q->ord_flags, Q->ord_bits, Q->sort_tie) : 0ull;
  }
}

void launch_pack_orows(const PackORowsArgs& a, void* stream) {
  if (!a.n) return;
  hipLaunchKernelGGL(pack_orows_kernel, dim3(a.n), dim3(WG), 0, (hipStream_t)stream, a);
}

// ---------------------------------------------------------------------------------------
// merge of <= 8 sorted ORDER rows per query: the same pairwise bitonic merges over entries of 16 bytes -- the u64 key and, in a
// plane of its own, the u64 mapped key.  An ordered query compares (mapped key, the key as the tie rule reads it); a relevance
// query (spec 0) compares the key alone and never touches the mapped plane: exactly merge_rows_kernel's order.
// LDS: P lists x KCAP x 16 B = 128 KB for 8 lists (one workgroup per CU on gfx950's 160 KB; 64 KB and two workgroups for up to 4).
// ---------------------------------------------------------------------------------------
template <bool SORTED, uint32_t TIE>
static __device__ void merge_orows_rounds(uint64_t* mk, uint64_t* mm, uint32_t P) {
  const uint32_t tid = threadIdx.x;
  auto less = [](uint64_t xk, uint64_t xm, uint64_t yk, uint64_t ym) -> bool {
    if (SORTED && xm != ym) return xm < ym;
    return tie_key<TIE>(xk) < tie_key<TIE>(yk);
  };
  for (uint32_t step = 1; step < P; step <<= 1) { // this round merges list slot 2 p step with slot (2 p + 1) step
    const uint32_t pairs = P / (2 * step);
    for (uint32_t t = tid; t < pairs * KCAP; t += WG) { // top K of A and B as a bitonic sequence, in A's place
      const uint32_t p = t / KCAP, i = t % KCAP;
      const size_t ia = (size_t)(2 * p * step) * KCAP + i, ib = (size_t)((2 * p + 1) * step) * KCAP + (KCAP - 1 - i);
      const uint64_t xk = mk[ia], yk = mk[ib];
      const uint64_t xm = SORTED ? mm[ia] : 0ull, ym = SORTED ? mm[ib] : 0ull;
      if (less(xk, xm, yk, ym)) {
        mk[ia] = yk;
        if (SORTED) mm[ia] = ym;
      }
    }
    __syncthreads();
    for (uint32_t j = KCAP / 2; j > 0; j >>= 1) { // ... sorted descending by half-cleaners
      for (uint32_t t = tid; t < pairs * (KCAP / 2); t += WG) {
        const uint32_t p = t / (KCAP / 2), i0 = t % (KCAP / 2);
        const size_t base = (size_t)(2 * p * step) * KCAP;
        const size_t i = base + (((i0 & ~(j - 1)) << 1) | (i0 & (j - 1))), ij = i + j;
        const uint64_t xk = mk[i], yk = mk[ij];
        const uint64_t xm = SORTED ? mm[i] : 0ull, ym = SORTED ? mm[ij] : 0ull;
        if (less(xk, xm, yk, ym)) {
          mk[i] = yk, mk[ij] = xk;
          if (SORTED) mm[i] = ym, mm[ij] = xm;
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(WG) void merge_orows_kernel(MergeRowsArgs a, uint32_t P) { // P = power of two >= n_lists
  extern __shared__ uint64_t ok[];          // [P][KCAP] keys ...
  uint64_t* om = ok + (size_t)P * KCAP;     // ... then [P][KCAP] mapped keys
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  if (q >= a.n_queries) return;
  // The query's spec word: that of the lists which answer it, and they must agree.  A list that carries the query with MRK_ROW_DECLINED
  // has no say: a shard whose planner declined the query holds no order for it and sends spec 0 (pack_orows_kernel), so the merged
  // row's spec word does not depend on which list declined.
  uint64_t spec = 0;
  bool have_spec = false, mismatch = false;
  for (uint32_t l = 0; l < a.n_lists; ++l) { // (uniform: scalar loads)
    const uint64_t* __restrict__ row = a.in_rows + ((uint64_t)l * a.list_stride + q) * OROW_WORDS;
    if (row[KCAP + 1] & ROW_DECLINED) continue;
    const uint64_t sp = row[OROW_SPEC];
    if (!have_spec) spec = sp, have_spec = true;
    mismatch = mismatch || sp != spec;
  }
  uint64_t total = 0, flags = 0, have = 0;
  for (uint32_t l = 0; l < P; ++l) {
    uint32_t cnt = 0;
    const uint64_t* __restrict__ row = nullptr;
    if (l < a.n_lists) {
      row = a.in_rows + ((uint64_t)l * a.list_stride + q) * OROW_WORDS;
      cnt = (uint32_t)row[KCAP];
      if (cnt > (uint32_t)KCAP) cnt = KCAP;
      const uint64_t t = row[KCAP + 1];
      total += t & ~ROW_FLAG_MASK, flags |= t & ROW_FLAG_MASK, have += cnt;
    }
    for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) ok[l * KCAP + i] = i < cnt ? row[i] : 0ull;
    if (spec)
      for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) om[l * KCAP + i] = i < cnt ? row[OROW_MKEYS + i] : 0ull;
  }
  __syncthreads();
  // answering lists that do not compare (spec words differing in any bit: direction of either part, kind, width, tie rule, a sort
  // next to a 64-bit order, a relevance row next to either), and an ordered query some shard declined: MRK_ROW_DECLINED and no keys
  const bool none = mismatch || (spec != 0 && (flags & ROW_DECLINED) != 0);
  if (mismatch) flags |= ROW_DECLINED;
  if (!none) { // (uniform)
    const uint32_t tie = order_spec_tie(spec);
    if (!spec)
      merge_orows_rounds<false, 1u>(ok, om, P);
    else if (tie == 1u)
      merge_orows_rounds<true, 1u>(ok, om, P);
    else if (tie == 2u)
      merge_orows_rounds<true, 2u>(ok, om, P);
    else
      merge_orows_rounds<true, 0u>(ok, om, P);
  }
  const uint32_t n = none ? 0u : have < a.k ? (uint32_t)have : a.k;
  uint64_t* __restrict__ out = a.out_rows + (uint64_t)(a.out_first + q) * OROW_WORDS;
  const uint32_t nm = spec ? n : 0u;
  for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) {
    out[i] = i < n ? ok[i] : 0ull;
    out[OROW_MKEYS + i] = i < nm ? om[i] : 0ull;
  }
  if (tid == 0) {
    out[KCAP] = n;
    out[KCAP + 1] = (total & ~ROW_FLAG_MASK) | flags; // totals add up, the shards' flag bits are OR-ed through (merge_rows_kernel)
    out[OROW_SPEC] = spec;
    if (a.flags_any) {
      if (flags & ROW_RERUN) a.flags_any[0] = 1u;
      if (flags & ROW_DECLINED) a.flags_any[1] = 1u;
    }
  }
}

void launch_merge_orows(const MergeRowsArgs& a, void* stream) {
  if (!a.n_queries) return;
  uint32_t P = 1;
  while (P < a.n_lists) P <<= 1;
  const size_t lds = (size_t)P * KCAP * 2 * sizeof(uint64_t);
  // the 128 KB of 5-8 lists need the function's limit raised, once per DEVICE (the attribute belongs to the device's copy of the
  // kernel); contexts of several devices launch from threads of their own, so the marks are atomic -- raising twice is harmless.  A
  // refusal is not marked: the launch then fails with the runtime's own error, which the caller's hipGetLastError reports.
  static std::atomic<bool> raised[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
  if (dev < 0 || !raised[dev].load(std::memory_order_acquire)) {
    const hipError_t e = hipFuncSetAttribute((const void*)merge_orows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * KCAP * 2 * (int)sizeof(uint64_t));
    if (e == hipSuccess && dev >= 0) raised[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(merge_orows_kernel, dim3(a.n_queries), dim3(WG), lds, (hipStream_t)stream, a, P);
}

} // namespace mrk
