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
// Below it: the exchange rows that carry a batch's results across segments and shards, in their three formats (mrk_krows.h) -- one
// pack kernel (pack_xrows_kernel) and one merge of <= 8 lists per query (merge_xrows_kernel), each instantiated per format.
#include "mrk_kcommon.h"
#include "mrk_kprune.h"
#include "mrk_krows.h"
#include "mrk_sortkey.h"

#include <atomic>
#include <type_traits>

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
  // (uniform) which of mrk_sortkey.h's three candidate layouts the list holds, and what its bins are taken from
  const uint32_t sort_on = Q->sort_on, tie = Q->sort_tie, shift = Q->bin_shift;
  const int32_t blo = Q->bin_lo;
  const OrderGeom og = Q->ord_geom;
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
      push = cand_bin(sort_on, tie, blo, shift, og, c.x) >= tau_bin && (!have_tau || sortkey_gt(c.x, c.y, th, tl));
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
  auto key_at = [&](uint32_t i) { return cand_out_key(sort_on, tie, s.hi[i], s.lo[i]); };
  auto mkey_at = [&](uint32_t i) { return cand_mkey(sort_on, s.hi[i], s.lo[i]); };
  for (uint32_t i = tid; i < m; i += WG) {
    const uint64_t key = key_at(i), mk = mkey_at(i);
    a.out_keys[(uint64_t)q * KCAP + i] = key;
    if (a.h_keys) a.h_keys[(uint64_t)q * KCAP + i] = key;
    a.out_mkeys[(uint64_t)q * KCAP + i] = (uint32_t)(mk >> 32); // the mapped key travels with the row (wide exchange rows)
    if (a.out_mkeys64) a.out_mkeys64[(uint64_t)q * KCAP + i] = mk; // ... all of it (order rows)
  }
  // The standing destination's row.  A 64-bit key does not fit a wide row, and the weight's position is carried by an order row's spec
  // word only, where the batch asked for it (a.orows_wfirst): no row is written otherwise, and pack_xrows_kernel marks that query's row
  // MRK_ROW_DECLINED.  sel_sort_kernel's rule (row_total_word): a query
  // whose candidate list overflowed leaves empty with MRK_ROW_RERUN, one that met a run-time decline empty with MRK_ROW_DECLINED.
  if constexpr (DST != DST_NONE) {
    using Fmt = std::conditional_t<DST == DST_WIDE, WideFmt, OrderFmt>;
    const bool wfirst_row = DST == DST_ORDER && a.orows_wfirst != 0u;
    if ((sort_on != SORT_ON_WEIGHT || wfirst_row) && (Fmt::WIDE_KEYS || sort_on != SORT_ON_ORDER)) { // (uniform)
      const uint32_t qf = a.q_flags[q];
      const uint32_t nr = row_unflagged(false, qf) ? m : 0u;
      uint64_t* __restrict__ row = (DST == DST_WIDE ? a.srows_dst : a.orows_dst) + (uint64_t)q * Fmt::WORDS;
      write_row_keys(row, nr, key_at);
      Fmt::store_plane(row, nr, [&](uint32_t i) { return Fmt::mkey_of(mkey_at(i)); });
      if (tid == 0) write_row_header<Fmt>(row, nr, row_total_word(false, qf, a.q_total[q]), Fmt::spec_of(*Q));
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
// a batch's results as exchange rows of one format.  Sorts and 64-bit orders leave with their mapped keys where the format has a
// plane for them; relevance queries with spec 0 and a zero plane.
// ---------------------------------------------------------------------------------------
template <class Fmt>
__global__ __launch_bounds__(WG) void pack_xrows_kernel(PackXRowsArgs a) {
  constexpr bool PLANE = Fmt::MK_BYTES != 0;
  const uint32_t q = blockIdx.x;
  if (q >= a.n) return;
  const bool declined = a.declined && ((a.declined[q] >> Fmt::KIND) & 1u) != 0u; // (the query's decline mask: this format's bit)
  const uint32_t sort_on = PLANE ? a.queries[q].sort_on : 0u; // (narrow rows: a sorted query is a declined one)
  const bool sorted = sort_on != 0 && !declined;
  if (a.skip_sorted && sorted) return; // (uniform) sort_select_kernel wrote this row
  const uint32_t qf = a.flags ? a.flags[q] : 0u;
  const uint32_t n = !row_unflagged(declined, qf) ? 0u : a.cnt[q] < (uint32_t)KCAP ? a.cnt[q] : (uint32_t)KCAP;
  uint64_t* __restrict__ row = a.rows + (uint64_t)q * Fmt::WORDS;
  // a 64-bit key needs the 64-bit plane; a sort's key is whole in the u32 plane too (a batch that never saw a 64-bit key has no other)
  const uint32_t nm = sorted && (a.mkeys64 || (a.mkeys && (!Fmt::WIDE_KEYS || sort_on != SORT_ON_ORDER))) ? n : 0u;
  write_row_keys(row, n, [&](uint32_t i) { return a.keys[(uint64_t)q * KCAP + i]; });
  Fmt::store_plane(row, nm, [&](uint32_t i) { return Fmt::mkey_of(a.mkeys64 ? a.mkeys64[(uint64_t)q * KCAP + i] : (uint64_t)a.mkeys[(uint64_t)q * KCAP + i] << 32); });
  if (threadIdx.x == 0) write_row_header<Fmt>(row, n, row_total_word(declined, qf, a.total[q]), sorted ? Fmt::spec_of(a.queries[q]) : 0ull);
}

void launch_pack_xrows(RowKind kind, const PackXRowsArgs& a, void* stream) {
  if (!a.n) return;
  auto* kernel = kind == ROWS_ORDER ? pack_xrows_kernel<OrderFmt> : kind == ROWS_WIDE ? pack_xrows_kernel<WideFmt> : pack_xrows_kernel<NarrowFmt>;
  hipLaunchKernelGGL(kernel, dim3(a.n), dim3(WG), 0, (hipStream_t)stream, a);
}

// ---------------------------------------------------------------------------------------
// merge of <= 8 sorted rows per query (the shard exchange's merge step; CSphMatchQueue::MoveTo across chunks, sphinxsort.cpp:681-710):
// one workgroup per query, all lists in LDS, merged pairwise by bitonic merges over entries of 8 + Fmt::MK_BYTES bytes -- the u64 key
// and, in a plane of its own, the mapped key.  The weight and the docid come out of the u64 key, so a sorted or ordered query compares
// (mapped key, the key as the tie rule reads it); a relevance query (spec 0), and every query of narrow rows, compares the key alone
// and never touches the mapped plane.  A weight-first order (OSPEC_WFIRST, order rows only) compares the key's weight dword as the
// spec's direction reads it, then the mapped key, then the key's docid dword.  LDS for 8 lists: 64 KB narrow, 96 KB wide, 128 KB order
// rows (one workgroup per CU on gfx950's 160 KB); half that for up to 4 lists.
// ---------------------------------------------------------------------------------------
// the u64 key as tie rule `tie` orders it, larger = better; the zero key is the lists' padding and stays the smallest
template <uint32_t TIE>
__device__ __forceinline__ uint64_t tie_key(uint64_t k) {
  if (TIE == 1u) return k;
  if (k == 0ull) return 0ull;
  return TIE == 2u ? k ^ 0xFFFFFFFF00000000ull : k & 0xFFFFFFFFull; // weight ascending / the weight is no part of the order
}

template <class MK, bool SORTED, uint32_t TIE, bool WFIRST = false>
static __device__ void merge_rounds(uint64_t* mk, MK* mm, uint32_t P) {
  const uint32_t tid = threadIdx.x;
  auto less = [](uint64_t xk, MK xm, uint64_t yk, MK ym) -> bool {
    if (WFIRST) { // TIE = the weight's direction; ~docid is the low dword under either
      const uint64_t xt = tie_key<TIE>(xk), yt = tie_key<TIE>(yk);
      const uint32_t xw = (uint32_t)(xt >> 32), yw = (uint32_t)(yt >> 32);
      if (xw != yw) return xw < yw;
      if (xm != ym) return xm < ym;
      return (uint32_t)xt < (uint32_t)yt;
    }
    if (SORTED && xm != ym) return xm < ym;
    return tie_key<TIE>(xk) < tie_key<TIE>(yk);
  };
  for (uint32_t step = 1; step < P; step <<= 1) { // this round merges list slot 2 p step with slot (2 p + 1) step
    const uint32_t pairs = P / (2 * step);
    for (uint32_t t = tid; t < pairs * KCAP; t += WG) { // top K of A and B as a bitonic sequence, in A's place
      const uint32_t p = t / KCAP, i = t % KCAP;
      const uint32_t ia = 2 * p * step * KCAP + i, ib = (2 * p + 1) * step * KCAP + (KCAP - 1 - i); // (< P KCAP <= 8192)
      const uint64_t xk = mk[ia], yk = mk[ib];
      const MK xm = SORTED ? mm[ia] : MK(0), ym = SORTED ? mm[ib] : MK(0);
      if (less(xk, xm, yk, ym)) {
        mk[ia] = yk;
        if (SORTED) mm[ia] = ym;
      }
    }
    __syncthreads();
    for (uint32_t j = KCAP / 2; j > 0; j >>= 1) { // ... sorted descending by half-cleaners
      for (uint32_t t = tid; t < pairs * (KCAP / 2); t += WG) {
        const uint32_t p = t / (KCAP / 2), i0 = t % (KCAP / 2);
        const uint32_t i = 2 * p * step * KCAP + (((i0 & ~(j - 1)) << 1) | (i0 & (j - 1))), ij = i + j;
        const uint64_t xk = mk[i], yk = mk[ij];
        const MK xm = SORTED ? mm[i] : MK(0), ym = SORTED ? mm[ij] : MK(0);
        if (less(xk, xm, yk, ym)) {
          mk[i] = yk, mk[ij] = xk;
          if (SORTED) mm[i] = ym, mm[ij] = xm;
        }
      }
      __syncthreads();
    }
  }
}

template <class Fmt>
__global__ __launch_bounds__(WG) void merge_xrows_kernel(MergeRowsArgs a, uint32_t P) { // P = power of two >= n_lists
  using MK = typename Fmt::MK;
  constexpr bool PLANE = Fmt::MK_BYTES != 0;
  extern __shared__ uint64_t mk[];                       // [P][KCAP] keys ...
  MK* mm = reinterpret_cast<MK*>(mk + (size_t)P * KCAP); // ... then [P][KCAP] mapped keys (narrow rows: the end of the allocation, never read or written)
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  if (q >= a.n_queries) return;
  // The query's spec word, by the format's election rule
  uint64_t spec = 0;
  bool mismatch = false;
  if (Fmt::ELECT == SPEC_OF_LIST0) spec = a.in_rows[(uint64_t)q * Fmt::WORDS + Fmt::SPEC];
  if (Fmt::ELECT == SPEC_OF_ANSWERING) {
    // a shard whose planner declined the query holds no order for it and sends spec 0 (pack_xrows_kernel), so the merged row's spec
    // word does not depend on which list declined
    bool have_spec = false;
    for (uint32_t l = 0; l < a.n_lists; ++l) { // (uniform: scalar loads)
      const uint64_t* __restrict__ row = a.in_rows + ((uint64_t)l * a.list_stride + q) * Fmt::WORDS;
      if (row[KCAP + 1] & ROW_DECLINED) continue;
      const uint64_t sp = row[Fmt::SPEC];
      if (!have_spec) spec = sp, have_spec = true;
      mismatch = mismatch || sp != spec;
    }
  }
  uint64_t total = 0, flags = 0, have = 0;
  for (uint32_t l = 0; l < P; ++l) {
    uint32_t cnt = 0;
    const uint64_t* __restrict__ row = nullptr;
    if (l < a.n_lists) {
      row = a.in_rows + ((uint64_t)l * a.list_stride + q) * Fmt::WORDS;
      cnt = (uint32_t)row[KCAP];
      if (cnt > (uint32_t)KCAP) cnt = KCAP;
      const uint64_t t = row[KCAP + 1];
      total += t & ~ROW_FLAG_MASK, flags |= t & ROW_FLAG_MASK, have += cnt;
      if (Fmt::ELECT == SPEC_OF_LIST0) mismatch = mismatch || row[Fmt::SPEC] != spec;
    }
    for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) mk[l * KCAP + i] = i < cnt ? row[i] : 0ull;
    if (PLANE && spec)
      for (uint32_t i = tid; i < (uint32_t)KCAP; i += WG) mm[l * KCAP + i] = i < cnt ? Fmt::load_mkey(row, i) : MK(0);
  }
  __syncthreads();
  // a weight-first spec (order rows only) whose direction of the weight is neither DESC nor ASC is no spec: a mismatch
  const bool wfirst = Fmt::WIDE_KEYS && (spec & OSPEC_WFIRST) != 0;
  if (wfirst && !order_spec_wfirst_valid(spec)) mismatch = true;
  // lists that do not compare (spec words differing in any bit: kind, direction of a part, width, tie rule, a sort next to a 64-bit
  // order, a relevance row next to either, a weight-first order next to any other), and a sorted or ordered query some shard
  // declined: the merged row is no answer -- MRK_ROW_DECLINED and no keys
  const bool none = mismatch || (spec != 0 && (flags & ROW_DECLINED) != 0);
  if (mismatch) flags |= ROW_DECLINED;
  if (!none) { // (uniform)
    const uint32_t tie = Fmt::spec_tie(spec);
    if (!PLANE || !spec)
      merge_rounds<MK, false, 1u>(mk, mm, P);
    else if (wfirst) {
      if constexpr (Fmt::WIDE_KEYS) {
        if (tie == 1u)
          merge_rounds<MK, true, 1u, true>(mk, mm, P);
        else
          merge_rounds<MK, true, 2u, true>(mk, mm, P);
      }
    } else if (tie == 1u)
      merge_rounds<MK, true, 1u>(mk, mm, P);
    else if (tie == 2u)
      merge_rounds<MK, true, 2u>(mk, mm, P);
    else
      merge_rounds<MK, true, 0u>(mk, mm, P);
  }
  const uint32_t n = none ? 0u : have < a.k ? (uint32_t)have : a.k;
  uint64_t* __restrict__ out = a.out_rows + (uint64_t)(a.out_first + q) * Fmt::WORDS;
  write_row_keys(out, n, [&](uint32_t i) { return mk[i]; });
  Fmt::store_plane(out, spec ? n : 0u, [&](uint32_t i) { return mm[i]; });
  if (tid == 0) {
    write_row_header<Fmt>(out, n, (total & ~ROW_FLAG_MASK) | flags, spec); // CSphMatchQueue::MoveTo adds the totals up; the shards' flag bits are OR-ed through
    if (a.flags_any) {
      if (flags & ROW_RERUN) a.flags_any[0] = 1u;
      if (flags & ROW_DECLINED) a.flags_any[1] = 1u;
    }
  }
}

template <class Fmt>
static void launch_merge_of(const MergeRowsArgs& a, void* stream) {
  uint32_t P = 1;
  while (P < a.n_lists) P <<= 1;
  constexpr size_t ENTRY = sizeof(uint64_t) + Fmt::MK_BYTES;
  // 5-8 lists need more than the 64 KB a launch may ask for by default: the function's limit is raised, once per DEVICE (the attribute
  // belongs to the device's copy of the kernel); contexts of several devices launch from threads of their own, so the marks are atomic
  // -- raising twice is harmless.  A refusal is not marked: the launch then fails with the runtime's own error, which the caller's
  // hipGetLastError reports.
  static std::atomic<bool> raised[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
  if (dev < 0 || !raised[dev].load(std::memory_order_acquire)) {
    const hipError_t e = hipFuncSetAttribute((const void*)merge_xrows_kernel<Fmt>, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * KCAP * (int)ENTRY);
    if (e == hipSuccess && dev >= 0) raised[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(merge_xrows_kernel<Fmt>, dim3(a.n_queries), dim3(WG), (size_t)P * KCAP * ENTRY, (hipStream_t)stream, a, P);
}

void launch_merge_xrows(RowKind kind, const MergeRowsArgs& a, void* stream) {
  if (!a.n_queries) return;
  if (kind == ROWS_ORDER)
    launch_merge_of<OrderFmt>(a, stream);
  else if (kind == ROWS_WIDE)
    launch_merge_of<WideFmt>(a, stream);
  else
    launch_merge_of<NarrowFmt>(a, stream);
}

} // namespace mrk
