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
#include "mrk_kcommon.h"
#include "mrk_kprune.h"
#include "mrk_sortkey.h"

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
      push = sort_bin(lo, shift, (uint32_t)(c.x >> 32)) >= tau_bin && (!have_tau || sortkey_gt(c.x, c.y, th, tl));
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
    const uint64_t l = s.lo[i];
    const uint64_t key = make_key((int32_t)(uint32_t)l, ~(uint32_t)(l >> 32));
    a.out_keys[(uint64_t)q * KCAP + i] = key;
    if (a.h_keys) a.h_keys[(uint64_t)q * KCAP + i] = key;
  }
  if (tid == 0) {
    a.out_cnt[q] = m;
    if (a.h_cnt) a.h_cnt[q] = m;
  }
}

void launch_sort_select(const SortSelArgs& a, void* stream) {
  if (!a.n_queries) return;
  hipLaunchKernelGGL(sort_select_kernel, dim3(a.n_queries), dim3(WG), 0, (hipStream_t)stream, a);
}

} // namespace mrk
