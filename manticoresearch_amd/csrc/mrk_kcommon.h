// mrk_kcommon.h -- device helpers shared by the gfx950 kernels (wave64).
#pragma once
#include <hip/hip_runtime.h>

#include "mrk_dev.h"

namespace mrk {

constexpr uint32_t NOBLK = 0xFFFFFFFFu;
constexpr uint32_t INF_ROWID = 0xFFFFFFFFu;
constexpr int CHUNK = 63; // usable block-index entries per 64-lane metadata chunk (one spare for "next")

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// ---- wave-wide primitives on DPP (row_shr within rows of 16, then row_bcast15 / row_bcast31)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t old, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xf, false);
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  v += dpp_u32<0x111, 0xf>(0, v); // row_shr:1
  v += dpp_u32<0x112, 0xf>(0, v); // row_shr:2
  v += dpp_u32<0x114, 0xf>(0, v); // row_shr:4
  v += dpp_u32<0x118, 0xf>(0, v); // row_shr:8
  v += dpp_u32<0x142, 0xa>(0, v); // row_bcast:15 -> rows 1,3
  v += dpp_u32<0x143, 0xc>(0, v); // row_bcast:31 -> rows 2,3
  return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  v = min(v, dpp_u32<0x111, 0xf>(0xFFFFFFFFu, v));
  v = min(v, dpp_u32<0x112, 0xf>(0xFFFFFFFFu, v));
  v = min(v, dpp_u32<0x114, 0xf>(0xFFFFFFFFu, v));
  v = min(v, dpp_u32<0x118, 0xf>(0xFFFFFFFFu, v));
  v = min(v, dpp_u32<0x142, 0xa>(0xFFFFFFFFu, v));
  v = min(v, dpp_u32<0x143, 0xc>(0xFFFFFFFFu, v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint64_t rdlane64(uint64_t v, uint32_t l) {
  return ((uint64_t)rdlane((uint32_t)(v >> 32), l) << 32) | rdlane((uint32_t)v, l);
}

// LDS hand-off between lanes of ONE wave: make earlier ds_writes visible and keep the
// compiler from moving LDS accesses across this point.
// (MRK_WAVE_FENCE=1: wavefront-scope fences -- ordering for the compiler only.  One wave's DS instructions execute in issue
// order, so another lane's earlier ds_write / ds_or is seen by a later ds_read without any s_waitcnt; the workgroup-scope
// form also drains vmcnt, i.e. stalls on every global load and store still in flight.)
#ifndef MRK_WAVE_FENCE
#define MRK_WAVE_FENCE 0
#endif
__device__ __forceinline__ void wave_lds_fence() {
#if MRK_WAVE_FENCE
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#else
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

// bit k of the result = byte k of w is a varint terminator (bit 7 clear)
__device__ __forceinline__ uint32_t term4(uint32_t w) { return (((~w & 0x80808080u) >> 7) * 0x10204080u) >> 28; }

__host__ __device__ __forceinline__ float term_tfidf(uint32_t tf, float idf) {
  // float(hits) / float(hits + 1.2f) * idf  -- searchnode.cpp:2828; no contraction (-ffp-contract=off)
  const float fh = (float)tf;
  const float den = fh + 1.2f;
  const float q = fh / den;
  return q * idf;
}

// Upper bound of a keyword's tfidf over the postings of a bitmap word whose largest-tf class is cls (DevSegment::bm_wmax: 1..14 = that
// tf, 15 = 15 and more), in the very floats score() reads from its tfidf table.  idf >= 0: tfidf rises with tf, so the class's own
// value bounds every posting of the word, and the idf bounds class 15 (tf / (tf + 1.2) never exceeds 1 in fp32; this covers the
// tf >= 255 escape).  idf < 0: tfidf falls with tf and every posting has tf >= 1.  (tests/cpp/bm_wmax.cpp checks it for every tf up to 300.)
__host__ __device__ __forceinline__ float bm_wmax_bound(uint32_t cls, float idf) {
  if (idf < 0.0f) return term_tfidf(1u, idf);
  return cls == 15u ? idf : term_tfidf(cls, idf);
}

// The bound's pruning test as a cutoff on bmw, the (int32_t)((acc + 0.5f) * 1000.0f) of the bound's float sum: the smallest x with
//   weight_bin(bin_lo, bin_shift, (int32_t)(((uint32_t)x + rmax1000) * index_weight)) >= tau_bin,
// so that "the word's best weight lies in a bin behind the threshold" is x < bm_wmax_cut(..).  tau_bin == 0 drops nothing (INT32_MIN).
// Otherwise, with w = (x + rmax1000) * index_weight: weight_bin(w) >= tau_bin  <=>  w >= T = bin_lo + (tau_bin << bin_shift) (the
// clamp to bin 1023 does not matter for tau_bin <= 1023)  <=>  x >= ceil(T / index_weight) - rmax1000, for index_weight > 0.
// Preconditions, the ones the kernel's wprune holds: index_weight > 0 and a geometry of bins_by_weight (mrk_plan.cpp) that is not its
// fallback.  That one is only set when every corner (bm_lo|bm_hi + (rmin|rmax) * 1000) * index_weight of the weights lies strictly
// inside int32, bm_hi being above every float sum of two tfidf bounds and rmax the sum of the positive field weights: so
// (x + rmax1000) * index_weight fits int32 for every x the bound can produce, the kernel's uint32 product never wraps there, and the
// equivalences above hold in plain integers.  bin_shift <= 22 then (a span below 2^32 in 1024 bins), so tau_bin << bin_shift fits
// uint32 and |T| < 2^33.
// No division runs per threshold: the caller keeps inv = bm_cut_inv(index_weight), worked out once per wave, and the quotient comes from a
// 32-bit multiply-high with one fix-up, all of it scalar work on wave-uniform values.
//  - T is first capped at INT32_MAX (in uint32, as an offset from bin_lo): no weight of such a geometry reaches INT32_MAX, so
//    "w >= T" is false for every T from there up all the same, and the capped T fits int32.
//  - floor(n / d) for uint32 n: inv = floor((2^32 - 1) / d) lies in (2^32 / d - 1, 2^32 / d], so n * inv / 2^32 lies in (n / d - 1, n / d]
//    and its floor q0 is floor(n / d) or one below; the remainder n - q0 * d tells which.
//  - ceil(T / d) is floor((T - 1) / d) + 1 for T > 0 and -floor(-T / d) for T <= 0.
// The result is clamped to int32: a cutoff below INT32_MIN drops nothing, as it should, and one above INT32_MAX cannot occur (T <= INT32_MAX).
// (tests/cpp/bm_cut.cpp checks it against the expression above.)
__host__ __device__ __forceinline__ uint32_t bm_cut_inv(uint32_t index_weight) { return 0xFFFFFFFFu / index_weight; }

__host__ __device__ __forceinline__ int32_t bm_wmax_cut(int32_t bin_lo, uint32_t bin_shift, uint32_t tau_bin, uint32_t rmax1000, uint32_t index_weight,
                                                        uint32_t inv) {
  if (!tau_bin) return INT32_MIN;
  const uint32_t room = 0x7FFFFFFFu - (uint32_t)bin_lo; // INT32_MAX - bin_lo, in [0, 2^32)
  uint32_t off = tau_bin << bin_shift;
  off = off < room ? off : room;
  const int32_t T = (int32_t)((uint32_t)bin_lo + off); // (in range: no wrap)
  const uint32_t n = T > 0 ? (uint32_t)T - 1u : 0u - (uint32_t)T;
  uint32_t q = (uint32_t)(((uint64_t)n * inv) >> 32);
  if (n - q * index_weight >= index_weight) ++q;
  const int64_t c = (T > 0 ? (int64_t)q + 1 : -(int64_t)q) - (int64_t)rmax1000;
  return c < (int64_t)INT32_MIN ? INT32_MIN : (int32_t)c;
}
__host__ __device__ __forceinline__ int32_t bm_wmax_cut(int32_t bin_lo, uint32_t bin_shift, uint32_t tau_bin, uint32_t rmax1000, uint32_t index_weight) {
  return bm_wmax_cut(bin_lo, bin_shift, tau_bin, rmax1000, index_weight, bm_cut_inv(index_weight));
}

// bitonic sort of c[0..len) descending, all WG threads; len = a power of two <= CAND (entries past the keys are zeros: a
// short list sorts a short network -- 15 stages for 32 keys instead of the 66 of the full buffer)
__device__ void sort_cand_desc(uint64_t* c, uint32_t len = (uint32_t)CAND) {
  for (uint32_t k = 2; k <= len; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < len / 2; t += WG) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)); // lower index of the pair
        const uint32_t p = i | j;
        const uint64_t x = c[i], y = c[p];
        const bool desc = (i & k) == 0;
        if ((x < y) == desc) {
          c[i] = y;
          c[p] = x;
        }
      }
      __syncthreads();
    }
  }
}

// exclusive positions of flags laid out as i = tid + r*WG; returns total
__device__ __forceinline__ uint32_t block_scan2(uint32_t* wave_cnt, bool f0, bool f1, uint32_t& pos0, uint32_t& pos1) {
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  const uint64_t b0 = __ballot(f0), b1 = __ballot(f1);
  __syncthreads(); // wave_cnt reuse
  if (lane == 0) {
    wave_cnt[wave] = __popcll(b0);
    wave_cnt[WAVES + wave] = __popcll(b1);
  }
  __syncthreads();
  uint32_t base0 = 0, base1 = 0, tot0 = 0, tot1 = 0;
#pragma unroll
  for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) {
    const uint32_t c0 = wave_cnt[w], c1 = wave_cnt[WAVES + w];
    if (w < wave) base0 += c0, base1 += c1;
    tot0 += c0;
    tot1 += c1;
  }
  const uint64_t lt = (1ull << lane) - 1ull;
  pos0 = base0 + __popcll(b0 & lt);
  pos1 = tot0 + base1 + __popcll(b1 & lt);
  return tot0 + tot1;
}


// wave-cooperative search: largest i in [lo, n) with base[i] <= r, given base[lo] <= r.
// 64-ary: every step probes 64 evenly spaced entries.
__device__ uint32_t wave_find_block(const uint32_t* __restrict__ base, uint32_t lo, uint32_t n, uint32_t r) {
  const uint32_t lane = lane_id();
  uint32_t hi = n;
  while (hi - lo > 1) {
    const uint32_t len = hi - lo;
    const uint32_t stride = (len + 63) / 64;
    const uint32_t idx = lo + lane * stride;
    const bool le = idx < hi && base[idx] <= r;
    const uint64_t bal = __ballot(le);
    const uint32_t p = 63u - (uint32_t)__builtin_clzll(bal | 1ull); // lane 0 always qualifies
    const uint32_t nlo = lo + p * stride;
    const uint32_t nhi = nlo + stride < hi ? nlo + stride : hi;
    lo = nlo;
    hi = nhi;
  }
  return lo;
}

// keep the best min(n, k) keys; once k keys are held their worst one is a valid lower bound of
// the query's final K-th best key: raise the shared threshold with it
template <typename S>
__device__ uint32_t compact_cand(S& s, uint32_t k, uint64_t* gtau) {
  __syncthreads();
  const uint32_t n = s.cand_n;
  uint32_t len = 64; // the smallest power of two that holds the keys
  while (len < n) len <<= 1;
  if (len > (uint32_t)CAND) len = (uint32_t)CAND;
  for (uint32_t i = n + threadIdx.x; i < len; i += WG) s.cand[i] = 0;
  __syncthreads();
  sort_cand_desc(s.cand, len);
  const uint32_t keep = n < k ? n : k;
  if (threadIdx.x == 0) {
    s.cand_n = keep;
    if (keep == k && s.cand[k - 1] > s.tau) {
      s.tau = s.cand[k - 1];
      atomicMax((unsigned long long*)gtau, (unsigned long long)s.tau);
    }
  }
  __syncthreads();
  return keep;
}


} // namespace mrk
