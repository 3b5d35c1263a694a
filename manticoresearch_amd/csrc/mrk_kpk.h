// mrk_kpk.h -- packed-doclist block access shared by the block-scan kernel and the window-driven tree kernel: a
// 64-entry register chunk of a keyword's block index, a block's words straight into registers, and the decode of the
// two docs a lane owns (mrk_pack.cpp layout).  gfx950 / wave64.
#pragma once
#include "mrk_kcommon.h"

namespace mrk {

struct PkChunk {
  uint32_t first; // block index (within the term) held by lane 0
  uint32_t bp1;   // first possible rowid of block first+lane (INF past the end)
  uint32_t doff;  // word offset of its deltas
  uint32_t w;     // bits per delta / PK_WIDE
};

__device__ __forceinline__ void load_pk_chunk(PkChunk& c, const DevSegment& seg, const DevTerm& T, uint32_t first) {
  const uint32_t i = first + lane_id();
  c.first = first;
  if (i < T.nblocks) {
    const uint32_t g = T.blk_first + i;
    c.bp1 = seg.pk_base[g];
    c.doff = seg.pk_doff[g];
    c.w = seg.pk_w[g];
  } else {
    c.bp1 = INF_ROWID;
    c.doff = 0;
    c.w = 0;
  }
}

struct PkRaw {
  uint32_t lo, hi, attr;
};

// a block's words for this lane, straight into registers (issued early, used late)
__device__ __forceinline__ PkRaw issue_pk(const DevSegment& seg, const DevTerm& T, const PkChunk& c, uint32_t ci) {
  const uint32_t lane = lane_id();
  const uint32_t w = rdlane(c.w, ci);
  const uint32_t* __restrict__ dp = seg.pk_delta + rdlane(c.doff, ci);
  PkRaw r;
  if (w == PK_WIDE) {
    r.lo = dp[lane];
    r.hi = dp[64 + lane];
  } else {
    const uint32_t wi = (lane * 2 * w) >> 5;
    r.lo = dp[wi];
    r.hi = dp[wi + 1];
  }
  r.attr = seg.pk_attr[(uint64_t)(T.blk_first + c.first + ci) * 64 + lane];
  return r;
}

// rowids of the block's docs lane and lane+64 (o0/o1: their offsets from the block base)
__device__ __forceinline__ void decode_pk(const PkRaw& raw, uint32_t w, uint32_t bp1, uint32_t nd, uint32_t& r0, uint32_t& r1,
                                          uint32_t& o0, uint32_t& o1, bool& ok0, bool& ok1) {
  const uint32_t lane = lane_id();
  if (w == PK_WIDE) {
    o0 = raw.lo;
    o1 = raw.hi;
  } else {
    const uint32_t f = __builtin_amdgcn_alignbit(raw.hi, raw.lo, (lane * 2 * w) & 31u);
    const uint32_t mask = (1u << w) - 1u;
    o0 = f & mask;
    o1 = (f >> w) & mask;
  }
  ok0 = lane < nd;
  ok1 = lane + 64 < nd;
  r0 = bp1 + o0;
  r1 = bp1 + o1;
}

// ---- one doc of a block on its own: offsets are stored at a fixed width from the block base, so slot i needs no other slot.
// (host code too: tests/cpp/pk_probe.cpp runs these against the plain decode)

// the window of `sh` + 32 bits that decode_pk reads
__host__ __device__ inline uint32_t pk_alignbit(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u));
#endif
}

// offset from the block base of doc i (0 .. 127) of the block whose words start at dp; w: its width.  A narrow block's doc i
// lives in value slot 2 * (i & 63) + (i >> 6); the two-word read stays inside the block's 4 * w + 1 words.  w == 0: one doc, offset 0
// (slots past the block's docs hold zeros: the caller compares i with the doc count)
__host__ __device__ inline uint32_t pk_doc_off(const uint32_t* __restrict__ dp, uint32_t w, uint32_t i) {
  if (w == PK_WIDE) return dp[i];
  if (w == 0) return 0u;
  const uint32_t bit = (2u * (i & 63u) + (i >> 6)) * w;
  struct __attribute__((packed, aligned(4))) Pair {
    uint32_t lo, hi;
  };
  const Pair pr = *reinterpret_cast<const Pair*>(dp + (bit >> 5));
  return pk_alignbit(pr.hi, pr.lo, bit & 31u) & ((1u << w) - 1u);
}

// one step of the lower bound below: doc `at`'s offset against `want`; a doc index past the block's docs compares as +infinity
__host__ __device__ inline bool pk_doc_below(uint32_t off_at, uint32_t at, uint32_t nd, uint32_t want) { return at < nd && off_at < want; }

// Lower bound over the docs of one block in seven fixed steps: the number of docs among the block's first 127 whose offset is below
// `want`, i.e. min(index of the first doc with offset >= want, 127).  A hit is pos < nd && pk_doc_off(pos) == want; with all 128 docs
// below `want` the result is 127, whose offset differs from `want`.
// This function is the host-side model of the kernel's loop, not the loop itself: scan_p2_kernel writes the same seven steps out
// for a lane's two docs side by side, so that both docs' reads of a step are in flight together.  What the two share, and what
// tests/cpp/pk_probe.cpp therefore checks of the device code, are the step's parts: pk_doc_off and pk_doc_below.
__host__ __device__ inline uint32_t pk_lower_bound(const uint32_t* __restrict__ dp, uint32_t w, uint32_t nd, uint32_t want) {
  uint32_t pos = 0;
  for (uint32_t step = DEVBLK / 2; step; step >>= 1) {
    const uint32_t at = pos + step - 1;
    if (pk_doc_below(pk_doc_off(dp, w, at), at, nd, want)) pos += step;
  }
  return pos;
}

} // namespace mrk
