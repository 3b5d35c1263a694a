// mrk_scan_p2.hip -- the lean instance of the block scan over packed doclists: one or two keywords under the weight-sum
// rankers (NONE, BM25, single-keyword PROXIMITY), segments of <= 8 fields, gfx950 / wave64.
//
// Same work items, DevQuery / DevItem and semantics as scan_pk_kernel<false, false> (mrk_scan_pk.hip), which keeps every
// other launch.  The selective two-keyword launches cut their items down to one driver block per wave, so a wave is a
// chain of dependent round trips and little else; what this instance changes serves that chain and the number of waves a
// SIMD can hold against it:
//   * no trees, hit references, match queue, sort descriptors or wide field masks: none of their state is live;
//   * no per-workgroup tables and no workgroup barrier: tfidf(tf) is the reference's three fp32 operations per doc and
//     the field-weight sum a loop over <= 8 scalars, both cheaper here than a table fill for 128 docs;
//   * no LDS histogram and no direct rowid -> slot map: candidates' bins go to the query's histogram with one atomic per
//     distinct bin (hist_add_keys).  A keyword dense enough for the map carries a bitmap and is probed through it;
//   * a sparse second keyword is never decoded block by block: each driver doc finds its own block in the register chunk of
//     the block index and its slot by a lower bound over the packed words themselves (mrk_kpk.h, pk_doc_off), so a driver
//     block costs the same chain of round trips whether its docs fall into one block of that keyword or into sixty.  LDS is
//     the candidate buffer alone, 4 KB per workgroup;
//   * the wave's first loads -- overflow flag, threshold word, block-index chunk -- are requested together;
//   * the dense probe asks for the rank-directory word only in lanes whose bit is set (a second 128-byte line per driver
//     doc otherwise, needed by the few that match): one more dependent round trip, measured 11 % faster than asking for it
//     with the bitmap group.
#include "mrk_kcommon.h"
#include "mrk_kprune.h"
#include "mrk_kpk.h"

namespace mrk {

namespace {

constexpr int P2_CBUF = 128; // candidates a wave collects before it publishes them

struct __align__(16) P2WaveLds {
  uint64_t cbuf[P2_CBUF]; // candidates not yet published to the query's global list
};

// LDS hand-off between lanes of ONE wave.  A wave's DS instructions execute in issue order, so wavefront-scope fences --
// ordering for the compiler -- are enough; the workgroup-scope form (wave_lds_fence) would also wait for every global load
// and store still in flight, here the blocks requested ahead and the candidates just written
__device__ __forceinline__ void p2_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// v of lane l (0 .. 63), l a per-lane value; the source lane must be active
__device__ __forceinline__ uint32_t lane_read(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(l << 2), (int)v); }

} // namespace

__global__ __launch_bounds__(WG, 8) void scan_p2_kernel(ScanArgs a) {
  __shared__ P2WaveLds lds[WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (blockIdx.x >= a.n_items) return;
  const DevItem item = a.items[blockIdx.x];
  const DevQuery* __restrict__ Q = a.queries + item.query;
  const uint32_t oq = Q->out_q;
  const uint32_t nterms = Q->n_terms, K = Q->k, ranker = Q->ranker;
  const uint32_t nw = Q->n_weights < 8u ? Q->n_weights : 8u;
  const uint32_t index_weight = Q->index_weight;
  const DevTerm T0 = Q->t[0];
  const DevTerm T1 = Q->t[nterms > 1 ? 1 : 0];
  const uint32_t bin_mode = Q->bin_mode, bin_shift = Q->bin_shift;
  const int32_t bin_lo = Q->bin_lo;
  const uint32_t cand_cap = Q->cand_cap;
  uint64_t* __restrict__ cand = a.cand + Q->cand_off;
  uint32_t* __restrict__ ghist = a.q_hist + (uint64_t)oq * NBINS;
  uint32_t* __restrict__ gcount = a.q_cand_n + (size_t)oq * QSTRIDE;
  uint32_t* __restrict__ gtaubin = a.q_tau_bin + (size_t)oq * QSTRIDE;
  const uint32_t nb = item.blk_end - item.blk_begin;
  const uint32_t per = (nb + WAVES - 1) / WAVES;
  const uint32_t wb0 = item.blk_begin + wave * per;
  const uint32_t wb1 = wb0 + per < item.blk_end ? wb0 + per : item.blk_end;
  P2WaveLds& L = lds[wave];

  // the wave's first requests, side by side: the query's overflow flag, the threshold the earlier waves reached (items of
  // one block per wave are too short to learn it on the way), the driver keyword's block index
  const uint32_t qf = __hip_atomic_load(a.q_flags + oq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t tau_bin = __hip_atomic_load(gtaubin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  PkChunk c0, cj;
  c0.first = NOBLK;
  if (wb0 < wb1) load_pk_chunk(c0, a.seg, T0, wb0);
  // a query that already overflowed is rerun alone by the host whatever else this launch finds for it
  if (qf & QF_OVERFLOW) return;
  if (wb0 >= wb1) return; // (the waves never meet: no table, no barrier)

  // field-weight sum of a mask (ExtRanker_WeightSum_c, sphinxsearch.cpp:1112-1129); the empty mask: "just fake it" (:1114-1118)
  int32_t fw[8];
#pragma unroll
  for (uint32_t f = 0; f < 8; ++f) fw[f] = f < nw ? Q->weights[f] : 0;
  auto rank_of = [&](uint32_t m) -> uint32_t {
    uint32_t rk = 0;
#pragma unroll
    for (uint32_t f = 0; f < 8; ++f)
      if (m & (1u << f)) rk += (uint32_t)fw[f];
    return m ? rk : 1u;
  };

  uint32_t total = 0, cn = 0, flush_at = 64;
  cj.first = NOBLK;
  uint32_t kj = 0;
  uint32_t gt_new = 0;

  // publish the wave's buffered candidates: reserve a slice of the query's list with ONE atomic, write it coalesced, add
  // the keys' bins to the query's histogram; `more`: the wave goes on, so it takes the shared threshold along
  auto publish = [&](bool more) {
    if (cn) {
      uint32_t basep = 0;
      if (lane == 0) basep = atomicAdd(gcount, cn);
      basep = rdlane(basep, 0);
      const bool fits = basep + cn <= cand_cap;
      const uint32_t npub = cn;
      p2_lds_fence();
      if (fits)
        for (uint32_t i = lane; i < cn; i += 64) cand[basep + i] = L.cbuf[i];
      else if (lane == 0)
        atomicOr(a.q_flags + oq, QF_OVERFLOW);
      hist_add_keys(ghist, L.cbuf, cn, bin_mode, bin_lo, bin_shift);
      p2_lds_fence();
      cn = 0;
      // recomputing the threshold reads the whole (hot) histogram: only the publisher whose slice crosses a 2048-candidate
      // boundary of the query's list does it, and shares the result
      if ((basep >> 11) != ((basep + npub) >> 11) || basep == 0) {
        const uint32_t tb = threshold_bin(ghist, K);
        if (tb > tau_bin) {
          tau_bin = tb;
          if (lane == 0) atomicMax(gtaubin, tb);
        }
      }
    }
    if (more) {
      const uint32_t gt = __hip_atomic_load(gtaubin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (gt > tau_bin) tau_bin = gt;
    }
  };

  const uint32_t rowid_base = a.seg.rowid_base;
  // one match: weight, pruning bin, candidate buffer (all lanes call it; is_live = this lane holds a match)
  auto emit_match = [&](bool is_live, uint32_t rowid, float tfidf, uint32_t fields) {
    bool push = false;
    uint64_t key = 0;
    if (is_live) {
      uint32_t weight;
      if (ranker == MRK_RANK_NONE)
        weight = 1u; // ExtRanker_None_c, sphinxsearch.cpp:1160
      else if (ranker == MRK_RANK_PROXIMITY)
        weight = rank_of(fields); // single keyword: ExtRanker_WeightSum_c<> without BM25 (sphinxsearch.cpp:4216-4217, 1131)
      else {
        // ExtRanker_WeightSum_c<BM25>, sphinxsearch.cpp:1070, 1112-1129
        const int32_t bm = (int32_t)((tfidf + 0.5f) * 1000.0f);
        weight = (uint32_t)bm + rank_of(fields) * 1000u;
      }
      weight *= index_weight; // MatchExtended, sphinx.cpp:12220
      ++total;
      const uint32_t grow = rowid_base + rowid;
      if (bin_of(bin_mode, bin_lo, bin_shift, (int32_t)weight, grow) >= tau_bin) {
        push = true;
        key = make_key((int32_t)weight, grow);
      }
    }
    const uint64_t bal = __ballot(push);
    if (bal) {
      const uint32_t n = (uint32_t)__popcll(bal);
      if (cn + n > (uint32_t)P2_CBUF) publish(true); // keys pushed under the older threshold stay valid candidates
      if (push) L.cbuf[cn + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = key;
      cn += n;
      if (cn >= flush_at) {
        publish(true);
        flush_at = P2_CBUF - 64;
      }
    }
  };

  for (uint32_t b = wb0; b < wb1; ++b) {
    // ---- driver block b.  One block per request on either keyword: requesting the next one ahead (the generic kernel's bursts)
    // measured no faster on the selective launches and costs the registers the eighth wave needs
    if (b < c0.first || b - c0.first >= (uint32_t)CHUNK) load_pk_chunk(c0, a.seg, T0, b);
    const PkRaw cur0 = issue_pk(a.seg, T0, c0, b - c0.first);
    const uint32_t w0 = rdlane(c0.w, b - c0.first), bp0 = rdlane(c0.bp1, b - c0.first);
    const uint32_t left0 = T0.docs - b * DEVBLK;
    uint32_t row[2], off0[2];
    bool ok[2];
    decode_pk(cur0, w0, bp0, left0 < (uint32_t)DEVBLK ? left0 : (uint32_t)DEVBLK, row[0], row[1], off0[0], off0[1], ok[0], ok[1]);

    uint32_t fld[2];
    float acc[2];
    bool live[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const uint32_t tf = (cur0.attr >> (8 * r)) & 0xffu;
      fld[r] = ((cur0.attr >> (16 + 8 * r)) & 0xffu) & T0.queried32; // FitsFields
      live[r] = ok[r] && fld[r] != 0;
      float t = term_tfidf(tf, T0.idf);
      if (tf == 255u && live[r]) t = term_tfidf(exc_tf(a.seg, T0, row[r]), T0.idf);
      acc[r] = 0.0f + t;
    }

    // ---- the second keyword
    if (nterms > 1 && __ballot(live[0] || live[1])) {
      const DevTerm& Tj = T1;
      bool done[2] = {!live[0], !live[1]};
      bool hit[2] = {false, false};
      if (Tj.bm_off != ~0ull) {
        // Dense keyword: test each waiting doc's bit in the keyword's doc-set bitmap; a set bit's RANK (directory count of
        // the 256-rowid group + popcounts inside it) is the doc's slot in the keyword's packed arrays (block = rank >> 7,
        // slot = rank & 127).  Only a doc whose bit is set asks for the directory word and the tf / field word.
        const uint32_t* __restrict__ bmj = a.seg.bm + Tj.bm_off;
        const uint32_t* __restrict__ dirj = a.seg.bm_dir + Tj.dir_off;
        const uint32_t row_end = a.seg.n_windows * 2048u;
        uint4 g0[2], g1[2];
        bool inb[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          inb[r] = !done[r] && row[r] < row_end;
          g0[r] = g1[r] = make_uint4(0u, 0u, 0u, 0u);
          if (inb[r]) {
            const uint4* __restrict__ gp = reinterpret_cast<const uint4*>(bmj + (uint64_t)(row[r] >> 8) * 8);
            g0[r] = gp[0];
            g1[r] = gp[1];
          }
        }
        uint32_t rk[2];
        bool present[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const uint32_t wi = (row[r] >> 5) & 7u, bit = row[r] & 31u;
          const uint32_t w[8] = {g0[r].x, g0[r].y, g0[r].z, g0[r].w, g1[r].x, g1[r].y, g1[r].z, g1[r].w};
          uint32_t word = w[0], cnt = 0;
#pragma unroll
          for (uint32_t i = 0; i < 7; ++i) {
            if (i < wi) cnt += (uint32_t)__popc(w[i]);
            if (i + 1 == wi) word = w[i + 1];
          }
          present[r] = inb[r] && ((word >> bit) & 1u);
          rk[r] = cnt + (uint32_t)__popc(word & ((1u << bit) - 1u));
        }
        uint32_t db[2] = {0u, 0u};
#pragma unroll
        for (int r = 0; r < 2; ++r)
          if (present[r]) db[r] = dirj[row[r] >> 8];
        uint32_t aw[2] = {0u, 0u};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          rk[r] += db[r];
          if (present[r]) aw[r] = a.seg.pk_attr[(uint64_t)(Tj.blk_first + (rk[r] >> 7)) * 64 + (rk[r] & 63u)];
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const uint32_t sh = ((rk[r] >> 6) & 1u) * 8u;
          const uint32_t tfq = (aw[r] >> sh) & 0xffu;
          const uint32_t fq = ((aw[r] >> (16u + sh)) & 0xffu) & Tj.queried32;
          if (present[r] && fq != 0) {
            hit[r] = true;
            const float tvx = term_tfidf(tfq == 255u ? exc_tf(a.seg, Tj, row[r]) : tfq, Tj.idf);
            acc[r] = acc[r] + tvx;
            fld[r] |= fq;
          }
        }
      } else {
        // Sparse keyword: every waiting doc finds its OWN block in the register chunk and its slot in that block by a lower
        // bound straight over the packed words (pk_doc_off: any slot of any block can be read on its own) -- the depth of the
        // chain is the same whether the driver block's docs fall into one block of this keyword or into sixty.
        // The shared threshold word rides along once per driver block.
        gt_new = __hip_atomic_load(gtaubin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (;;) {
          // smallest driver rowid still waiting for this keyword (docs are in rowid order lane by lane)
          const uint64_t p0 = __ballot(!done[0]), p1 = __ballot(!done[1]);
          if (!(p0 | p1)) break;
          const uint32_t r_min = p0 ? rdlane(row[0], (uint32_t)__builtin_ctzll(p0)) : rdlane(row[1], (uint32_t)__builtin_ctzll(p1));
          // its block: the last one whose base <= r_min (HintRowID's FindSpan), never behind the cursor
          if (cj.first == NOBLK || kj < cj.first || kj - cj.first >= (uint32_t)CHUNK) load_pk_chunk(cj, a.seg, Tj, kj);
          {
            const uint64_t le = __ballot(cj.bp1 <= r_min);
            const uint32_t p = le ? 63u - (uint32_t)__builtin_clzll(le) : 0u;
            if (p >= (uint32_t)CHUNK) { // beyond this chunk: wave-wide 64-ary search, then reload
              kj = wave_find_block(a.seg.pk_base + Tj.blk_first, cj.first + CHUNK - 1, Tj.nblocks, r_min);
              load_pk_chunk(cj, a.seg, Tj, kj);
            } else if (cj.first + p > kj)
              kj = cj.first + p;
          }
          // own block: p = the chunk's last entry with bp1 <= row, six fixed steps over the chunk's registers (the loop is
          // wave-uniform: every source lane is active).  Entry 63 only bounds block 62: a doc with p == 63 waits for the next
          // pass, whose chunk starts at or behind its block.
          uint32_t p[2] = {0u, 0u}, bp[2];
          bp[0] = bp[1] = rdlane(cj.bp1, 0);
#pragma unroll
          for (uint32_t step = 32; step; step >>= 1) {
            uint32_t v[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) v[r] = lane_read(cj.bp1, p[r] + step);
#pragma unroll
            for (int r = 0; r < 2; ++r)
              if (v[r] <= row[r]) p[r] += step, bp[r] = v[r];
          }
          bool act[2];
          uint32_t wj[2], want[2], ndj[2], pos[2] = {0u, 0u};
          const uint32_t* __restrict__ dp[2];
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            wj[r] = lane_read(cj.w, p[r]);
            dp[r] = a.seg.pk_delta + lane_read(cj.doff, p[r]);
            const bool here = !done[r] && p[r] < (uint32_t)CHUNK;
            done[r] = done[r] || here;
            act[r] = here && row[r] >= bp[r]; // (a row below the chunk's first block cannot happen: the cursor only moves forward)
            want[r] = row[r] - bp[r];
            const uint32_t leftj = Tj.docs - (cj.first + p[r]) * DEVBLK;
            ndj[r] = act[r] ? (leftj < (uint32_t)DEVBLK ? leftj : (uint32_t)DEVBLK) : 0u;
          }
          // slot in the block: both docs of a lane go through the dependent reads side by side
#pragma unroll
          for (uint32_t step = DEVBLK / 2; step; step >>= 1) {
            uint32_t o[2] = {0u, 0u};
#pragma unroll
            for (int r = 0; r < 2; ++r)
              if (act[r]) o[r] = pk_doc_off(dp[r], wj[r], pos[r] + step - 1);
#pragma unroll
            for (int r = 0; r < 2; ++r)
              if (pk_doc_below(o[r], pos[r] + step - 1, ndj[r], want[r])) pos[r] += step;
          }
          uint32_t fo[2] = {0u, 0u}, aw[2] = {0u, 0u};
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            act[r] = act[r] && pos[r] < ndj[r];
            if (act[r]) {
              fo[r] = pk_doc_off(dp[r], wj[r], pos[r]);
              aw[r] = a.seg.pk_attr[(uint64_t)(Tj.blk_first + cj.first + p[r]) * 64 + (pos[r] & 63u)];
            }
          }
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const uint32_t sh = (pos[r] >> 6) * 8;
            const uint32_t tfj = (aw[r] >> sh) & 0xffu;
            const uint32_t fj = (aw[r] >> (16 + sh)) & 0xffu & Tj.queried32;
            if (act[r] && fo[r] == want[r] && fj != 0) {
              hit[r] = true;
              const float tvx = term_tfidf(tfj == 255u ? exc_tf(a.seg, Tj, row[r]) : tfj, Tj.idf);
              acc[r] = acc[r] + tvx;
              fld[r] |= fj;
            }
          }
        }
      }
      live[0] = live[0] && hit[0];
      live[1] = live[1] && hit[1];
    }

    if (gt_new > tau_bin) tau_bin = gt_new;
    if (a.seg.dead) { // MatchExtended drops dead rows before they reach the sorter (sphinx.cpp:12213-12217)
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (live[r] && row_is_dead(a.seg, row[r])) live[r] = false;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) emit_match(live[r], row[r], acc[r], fld[r]);
  }

  // ---- wave epilogue
  if (cn) publish(false);
  {
    uint32_t t = total;
    for (int dlt = 32; dlt; dlt >>= 1) t += __shfl_down(t, dlt, 64);
    if (lane == 0 && t) atomicAdd((unsigned long long*)(a.q_total + oq), (unsigned long long)t);
  }
}

void launch_scan_p2(const ScanArgs& a, void* stream) {
  if (!a.n_items) return;
  hipLaunchKernelGGL(scan_p2_kernel, dim3(a.n_items), dim3(WG), 0, (hipStream_t)stream, a);
}

} // namespace mrk
