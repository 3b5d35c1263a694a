// mrk_groupsel.hip -- the groups of the GROUPED queries (mrk_group: CSphKBufferGroupSorter::FinalizeMatches / Flatten,
// sphinxsort.cpp:3233-3300, over a sorter that never had to cut), gfx950 / wave64.
//
// The scan and rank kernels left one slot per distinct group value in the query's table (mrk_kgroup.h): the value, the head --
// the largest make_key(weight, global rowid) among the group's matches -- and the count.  One workgroup per grouped query:
//   - more claimed slots than 4 k (GROUPBY_FACTOR), or a probe that found the table full (QF_GROUPS): the reference would have cut
//     groups by now and its answer would depend on the arrival order.  The query gets QF_GROUPS and no rows; the row writers and
//     mrk_batch_wait make MRK_ROW_DECLINED / MRK_E_UNSUPPORTED of it;
//   - else the occupied slots (<= 4096) are compacted into LDS with their order key -- the part the query sorts its groups by, in
//     its direction, over ~head rowid (group_order_key) -- and sorted descending, bitonic as in mrk_sortsel.hip.  The best k leave:
//     head key, group value, count; q_total = the number of groups.
// 4096 x (8-byte key + 4-byte slot index) = 48 KB of the 64 KB static LDS.  Slots are compacted in whatever order the atomics fall;
// the order keys are distinct (heads are distinct rows), so the sorted result is the same from run to run.
#include "mrk_kcommon.h"
#include "mrk_kgroup.h"

namespace mrk {

struct __align__(16) GroupSelSmem {
  uint64_t key[GRP_MAX_GROUPS];
  uint32_t idx[GRP_MAX_GROUPS];
  uint32_t n;
};

__global__ __launch_bounds__(WG) void group_select_kernel(GroupSelArgs a) {
  __shared__ GroupSelSmem s;
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  if (q >= a.n_queries) return;
  const DevQuery* __restrict__ Q = a.queries + q;
  if (!Q->grp_on) return; // (uniform: another selection answered this query)
  const uint32_t K = Q->k ? (Q->k < (uint32_t)KCAP ? Q->k : (uint32_t)KCAP) : 1u;
  const uint32_t S = Q->grp_slots;
  const GroupTable T = group_table_at(a.gtab + Q->grp_off, S);
  const uint32_t claimed = *T.claimed, qf = a.q_flags[q];
  if (tid == 0) s.n = 0;
  if (qf & QF_OVERFLOW) { // its match queue was full: mrk_batch_wait reruns the query alone, over a cleared table
    if (tid == 0) {
      a.out_cnt[q] = 0;
      if (a.h_cnt) a.h_cnt[q] = 0;
    }
    return;
  }
  if (claimed > group_limit(K) || claimed > GRP_MAX_GROUPS || (qf & QF_GROUPS)) {
    if (tid == 0) {
      a.q_flags[q] = qf | QF_GROUPS;
      a.out_cnt[q] = 0;
      if (a.h_flags) a.h_flags[q] = qf | QF_GROUPS;
      if (a.h_cnt) a.h_cnt[q] = 0;
    }
    return;
  }
  __syncthreads();
  const uint32_t sort_by = Q->grp_sort_by, desc = Q->grp_desc;
  for (uint32_t i = tid; i < S; i += WG) {
    const uint64_t kw = T.keys[i];
    if (kw) {
      const uint32_t at = atomicAdd(&s.n, 1u); // (< claimed <= GRP_MAX_GROUPS: a slot is counted once)
      if (at < GRP_MAX_GROUPS) {
        s.key[at] = group_order_key(sort_by, desc, (uint32_t)kw, T.counts[i], T.heads[i]);
        s.idx[at] = i;
      }
    }
  }
  __syncthreads();
  const uint32_t n = s.n < GRP_MAX_GROUPS ? s.n : GRP_MAX_GROUPS;
  uint32_t len = 64;
  while (len < n) len <<= 1;
  for (uint32_t i = n + tid; i < len; i += WG) s.key[i] = 0, s.idx[i] = 0xFFFFFFFFu; // (padding loses every tie: a real entry may have key 0)
  __syncthreads();
  for (uint32_t k = 2; k <= len; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < len / 2; t += WG) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const bool down = (i & k) == 0;
        const uint64_t ak = s.key[i], bk = s.key[p];
        const uint32_t ai = s.idx[i], bi = s.idx[p];
        const bool b_gt = bk > ak || (bk == ak && bi < ai);
        if (b_gt == down) s.key[i] = bk, s.idx[i] = bi, s.key[p] = ak, s.idx[p] = ai;
      }
      __syncthreads();
    }
  const uint32_t m = n < K ? n : K;
  for (uint32_t i = tid; i < m; i += WG) {
    const uint32_t slot = s.idx[i];
    const uint64_t head = T.heads[slot];
    const uint32_t value = (uint32_t)T.keys[slot], count = T.counts[slot];
    const uint64_t o = (uint64_t)q * KCAP + i;
    a.out_keys[o] = head, a.out_gkey[o] = value, a.out_gcnt[o] = count;
    if (a.h_keys) a.h_keys[o] = head;
    if (a.h_gkey) a.h_gkey[o] = value, a.h_gcnt[o] = count;
  }
  if (tid == 0) {
    a.out_cnt[q] = m;
    a.q_total[q] = n; // total_found = the number of groups (++m_iTotal on a new group only)
    if (a.h_cnt) a.h_cnt[q] = m;
    if (a.h_total) a.h_total[q] = n;
  }
}

void launch_group_select(const GroupSelArgs& a, void* stream) {
  if (!a.n_queries) return;
  hipLaunchKernelGGL(group_select_kernel, dim3(a.n_queries), dim3(WG), 0, (hipStream_t)stream, a);
}

} // namespace mrk
