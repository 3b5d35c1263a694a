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
// A query with aggregates (mrk_aggrs) may order its groups by an aggregate's 32-bit value in the place of that part, and the best k
// rows' aggregates leave next to them, the accumulators' mapping undone.
// 4096 x (8-byte key + 4-byte slot index) = 48 KB of the 64 KB static LDS.  Slots are compacted in whatever order the atomics fall;
// the order keys of a row attribute's groups are distinct (heads are distinct rows), and equal keys -- groups of a multi-value
// attribute that one doc heads -- leave by the smaller group value (group_sort_desc), so the sorted result is the same from run to run.
// The same compaction and sort (group_compact_sort) serve the GROUP rows further down: pack_grows_kernel writes all the groups of a
// query's table as its exchange row, merge_grows_kernel adds up to 8 such rows into one table and writes the merged row.
// The AGGREGATE rows behind them carry a query's aggregates too: pack_arows_kernel writes the groups with their aggregates' values,
// merge_arows_kernel adds / max-es the lists' values per group through the accumulators' own update -- kernels of their own, so that
// the three above compile to what they compiled to.
#include "mrk_kcommon.h"
#include "mrk_kgroup.h"
#include "mrk_krows.h"

namespace mrk {

struct __align__(16) GroupSelSmem {
  uint64_t key[GRP_MAX_GROUPS];
  uint32_t idx[GRP_MAX_GROUPS];
  uint32_t n;
};

// s.key / s.idx [0, n), n <= GRP_MAX_GROUPS, sorted by the whole workgroup: key descending; among equal keys the SMALLER GROUP VALUE
// first, read from tkeys[idx] (the table's key plane) on that rare branch; padding last.  Equal keys of real entries occur only
// between groups of a multi-value attribute that one doc heads (include/mrk.h, mrk_group_mva): the reference leaves their order
// open, and the table slot -- which depends on the hash and on who won a claim -- must not decide it.  tkeys == NULL (the narrow
// merge of relevance keys, whose idx are all 0): equal keys stay in either order, they are the same word.  The entries are written
// and the workgroup in step when it is called; it ends behind a barrier.
__device__ __forceinline__ void group_sort_desc(GroupSelSmem& s, uint32_t n, const uint64_t* __restrict__ tkeys = nullptr) {
  const uint32_t tid = threadIdx.x;
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
        bool b_gt = bk > ak;
        if (bk == ak) // (padding's idx is the largest: it loses to every real entry, whose values are read only when both are real)
          b_gt = tkeys && ai != 0xFFFFFFFFu && bi != 0xFFFFFFFFu ? (uint32_t)tkeys[bi] < (uint32_t)tkeys[ai] : bi < ai;
        if (b_gt == down) s.key[i] = bk, s.idx[i] = bi, s.key[p] = ak, s.idx[p] = ai;
      }
      __syncthreads();
    }
}

// The occupied slots of T (the caller checked: at most GRP_MAX_GROUPS claimed) compacted into s with their order key and sorted, best
// group first: s.idx[0 .. n) are the groups' slots in group order.  The one compact-and-sort of group_select_kernel, pack_grows_kernel
// and merge_grows_kernel; by the whole workgroup, which reads T with plain loads (a kernel that filled T itself fences first).
// order_aggr: 1 + the aggregate whose 32-bit value orders the groups in the place of sort_by (its op word: aggr_op), 0 = none.
__device__ __forceinline__ uint32_t group_compact_sort(GroupSelSmem& s, const GroupTable& T, uint32_t sort_by, uint32_t desc, uint32_t order_aggr = 0u, uint32_t aggr_op = 0u) {
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s.n = 0;
  __syncthreads();
  for (uint32_t i = tid; i < T.slots; i += WG) {
    const uint64_t kw = T.keys[i];
    if (kw) {
      const uint32_t at = atomicAdd(&s.n, 1u); // (< claimed <= GRP_MAX_GROUPS: a slot is counted once)
      if (at < GRP_MAX_GROUPS) {
        s.key[at] = order_aggr ? group_order_key_aggr(desc, (uint32_t)aggr_unmap(aggr_op, T.aggr[(uint64_t)(order_aggr - 1u) * T.slots + i]), T.heads[i])
                               : group_order_key(sort_by, desc, (uint32_t)kw, T.counts[i], T.heads[i]);
        s.idx[at] = i;
      }
    }
  }
  __syncthreads();
  const uint32_t n = s.n < GRP_MAX_GROUPS ? s.n : GRP_MAX_GROUPS;
  group_sort_desc(s, n, T.keys);
  return n;
}

// ---- a group row (MRK_GROW_WORDS), by the whole workgroup: n entries, entry i = key_at(i) over plane_at(i), zero past n.  SPEC_AT:
// where the layout keeps the group spec word (an aggregate row shares the words in front of it)
template <int SPEC_AT = GROW_SPEC, class KF, class PF>
__device__ __forceinline__ void write_grow(uint64_t* __restrict__ row, uint32_t n, KF key_at, PF plane_at, uint64_t total_word, uint64_t spec) {
  for (uint32_t i = threadIdx.x; i < (uint32_t)GROW_GROUPS; i += WG) {
    row[i] = i < n ? key_at(i) : 0ull;
    row[GROW_PLANE + i] = i < n ? plane_at(i) : 0ull;
  }
  if (threadIdx.x == 0) row[GROW_CNT] = n, row[GROW_TOTAL] = total_word, row[SPEC_AT] = spec;
}
// ... all the groups of T, s.idx[0 .. n) their slots in group order (group_compact_sort)
template <int SPEC_AT = GROW_SPEC>
__device__ __forceinline__ void write_grow_groups(uint64_t* __restrict__ row, uint32_t n, const GroupSelSmem& s, const GroupTable& T, uint64_t total_word, uint64_t spec) {
  write_grow<SPEC_AT>(
      row, n, [&](uint32_t i) { return T.heads[s.idx[i]]; }, [&](uint32_t i) { return group_plane_word((uint32_t)T.keys[s.idx[i]], T.counts[s.idx[i]]); }, total_word, spec);
}
// ---- what an aggregate row (MRK_AROW_WORDS) holds behind a group row's words: the MRK_MAX_AGGRS planes -- aggregate a of entry i =
// the VALUE of T's accumulator (aggr_unmap under op_of(a)) for a < n_aggr and i < n, zero elsewhere -- and the aggregate spec word.
// Every word is written.  T.aggr is read only where a < n_aggr: the table holds no more planes.
template <class OF>
__device__ __forceinline__ void write_arow_planes(uint64_t* __restrict__ row, uint32_t n, uint32_t n_aggr, const GroupSelSmem& s, const GroupTable& T, OF op_of, uint64_t aspec) {
  for (uint32_t a = 0; a < (uint32_t)MRK_MAX_AGGRS; ++a) { // (uniform)
    uint64_t* __restrict__ plane = row + AROW_AGGR + a * (uint32_t)GROW_GROUPS;
    if (a < n_aggr) {
      const uint32_t op = op_of(a);
      const uint64_t* __restrict__ acc = T.aggr + (uint64_t)a * T.slots;
      for (uint32_t i = threadIdx.x; i < (uint32_t)GROW_GROUPS; i += WG) plane[i] = i < n ? aggr_unmap(op, acc[s.idx[i]]) : 0ull;
    } else
      for (uint32_t i = threadIdx.x; i < (uint32_t)GROW_GROUPS; i += WG) plane[i] = 0ull;
  }
  if (threadIdx.x == 0) row[AROW_ASPEC] = aspec;
}

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
  const uint32_t n_aggr = a.out_aggr ? (Q->grp_naggr < (uint32_t)MRK_MAX_AGGRS ? Q->grp_naggr : (uint32_t)MRK_MAX_AGGRS) : 0u; // (uniform)
  const uint32_t ord = n_aggr && Q->grp_order_aggr <= n_aggr ? Q->grp_order_aggr : 0u;
  const uint32_t n = group_compact_sort(s, T, Q->grp_sort_by, Q->grp_desc, ord, ord ? Q->grp_aggr_op[ord - 1u] : 0u);
  const uint32_t m = n < K ? n : K;
  for (uint32_t i = tid; i < m; i += WG) {
    const uint32_t slot = s.idx[i];
    const uint64_t head = T.heads[slot];
    const uint32_t value = (uint32_t)T.keys[slot], count = T.counts[slot];
    const uint64_t o = (uint64_t)q * KCAP + i;
    a.out_keys[o] = head, a.out_gkey[o] = value, a.out_gcnt[o] = count;
    if (a.h_keys) a.h_keys[o] = head;
    if (a.h_gkey) a.h_gkey[o] = value, a.h_gcnt[o] = count;
    for (uint32_t ai = 0; ai < n_aggr; ++ai) { // the accumulators' mapping undone (aggr_unmap): the aggregates' values, row-major
      const uint64_t v = aggr_unmap(Q->grp_aggr_op[ai], T.aggr[(uint64_t)ai * S + slot]);
      a.out_aggr[o * MRK_MAX_AGGRS + ai] = v;
      if (a.h_aggr) a.h_aggr[o * MRK_MAX_AGGRS + ai] = v;
    }
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

// ---------------------------------------------------------------------------------------
// a batch's results as group rows (mrk_batch_export_grows, behind the batch's selection): one workgroup per query.  A grouped query
// leaves with ALL the groups of its table -- group_select_kernel's compaction and sort, every entry written instead of the best k;
// a relevance query with its keys over a zero plane and spec 0; a sorted or ordered one, and whatever the planner declined, with
// MRK_ROW_DECLINED.  A grouped query the scan flagged leaves empty under its own spec word: MRK_ROW_RERUN is an answering list to
// the merge and takes part in the election of the spec.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void pack_grows_kernel(PackGRowsArgs a) {
  __shared__ GroupSelSmem s;
  const uint32_t q = blockIdx.x;
  if (q >= a.n) return;
  const DevQuery* __restrict__ Q = a.queries + q;
  const bool declined = a.declined && ((a.declined[q] >> ROWS_GROUP) & 1u) != 0u;
  const uint32_t qf = a.flags ? a.flags[q] : 0u;
  uint64_t* __restrict__ row = a.rows + (uint64_t)q * GROW_WORDS;
  auto zero = [](uint32_t) { return 0ull; };
  if (!declined && Q->grp_on && a.gtab) { // (uniform)
    const uint32_t K = Q->k ? (Q->k < (uint32_t)KCAP ? Q->k : (uint32_t)KCAP) : 1u;
    const uint64_t spec = group_spec_word(Q->grp_sort_by, Q->grp_desc, Q->grp_bits, K);
    const GroupTable T = group_table_at(const_cast<uint64_t*>(a.gtab) + Q->grp_off, Q->grp_slots);
    const uint32_t claimed = *T.claimed;
    const uint32_t over = claimed > group_limit(K) || claimed > GRP_MAX_GROUPS ? QF_GROUPS : 0u; // (group_select_kernel set it already)
    if (!row_unflagged(false, qf | over)) {
      write_grow(row, 0u, zero, zero, row_total_word(false, qf | over, 0ull), spec);
      return;
    }
    const uint32_t n = group_compact_sort(s, T, Q->grp_sort_by, Q->grp_desc);
    write_grow_groups(row, n, s, T, n, spec); // total_found = the number of groups
    return;
  }
  const uint32_t n = !row_unflagged(declined, qf) ? 0u : a.cnt[q] < (uint32_t)KCAP ? a.cnt[q] : (uint32_t)KCAP;
  write_grow(
      row, n, [&](uint32_t i) { return a.keys[(uint64_t)q * KCAP + i]; }, zero, row_total_word(declined, qf, a.total[q]), 0ull);
}

void launch_pack_grows(const PackGRowsArgs& a, void* stream) {
  if (!a.n) return;
  hipLaunchKernelGGL(pack_grows_kernel, dim3(a.n), dim3(WG), 0, (hipStream_t)stream, a);
}

// ---------------------------------------------------------------------------------------
// a batch's results as AGGREGATE rows (mrk_batch_export_arows): pack_grows_kernel's cases under the decline bit ROWS_AGGR, which a
// query's aggregates do not set.  A grouped query leaves with all its groups in the QUERY's group order -- by its ordering aggregate
// where it has one -- and, behind the group row's words, its aggregates' values; one without aggregates with zero planes and
// aggregate spec 0; a relevance query as in group rows.  The table is the batch's, laid out with the query's grp_naggr planes.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void pack_arows_kernel(PackGRowsArgs a) {
  __shared__ GroupSelSmem s;
  const uint32_t q = blockIdx.x;
  if (q >= a.n) return;
  const DevQuery* __restrict__ Q = a.queries + q;
  const bool declined = a.declined && ((a.declined[q] >> ROWS_AGGR) & 1u) != 0u;
  const uint32_t qf = a.flags ? a.flags[q] : 0u;
  uint64_t* __restrict__ row = a.rows + (uint64_t)q * AROW_WORDS;
  const GroupTable none{};
  auto zero = [](uint32_t) { return 0ull; };
  auto no_op = [](uint32_t) { return 0u; };
  if (!declined && Q->grp_on && a.gtab) { // (uniform)
    const uint32_t K = Q->k ? (Q->k < (uint32_t)KCAP ? Q->k : (uint32_t)KCAP) : 1u;
    const uint64_t spec = group_spec_word(Q->grp_sort_by, Q->grp_desc, Q->grp_bits, K);
    const uint32_t n_aggr = Q->grp_naggr < (uint32_t)MRK_MAX_AGGRS ? Q->grp_naggr : (uint32_t)MRK_MAX_AGGRS;
    const uint32_t ord = n_aggr && Q->grp_order_aggr <= n_aggr ? Q->grp_order_aggr : 0u;
    const uint64_t aspec = n_aggr ? aggr_spec_word(n_aggr, ord, Q->grp_aggr_op) : 0ull;
    const GroupTable T = group_table_at(const_cast<uint64_t*>(a.gtab) + Q->grp_off, Q->grp_slots);
    const uint32_t claimed = *T.claimed;
    const uint32_t over = claimed > group_limit(K) || claimed > GRP_MAX_GROUPS ? QF_GROUPS : 0u; // (group_select_kernel set it already)
    if (!row_unflagged(false, qf | over)) {
      write_grow<AROW_GSPEC>(row, 0u, zero, zero, row_total_word(false, qf | over, 0ull), spec);
      write_arow_planes(row, 0u, 0u, s, none, no_op, aspec);
      return;
    }
    const uint32_t n = group_compact_sort(s, T, Q->grp_sort_by, Q->grp_desc, ord, ord ? Q->grp_aggr_op[ord - 1u] : 0u);
    write_grow_groups<AROW_GSPEC>(row, n, s, T, n, spec); // total_found = the number of groups
    write_arow_planes(
        row, n, n_aggr, s, T, [&](uint32_t ai) { return Q->grp_aggr_op[ai]; }, aspec);
    return;
  }
  const uint32_t n = !row_unflagged(declined, qf) ? 0u : a.cnt[q] < (uint32_t)KCAP ? a.cnt[q] : (uint32_t)KCAP;
  write_grow<AROW_GSPEC>(
      row, n, [&](uint32_t i) { return a.keys[(uint64_t)q * KCAP + i]; }, zero, row_total_word(declined, qf, a.total[q]), 0ull);
  write_arow_planes(row, 0u, 0u, s, none, no_op, 0ull);
}

void launch_pack_arows(const PackGRowsArgs& a, void* stream) {
  if (!a.n) return;
  hipLaunchKernelGGL(pack_arows_kernel, dim3(a.n), dim3(WG), 0, (hipStream_t)stream, a);
}

// ---------------------------------------------------------------------------------------
// merge of <= 8 group rows per query: ONE grouping sorter over the matches of all lists (the reference hands the same sorter to every
// chunk of an index, sphinxrt.cpp:6018-6077 and :6302-6346).  One workgroup per query.
//   spec 0 (a relevance query): the narrow merge of the rows' first ROW_WORDS words -- the lists' keys gathered in the sort area, at
//     most 4 lists of KCAP at a time, sorted, the best KCAP kept for the next round; words [0, KCAP), count and total word come out as
//     merge_xrows_kernel<NarrowFmt> writes them.
//   grouped: every entry of every list goes through group_update into the query's table of the scratch arena (zero at launch; the
//     count is added, the head key max-ed), then the shared compact-and-sort orders the merged groups and all of them leave.
// What makes the merged row MRK_ROW_DECLINED or MRK_ROW_RERUN instead: include/mrk.h.  A count past 2^32 - 1 is found without a
// second pass over the lists: the 64-bit sum of all counts that went in must equal the sum of the table's 32-bit counts, and a slot
// that wrapped is short by 2^32.
// LDS: the 48 KB sort area, the lists' counts and three words.  The table is read back with plain loads behind an agent-scope fence pair.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void merge_grows_kernel(MergeRowsArgs a, uint64_t* gtab, uint64_t tab_words) {
  __shared__ GroupSelSmem s;
  __shared__ unsigned long long sum_in, sum_out;
  // the lists' entry counts go through group_row_head ONCE and wait in LDS for the loops below.  (A first version called the reader
  // again in front of each loop, through an early-return form of it: the entry loop of every grouped list came out of the device
  // compiler with a bound of 0 -- an empty merged row under a good spec word, which the GPU tests caught against the numpy mirror.)
  __shared__ uint32_t full, l_cnt[8];
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  if (q >= a.n_queries) return;
  const uint64_t* __restrict__ rows = a.in_rows + (uint64_t)q * GROW_WORDS;
  const uint64_t list_words = (uint64_t)a.list_stride * GROW_WORDS;
  if (a.n_lists > 8u) return; // (the launch's contract; l_cnt holds 8)
  uint64_t spec = 0, flags = 0, total = 0, have = 0;
  bool have_spec = false, mismatch = false;
  for (uint32_t l = 0; l < a.n_lists; ++l) {
    uint64_t t, sp; // (uniform) the list's total word and spec word; a hostile list reads as declined and empty
    const uint32_t c = group_row_head(rows + l * list_words, t, sp);
    if (tid == 0) l_cnt[l] = c;
    flags |= t & ROW_FLAG_MASK, total += t & ~ROW_FLAG_MASK, have += c < (uint32_t)KCAP ? c : (uint32_t)KCAP;
    if (!group_row_has_say(t, sp)) continue; // (declined without a spec: the merged row does not depend on which list declined)
    if (!have_spec) spec = sp, have_spec = true;
    mismatch = mismatch || sp != spec;
  }
  __syncthreads();
  uint64_t* __restrict__ out = a.out_rows + (uint64_t)(a.out_first + q) * GROW_WORDS;
  auto zero = [](uint32_t) { return 0ull; };
  auto finish = [&](uint64_t f) {
    if (tid == 0 && a.flags_any) {
      if (f & ROW_RERUN) a.flags_any[0] = 1u;
      if (f & ROW_DECLINED) a.flags_any[1] = 1u;
    }
  };
  if (mismatch) flags |= ROW_DECLINED;
  if (spec == 0ull) { // ---- a relevance query: the narrow merge
    uint32_t acc = 0;
    if (!mismatch)
      for (uint32_t l = 0; l < a.n_lists; ++l) {
        uint32_t c = l_cnt[l];
        if (c > (uint32_t)KCAP) c = KCAP;
        if (!c) continue;
        if (acc + c > GRP_MAX_GROUPS) { // the area is full: keep the best KCAP of what it holds
          __syncthreads();
          group_sort_desc(s, acc);
          acc = acc < (uint32_t)KCAP ? acc : (uint32_t)KCAP;
        }
        const uint64_t* __restrict__ row = rows + l * list_words;
        for (uint32_t i = tid; i < c; i += WG) s.key[acc + i] = row[i], s.idx[acc + i] = 0u;
        acc += c;
      }
    __syncthreads();
    group_sort_desc(s, acc);
    const uint32_t n = mismatch ? 0u : have < a.k ? (uint32_t)have : a.k;
    write_grow(
        out, n, [&](uint32_t i) { return s.key[i]; }, zero, (total & ~ROW_FLAG_MASK) | flags, 0ull);
    finish(flags);
    return;
  }
  // ---- a grouped query
  GroupSpec gs;
  (void)group_spec_unpack(spec, gs); // (an answering list's spec word: list_head saw it unpack)
  if (gs.k > a.k) flags |= ROW_DECLINED; // (its table would not fit the arena's stride)
  uint32_t n = 0;
  GroupTable T{};
  if (!flags) { // (uniform)
    T = group_table_at(gtab + (uint64_t)q * tab_words, group_slots_for(gs.k));
    if (tid == 0) sum_in = 0ull, sum_out = 0ull, full = 0u;
    __syncthreads();
    unsigned long long mine = 0;
    bool ok = true;
    for (uint32_t l = 0; l < a.n_lists; ++l) {
      const uint32_t c = l_cnt[l];
      const uint64_t* __restrict__ row = rows + l * list_words;
      for (uint32_t i = tid; i < c; i += WG) {
        const uint64_t pw = row[GROW_PLANE + i];
        ok = group_update<GroupDevOps>(T, (uint32_t)(pw >> 32), (uint32_t)pw, row[i]) && ok;
        mine += (uint32_t)pw;
      }
    }
    if (mine) atomicAdd(&sum_in, mine);
    if (!ok) atomicOr(&full, 1u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t claimed = *T.claimed;
    if (full || claimed > group_limit(gs.k) || claimed > GRP_MAX_GROUPS)
      flags |= ROW_DECLINED; // one sorter over all the lists would have cut groups by now
    else {
      n = group_compact_sort(s, T, gs.sort_by, gs.desc);
      mine = 0;
      for (uint32_t i = tid; i < n; i += WG) mine += T.counts[s.idx[i]];
      if (mine) atomicAdd(&sum_out, mine);
      __syncthreads();
      if (sum_out != sum_in) flags |= ROW_DECLINED, n = 0; // some group's count passed 2^32 - 1
    }
  }
  if (flags)
    write_grow(out, 0u, zero, zero, flags, spec);
  else
    write_grow_groups(out, n, s, T, n, spec);
  finish(flags);
#ifdef MRK_GDBG
  __syncthreads();
  if (tid == 0) out[4090] = sum_in, out[4091] = T.claimed ? *T.claimed : 77u, out[4092] = n, out[4093] = full, out[4094] = T.slots, out[4095] = sum_out, out[4089] = flags, out[4088] = a.n_lists;
#endif
}

void launch_merge_grows(const MergeRowsArgs& a, uint64_t* gtab, uint64_t tab_words, void* stream) {
  if (!a.n_queries) return;
  hipLaunchKernelGGL(merge_grows_kernel, dim3(a.n_queries), dim3(WG), 0, (hipStream_t)stream, a, gtab, tab_words);
}

// ---------------------------------------------------------------------------------------
// merge of <= 8 AGGREGATE rows per query: merge_grows_kernel's steps, in a kernel of its own so that merge_grows_kernel stays the
// code it was.  The lists are read through aggr_row_head; the election is over both spec words (the aggregate spec words of the
// answering lists must be equal in every bit, "without aggregates" included).  Spec 0: the narrow merge, under zero planes.  Grouped:
// every entry claims or finds its slot (group_update_slot) and then, per aggregate, updates the slot's accumulator with the MAPPED
// value (aggr_map under the op word rebuilt from the spec's nibble: a 32-bit MIN maps as ~v over 64 bits and aggr_unmap takes the
// low dword back; a 32-bit SUM is the low dword of the 64-bit one).  The table is the arena's, zero at launch and tab_words apart,
// which leaves room for MRK_MAX_AGGRS planes behind group_slots_for(a.k) slots; the planes go from the rows to the table and from
// the table to the merged row, never through LDS.  The groups leave ordered by the group spec or by the ordering aggregate's merged
// 32-bit value (group_compact_sort).  The count check, the fence pair and the lists' heads read once into LDS: as above.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void merge_arows_kernel(MergeRowsArgs a, uint64_t* gtab, uint64_t tab_words) {
  __shared__ GroupSelSmem s;
  __shared__ unsigned long long sum_in, sum_out;
  __shared__ uint32_t full, l_cnt[8];
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  if (q >= a.n_queries) return;
  const uint64_t* __restrict__ rows = a.in_rows + (uint64_t)q * AROW_WORDS;
  const uint64_t list_words = (uint64_t)a.list_stride * AROW_WORDS;
  if (a.n_lists > 8u) return; // (the launch's contract; l_cnt holds 8)
  uint64_t spec = 0, aspec = 0, flags = 0, total = 0, have = 0;
  bool have_spec = false, mismatch = false;
  for (uint32_t l = 0; l < a.n_lists; ++l) {
    uint64_t t, sp, asp; // (uniform) the list's total word and spec words; a hostile list reads as declined and empty
    const uint32_t c = aggr_row_head(rows + l * list_words, t, sp, asp);
    if (tid == 0) l_cnt[l] = c;
    flags |= t & ROW_FLAG_MASK, total += t & ~ROW_FLAG_MASK, have += c < (uint32_t)KCAP ? c : (uint32_t)KCAP;
    if (!group_row_has_say(t, sp)) continue;
    if (!have_spec) spec = sp, aspec = asp, have_spec = true;
    mismatch = mismatch || sp != spec || asp != aspec;
  }
  __syncthreads();
  uint64_t* __restrict__ out = a.out_rows + (uint64_t)(a.out_first + q) * AROW_WORDS;
  const GroupTable none{};
  auto zero = [](uint32_t) { return 0ull; };
  auto no_op = [](uint32_t) { return 0u; };
  auto finish = [&](uint64_t f) {
    if (tid == 0 && a.flags_any) {
      if (f & ROW_RERUN) a.flags_any[0] = 1u;
      if (f & ROW_DECLINED) a.flags_any[1] = 1u;
    }
  };
  if (mismatch) flags |= ROW_DECLINED;
  if (spec == 0ull) { // ---- a relevance query: the narrow merge (aspec is 0: the reader lets no aggregate spec stand over group spec 0)
    uint32_t acc = 0;
    if (!mismatch)
      for (uint32_t l = 0; l < a.n_lists; ++l) {
        uint32_t c = l_cnt[l];
        if (c > (uint32_t)KCAP) c = KCAP;
        if (!c) continue;
        if (acc + c > GRP_MAX_GROUPS) { // the area is full: keep the best KCAP of what it holds
          __syncthreads();
          group_sort_desc(s, acc);
          acc = acc < (uint32_t)KCAP ? acc : (uint32_t)KCAP;
        }
        const uint64_t* __restrict__ row = rows + l * list_words;
        for (uint32_t i = tid; i < c; i += WG) s.key[acc + i] = row[i], s.idx[acc + i] = 0u;
        acc += c;
      }
    __syncthreads();
    group_sort_desc(s, acc);
    const uint32_t n = mismatch ? 0u : have < a.k ? (uint32_t)have : a.k;
    write_grow<AROW_GSPEC>(
        out, n, [&](uint32_t i) { return s.key[i]; }, zero, (total & ~ROW_FLAG_MASK) | flags, 0ull);
    write_arow_planes(out, 0u, 0u, s, none, no_op, 0ull);
    finish(flags);
    return;
  }
  // ---- a grouped query
  GroupSpec gs;
  AggrSpec as{0u, 0u};
  (void)group_spec_unpack(spec, gs); // (an answering list's spec words: aggr_row_head saw them unpack)
  if (aspec) (void)aggr_spec_unpack(aspec, gs.sort_by, as);
  const uint32_t n_aggr = as.n < (uint32_t)MRK_MAX_AGGRS ? as.n : (uint32_t)MRK_MAX_AGGRS; // (the planes the arena's stride has room for)
  const uint32_t ord = as.order <= n_aggr ? as.order : 0u;
  if (gs.k > a.k) flags |= ROW_DECLINED; // (its table would not fit the arena's stride)
  uint32_t n = 0;
  GroupTable T{};
  if (!flags) { // (uniform)
    T = group_table_at(gtab + (uint64_t)q * tab_words, group_slots_for(gs.k));
    if (tid == 0) sum_in = 0ull, sum_out = 0ull, full = 0u;
    __syncthreads();
    unsigned long long mine = 0;
    bool ok = true;
    for (uint32_t l = 0; l < a.n_lists; ++l) {
      const uint32_t c = l_cnt[l];
      const uint64_t* __restrict__ row = rows + l * list_words;
      for (uint32_t i = tid; i < c; i += WG) {
        const uint64_t pw = row[GROW_PLANE + i];
        const uint32_t slot = group_update_slot<GroupDevOps>(T, (uint32_t)(pw >> 32), (uint32_t)pw, row[i]);
        ok = ok && slot != 0xFFFFFFFFu;
        mine += (uint32_t)pw;
        if (slot != 0xFFFFFFFFu)
          for (uint32_t ai = 0; ai < n_aggr; ++ai) { // (uniform bound)
            const uint32_t op = aggr_spec_op(aspec, ai);
            group_aggr_update<GroupDevOps>(T, slot, ai, op, aggr_map(op, row[AROW_AGGR + ai * (uint32_t)GROW_GROUPS + i]));
          }
      }
    }
    if (mine) atomicAdd(&sum_in, mine);
    if (!ok) atomicOr(&full, 1u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t claimed = *T.claimed;
    if (full || claimed > group_limit(gs.k) || claimed > GRP_MAX_GROUPS)
      flags |= ROW_DECLINED; // one sorter over all the lists would have cut groups by now
    else {
      n = group_compact_sort(s, T, gs.sort_by, gs.desc, ord, ord ? aggr_spec_op(aspec, ord - 1u) : 0u);
      mine = 0;
      for (uint32_t i = tid; i < n; i += WG) mine += T.counts[s.idx[i]];
      if (mine) atomicAdd(&sum_out, mine);
      __syncthreads();
      if (sum_out != sum_in) flags |= ROW_DECLINED, n = 0; // some group's count passed 2^32 - 1
    }
  }
  if (flags) {
    write_grow<AROW_GSPEC>(out, 0u, zero, zero, flags, spec);
    write_arow_planes(out, 0u, 0u, s, none, no_op, aspec);
  } else {
    write_grow_groups<AROW_GSPEC>(out, n, s, T, n, spec);
    write_arow_planes(
        out, n, n_aggr, s, T, [&](uint32_t ai) { return aggr_spec_op(aspec, ai); }, aspec);
  }
  finish(flags);
}

void launch_merge_arows(const MergeRowsArgs& a, uint64_t* gtab, uint64_t tab_words, void* stream) {
  if (!a.n_queries) return;
  hipLaunchKernelGGL(merge_arows_kernel, dim3(a.n_queries), dim3(WG), 0, (hipStream_t)stream, a, gtab, tab_words);
}

} // namespace mrk
