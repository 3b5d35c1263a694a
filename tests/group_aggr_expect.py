"""The expectation of a grouped query WITH aggregates (Query.aggrs): group_expect's model of the grouping sorter, extended by import,
plus per-group numpy aggregates over the same matches -- the oracle's full match set, never anything the library computes.

    source   kind INT   the locator's raw bits, unsigned (1..32 bits inside one dword)
             kind INT64 the aligned 64 (low dword first), signed
    SUM      INT: np.uint32, wrapping modulo 2^32 (AggrSum_t<DWORD>, sphinxsort.cpp:1902-1914, :2623); widened INT and INT64: Python
             integers reduced modulo 2^64 (AggrSum_t<int64_t>, :2624: two's complement)
    MIN/MAX  INT: unsigned (AggrMin_t<DWORD> :2663, AggrMax_t<DWORD> :2674); INT64: signed (:2664, :2675)
    value    uint64: a 32-bit result zero-extended, a 64-bit one the integer's bits
    order    aggr_order >= 0: that aggregate's 32-bit value in the direction Group.desc gives, then the head's rowid ASC -- as @count is
             ordered (MatchGeneric1_fn, :4708-4720); else group_expect's"""
import numpy as np

from group_expect import DECLINED, GROUPSORT_KEY, expected_groups
from sorted_expect import all_matches, raw_of

AGGR_SUM, AGGR_MIN, AGGR_MAX = 1, 2, 3
KIND_INT, KIND_FLOAT, KIND_INT64 = 0, 1, 2
M64 = (1 << 64) - 1


def source_of(rows, rowid, a):
    """an aggregate's source value per match: uint64 (zero-extended raw bits) for an INT source, int64 for an INT64 one"""
    if a.kind == KIND_INT64:
        item = a.bit_offset >> 5
        return ((rows[rowid, item + 1].astype(np.uint64) << np.uint64(32)) | rows[rowid, item].astype(np.uint64)).view(np.int64)
    return raw_of(rows, rowid, a.bit_offset, a.bit_count).astype(np.uint64)


def aggregate(src, a):
    """one aggregate over one group's source values (non-empty) -> its uint64 value"""
    if a.func == AGGR_SUM:
        if a.kind == KIND_INT and not a.widen:
            return int(np.add.reduce(src.astype(np.uint32), dtype=np.uint32))  # wraps modulo 2^32
        return sum(int(x) for x in src) & M64
    v = src.min() if a.func == AGGR_MIN else src.max()  # (uint64: unsigned; int64: signed)
    return int(v) & M64


def expected_group_aggrs(rowid, weight, value, sources, aggrs, aggr_order, sort_by, desc, K):
    """(head rowid, head weight, key, count, total, aggr uint64 (n, len(aggrs))) of the matches (rowid, weight, group value, one source
    array per aggregate), or DECLINED"""
    rowid, value = np.asarray(rowid, np.uint32), np.asarray(value, np.uint32)
    base = expected_groups(rowid, weight, value, sort_by if aggr_order < 0 else GROUPSORT_KEY, desc, K)
    if base is DECLINED:
        return DECLINED
    # every group, keyed by value, with its aggregates
    o = np.argsort(value, kind="stable")
    sv = value[o]
    first = np.ones(len(sv), bool)
    first[1:] = sv[1:] != sv[:-1]
    at = np.append(np.flatnonzero(first), len(sv))
    keys = sv[at[:-1]]
    table = np.zeros((len(keys), len(aggrs)), np.uint64)
    for ai, (a, src) in enumerate(zip(aggrs, sources)):
        s = np.asarray(src)[o]
        for gi in range(len(keys)):
            table[gi, ai] = aggregate(s[at[gi]:at[gi + 1]], a)
    if aggr_order < 0:
        head_row, head_w, key, count, total = base
    else:
        a = aggrs[aggr_order]
        assert a.kind == KIND_INT and not a.widen, "only a 32-bit aggregate orders the groups"
        # all the groups with their heads (group_expect's model with room for every one of them), then the order by the aggregate
        hr, hw, k_all, c_all, total = expected_groups(rowid, weight, value, GROUPSORT_KEY, False, max(K, len(keys)))
        assert np.array_equal(k_all, keys)
        part = table[:, aggr_order].astype(np.int64)
        g = np.lexsort((hr, -part if desc else part))[:K]
        head_row, head_w, key, count = hr[g], hw[g], k_all[g], c_all[g]
    return head_row, head_w, key, count, total, table[np.searchsorted(keys, key)]


def expected_group_aggr(orc, oi, q, rows, n_docs):
    """the same for a Query with a Group and aggrs, from the oracle's full match set"""
    import dataclasses

    full = all_matches(orc, oi, dataclasses.replace(q, group=None, aggrs=None, aggr_order=-1), n_docs)
    g = q.group
    value = raw_of(rows, full.rowid, g.bit_offset, g.bit_count)
    sources = [source_of(rows, full.rowid, a) for a in q.aggrs]
    return expected_group_aggrs(full.rowid, full.weight, value, sources, q.aggrs, q.aggr_order, g.sort_by, bool(g.desc), q.max_matches)
