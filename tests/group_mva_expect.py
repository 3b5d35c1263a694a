"""The expectation of a query grouped by a multi-value attribute (Group(mva_bits=32, ...); mrk_group_mva, include/mrk.h): a plain numpy
model of MVAGroupSorter_T::Push (sphinxsort.cpp:4113-4156) over a grouping sorter that has not cut, fed with the oracle's full match
set (sorted_expect.all_matches) and the blob pool, and never with anything the library computes.

    pushes      every match once per STORED value of its MVA: no de-duplication, no re-sorting; a doc without values joins no group
    head        the group's best match by relevance: weight DESC, rowid ASC
    @count      the group's pushes
    order       ONE of group key / @count / head weight, desc or asc, then the head's rowid ASC (group_expect.expected_groups), and
                LAST the group value ascending: one doc may head several groups, and where (order part, head rowid) ties the reference's
                answer is open -- the device puts the smaller value first, whatever desc says (tests/cpp/group_mva.cpp restates it)
    result      the best min(groups, K) groups; total_found = the number of groups
    limit       more than 4 K distinct values over all pushes: DECLINED

Pinned on what the reference recorded for test_020's MVA group queries (tests/golden/group_mva_vectors.json, test_group_mva_cpu.py)."""
import dataclasses

import numpy as np

from group_expect import DECLINED, GROUPBY_FACTOR, GROUPSORT_COUNT, GROUPSORT_KEY, GROUPSORT_WEIGHT
from sorted_expect import all_matches


def mva_values(pool, off, blob_attr_id, n_blob_attrs):
    """the stored 32-bit values of blob attribute blob_attr_id in the blob row at pool[off:] (attribute.cpp:495-513), in stored order"""
    sz = (1, 2, 4)[int(pool[off])]
    ends = [int.from_bytes(bytes(pool[off + 1 + a * sz: off + 1 + (a + 1) * sz]), "little") for a in range(n_blob_attrs)]
    l0, l1 = (ends[blob_attr_id - 1] if blob_attr_id else 0), ends[blob_attr_id]
    data = off + 1 + n_blob_attrs * sz + l0
    return np.frombuffer(bytes(pool[data: data + (l1 - l0) // 4 * 4]), "<u4")


def expand(rowid, weight, values_of):
    """(rowid, weight, value) per push: match i repeated once per value of values_of(rowid[i])"""
    rr, ww, vv = [], [], []
    for r, w in zip(np.asarray(rowid).tolist(), np.asarray(weight).tolist()):
        v = values_of(r)
        rr.append(np.full(len(v), r, np.uint32)), ww.append(np.full(len(v), w, np.int64)), vv.append(np.asarray(v, np.uint32))
    if not rr:
        return np.zeros(0, np.uint32), np.zeros(0, np.int64), np.zeros(0, np.uint32)
    return np.concatenate(rr), np.concatenate(ww), np.concatenate(vv)


def expected_groups_mva(rowid, weight, value, sort_by, desc, K):
    """(head rowid, head weight, key, count, total) of the pushes (rowid, weight, value), or DECLINED"""
    rowid, weight, value = np.asarray(rowid, np.uint32), np.asarray(weight, np.int64), np.asarray(value, np.uint32)
    o = np.lexsort((rowid, -weight, value))
    rowid, weight, value = rowid[o], weight[o], value[o]
    first = np.ones(len(value), bool)
    first[1:] = value[1:] != value[:-1]
    at = np.flatnonzero(first)
    if len(at) > GROUPBY_FACTOR * K:
        return DECLINED
    key, head_row, head_w = value[at], rowid[at], weight[at]
    count = np.diff(np.append(at, len(value)))
    part = {GROUPSORT_KEY: key.astype(np.int64), GROUPSORT_COUNT: count.astype(np.int64), GROUPSORT_WEIGHT: head_w}[sort_by]
    g = np.lexsort((key, head_row, -part if desc else part))[:K]  # (the tie rule is the last key: the smaller group value first)
    return head_row[g], head_w[g].astype(np.int32), key[g], count[g].astype(np.uint32), len(at)


def has_tie(rowid, weight, value, sort_by, desc):
    """whether two groups of the pushes compare equal before the tie rule"""
    got = expected_groups_mva(rowid, weight, value, sort_by, desc, 1 << 30)
    head_row, head_w, key, count, _ = got
    part = {GROUPSORT_KEY: key.astype(np.int64), GROUPSORT_COUNT: count.astype(np.int64), GROUPSORT_WEIGHT: head_w.astype(np.int64)}[sort_by]
    pairs = set(zip(part.tolist(), head_row.tolist()))
    return len(pairs) < len(key)


def expected_group_mva(orc, oi, q, rows, pool, n_docs):
    """the same for a Query whose Group names an MVA, from the oracle's full match set (past dead rows, filters and weight filters)"""
    full = all_matches(orc, oi, dataclasses.replace(q, group=None), n_docs)
    g = q.group
    values_of = lambda r: mva_values(pool, int(rows[r, 2]) | (int(rows[r, 3]) << 32), g.blob_attr_id, g.n_blob_attrs)
    return expected_groups_mva(*expand(full.rowid, full.weight, values_of), g.sort_by, bool(g.desc), q.max_matches)
