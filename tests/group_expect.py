"""The expectation every grouped test compares against: a plain numpy model of the reference's grouping sorter while it has not cut
(CSphKBufferGroupSorter, sphinxsort.cpp:2961-3310), fed with the oracle's full match set (sorted_expect.all_matches) and never with
anything the library computes.

    group key   the raw bits of one row attribute, unsigned
    head        the group's best match by relevance: weight DESC, rowid ASC            (MatchRelevanceLt_fn)
    @count      the group's matches
    order       ONE of group key / @count / head weight, desc or asc, then the head's rowid ASC   (MatchGeneric1_fn, :4708-4720)
    result      the best min(groups, K) groups; total_found = the number of groups       (++m_iTotal on a new group only)
    limit       more than 4 K distinct keys (GROUPBY_FACTOR, :2767): the reference cuts in arrival order -> "declined"

The model is pinned on what the reference recorded for its own test_020 (tests/golden/group_vectors.json, tests/test_group_cpu.py)."""
import numpy as np

from sorted_expect import all_matches, raw_of

GROUPSORT_KEY, GROUPSORT_COUNT, GROUPSORT_WEIGHT = 0, 1, 2
GROUPBY_FACTOR = 4
DECLINED = "declined"


def expected_groups(rowid, weight, value, sort_by, desc, K):
    """(head rowid, head weight, key, count, total) of the matches (rowid, weight, group value), or DECLINED"""
    rowid, weight, value = np.asarray(rowid, np.uint32), np.asarray(weight, np.int64), np.asarray(value, np.uint32)
    # best match first inside each group: group key, weight DESC, rowid ASC
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
    g = np.lexsort((head_row, -part if desc else part))[:K]
    return head_row[g], head_w[g].astype(np.int32), key[g], count[g].astype(np.uint32), len(at)


def expected_group(orc, oi, q, rows, n_docs):
    """the same for a Query with a Group, from the oracle's full match set (every match with its weight, past dead rows and filters)"""
    full = all_matches(orc, oi, _ungrouped(q), n_docs)
    g = q.group
    value = raw_of(rows, full.rowid, g.bit_offset, g.bit_count)
    return expected_groups(full.rowid, full.weight, value, g.sort_by, bool(g.desc), q.max_matches)


def _ungrouped(q):
    import dataclasses

    return dataclasses.replace(q, group=None)


def seeded_value(seed, j):
    """the j-th distinct value of a seed (tests/cpp/group_table.cpp restates it and prints which seeds collide / wrap in small tables)"""
    M = 0xFFFFFFFF
    x = (seed * 0x9E3779B1 + j * 0x85EBCA6B + 0x165667B1) & M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M
    x ^= x >> 15
    x = (x * 0x846CA68B) & M
    x ^= x >> 16
    return x
