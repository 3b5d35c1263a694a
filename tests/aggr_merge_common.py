"""Shared by the tests of the AGGREGATE rows (grouped queries with SUM / MIN / MAX across segments and shards): aggregate rows built in
numpy from match sets with group_aggr_expect's model and never from the library's merge; the check of a merged row against the model
over the WHOLE match set -- all groups, all planes, the padding and both spec words.  Every comparison is exact."""
import dataclasses

import numpy as np

import group_aggr_expect as gae
import group_expect as ge
import group_merge_common as gmc
from group_merge_common import CNT, DECLINED, G, K1, PLANE, RERUN, TOTAL, make_keys, spec_of
from sorted_expect import all_matches, raw_of

MAX_AGGRS = 4
AGGR = 2 * G + 2                 # plane a: AGGR + a * G
GSPEC, ASPEC, WORDS = 6 * G + 2, 6 * G + 3, 6 * G + 4


def plane(a):
    return slice(AGGR + a * G, AGGR + (a + 1) * G)


def aspec_of(q):
    """the aggregate spec word of a Query, written from include/mrk.h's layout"""
    if not q.aggrs:
        return 0
    w = 1 | (len(q.aggrs) << 1) | ((q.aggr_order + 1) << 4)
    for a, g in enumerate(q.aggrs):
        w |= (int(g.func) | (4 if g.kind == gae.KIND_INT64 else 0) | (8 if g.widen else 0)) << (8 + 4 * a)
    return w


def model(q, matches, K):
    """the model's answer for grouped query q (with or without aggregates) -> (rowid, weight, key, count, total, aggr (n, n_aggrs)) or DECLINED"""
    rowid, weight, value, sources = matches
    if q.aggrs:
        return gae.expected_group_aggrs(rowid, weight, value, sources, q.aggrs, q.aggr_order, q.group.sort_by, bool(q.group.desc), K)
    want = ge.expected_groups(rowid, weight, value, q.group.sort_by, bool(q.group.desc), K)
    return want if want is ge.DECLINED else tuple(want) + (np.zeros((len(want[0]), 0), np.uint64),)


def all_groups(q, matches):
    """every group in group order with its aggregates: the model with a K that neither cuts nor declines"""
    return model(q, matches, max(len(matches[0]), 1))


def arow_of_matches(q, rowid, weight, value, sources):
    """The aggregate row a list leaves for grouped query q whose matches are (GLOBAL rowid, weight, group value, one source array per
    aggregate): all its groups with their aggregates' values, or MRK_ROW_DECLINED under the query's two spec words when the list alone
    is past 4 * max_matches."""
    row = np.zeros(WORDS, np.uint64)
    row[GSPEC], row[ASPEC] = spec_of(q), aspec_of(q)
    r, w, k, cnt, total, ag = all_groups(q, (rowid, weight, value, sources))
    if total > ge.GROUPBY_FACTOR * q.max_matches:
        row[TOTAL] = DECLINED
        return row
    row[:total] = make_keys(w, r)
    row[PLANE:PLANE + total] = (k.astype(np.uint64) << np.uint64(32)) | cnt.astype(np.uint64)
    for a in range(ag.shape[1]):
        row[AGGR + a * G:AGGR + a * G + total] = ag[:, a]
    row[CNT] = row[TOTAL] = total
    return row


def arow_of_relevance(rowid, weight, total):
    row = np.zeros(WORDS, np.uint64)
    n = len(rowid)
    row[:n] = make_keys(weight, rowid)
    row[CNT], row[TOTAL] = n, total
    return row


def whole_matches(orc, oi, q, rows, n_docs):
    """(rowid, weight, group value, [source per aggregate]) of every match of grouped query q over the whole corpus"""
    full = all_matches(orc, oi, dataclasses.replace(q, group=None, aggrs=None, aggr_order=-1), n_docs)
    value = raw_of(rows, full.rowid, q.group.bit_offset, q.group.bit_count)
    return full.rowid, full.weight, value, [gae.source_of(rows, full.rowid, a) for a in (q.aggrs or [])]


def cut_matches(matches, lo, hi):
    rowid, weight, value, sources = matches
    m = (rowid >= lo) & (rowid < hi)
    return rowid[m], weight[m], value[m], [s[m] for s in sources]


def shard_arows_np(q, matches, cuts):
    """one numpy aggregate row per rowid range [cuts[s], cuts[s + 1]) from the whole corpus's matches -> [S, WORDS]"""
    return np.stack([arow_of_matches(q, *cut_matches(matches, lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])])


def is_empty(row, flags, gspec, aspec):
    return int(row[TOTAL]) == flags and int(row[CNT]) == 0 and int(row[GSPEC]) == gspec and int(row[ASPEC]) == aspec and not row[:G].any() and not row[PLANE:GSPEC].any()


def check_merged(mdist, q, matches, row, what, must_answer=None):
    """A merged aggregate row against the model over the whole match set: both spec words, the first min(groups, K) entries with their
    aggregates, total_found, ALL groups in group order with all planes, and the zero padding of every plane.  Returns True when the
    model declines (then the row must be MRK_ROW_DECLINED without entries under both spec words).  must_answer: what the test designates."""
    want = model(q, matches, q.max_matches)
    if must_answer is not None:
        assert (want is not ge.DECLINED) == must_answer, (what, "the case is not what the test designates")
    assert int(row[GSPEC]) == spec_of(q) and int(row[ASPEC]) == aspec_of(q), (what, hex(int(row[GSPEC])), hex(int(row[ASPEC])))
    if want is ge.DECLINED:
        assert is_empty(row, DECLINED, spec_of(q), aspec_of(q)), (what, "not declined")
        return True
    assert not int(row[TOTAL]) & (RERUN | DECLINED), (what, "flagged where the model answers", hex(int(row[TOTAL])))
    r, w, k, cnt, total, ag = want
    gr, gw, gk, gc, gt, ga = mdist.arow_groups(row)
    assert gt == total == int(row[CNT]), (what, gt, total)
    assert np.array_equal(gr, r), (what, gr[:8], r[:8])
    assert np.array_equal(gw, w) and np.array_equal(gk, k) and np.array_equal(gc, cnt), (what, gk[:8], k[:8], gc[:8], cnt[:8])
    assert ga.shape == ag.shape and np.array_equal(ga, ag), (what, "aggregates", [hex(int(x)) for x in ga[:2].ravel()], [hex(int(x)) for x in ag[:2].ravel()])
    ar, aw, ak, ac, at, aa = all_groups(q, matches)
    assert np.array_equal(row[:at], make_keys(aw, ar)) and np.array_equal(row[PLANE:PLANE + at], (ak.astype(np.uint64) << np.uint64(32)) | ac.astype(np.uint64)), (what, "all groups")
    assert not row[at:G].any() and not row[PLANE + at:AGGR].any(), (what, "padding")
    for a in range(MAX_AGGRS):
        p = row[plane(a)]
        if a < aa.shape[1]:
            assert np.array_equal(p[:at], aa[:, a]) and not p[at:].any(), (what, "plane", a)
        else:
            assert not p.any(), (what, "a plane beyond n", a)
    return False


def staged(merge, rows, k):
    """((A + B) + C + ...) by pairwise merges with merge(rows [2, nq, WORDS], k): rows [S, nq, WORDS] -> [nq, WORDS]"""
    acc = rows[0]
    for s in range(1, len(rows)):
        acc = merge(np.stack([acc, rows[s]]), k)
    return acc
