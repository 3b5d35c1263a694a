"""Shared by the tests of the GROUP rows (grouped queries across segments and shards): group rows built in numpy from match sets,
from group_expect's model and never from the library's merge; the check of a merged row against the model over the WHOLE match set;
a small corpus cut into rowid-range shards.  Every comparison is exact."""
import dataclasses

import numpy as np

import group_expect as ge
from sorted_expect import all_matches, raw_of

K1 = 1024
G = 4 * K1
CNT, TOTAL, PLANE, SPEC, WORDS = G, G + 1, G + 2, 2 * G + 2, 2 * G + 3
RERUN, DECLINED = 1 << 63, 1 << 62


def make_keys(weight, rowid):
    w = (np.asarray(weight).astype(np.int64).astype(np.uint64) ^ np.uint64(0x80000000)) & np.uint64(0xFFFFFFFF)
    return (w << np.uint64(32)) | ((~np.asarray(rowid).astype(np.uint64)) & np.uint64(0xFFFFFFFF))


def spec_of(q):
    """the group spec word of a grouped Query, written from include/mrk.h's layout"""
    g = q.group
    return 1 | (int(g.sort_by) << 1) | (int(bool(g.desc)) << 3) | (int(g.bit_count) << 8) | (int(q.max_matches) << 16)


def all_groups(rowid, weight, value, sort_by, desc):
    """every group of a match set in group order: the model with a K that neither cuts nor declines"""
    return ge.expected_groups(rowid, weight, value, sort_by, desc, max(len(rowid), 1))


def grow_of_matches(q, rowid, weight, value):
    """The group row a list leaves for grouped query q whose matches are (GLOBAL rowid, weight, group value): all its groups, or
    MRK_ROW_DECLINED under the query's spec when the list alone is past 4 * max_matches."""
    row = np.zeros(WORDS, np.uint64)
    row[SPEC] = spec_of(q)
    r, w, k, cnt, total = all_groups(rowid, weight, value, q.group.sort_by, bool(q.group.desc))
    if total > ge.GROUPBY_FACTOR * q.max_matches:
        row[TOTAL] = DECLINED
        return row
    row[:total] = make_keys(w, r)
    row[PLANE:PLANE + total] = (k.astype(np.uint64) << np.uint64(32)) | cnt.astype(np.uint64)
    row[CNT] = row[TOTAL] = total
    return row


def grow_of_relevance(rowid, weight, total):
    row = np.zeros(WORDS, np.uint64)
    n = len(rowid)
    row[:n] = make_keys(weight, rowid)
    row[CNT], row[TOTAL] = n, total
    return row


def whole_matches(orc, oi, q, rows, n_docs):
    """(rowid, weight, group value) of every match of grouped query q over the whole corpus"""
    full = all_matches(orc, oi, dataclasses.replace(q, group=None), n_docs)
    return full.rowid, full.weight, raw_of(rows, full.rowid, q.group.bit_offset, q.group.bit_count)


def shard_rows_np(q, matches, cuts):
    """one numpy group row per rowid range [cuts[s], cuts[s + 1]) from the whole corpus's matches -> [S, WORDS]"""
    rowid, weight, value = matches
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m = (rowid >= lo) & (rowid < hi)
        out.append(grow_of_matches(q, rowid[m], weight[m], value[m]))
    return np.stack(out)


def check_merged(mdist, q, matches, row, what, must_answer=None):
    """A merged group row against the model over the whole match set: the first min(groups, K) entries, total_found, the zero
    padding, the spec word and -- beyond what mrk_result shows -- all groups in group order.  Returns True when the model declines
    (then the row must be MRK_ROW_DECLINED without entries).  must_answer: what the test designates."""
    want = ge.expected_groups(*matches, q.group.sort_by, bool(q.group.desc), q.max_matches)
    if must_answer is not None:
        assert (want is not ge.DECLINED) == must_answer, (what, "the case is not what the test designates")
    assert int(row[SPEC]) == spec_of(q), (what, hex(int(row[SPEC])))
    if want is ge.DECLINED:
        assert int(row[TOTAL]) == DECLINED and int(row[CNT]) == 0 and not row[:G].any() and not row[PLANE:SPEC].any(), (what, "not declined")
        return True
    assert not int(row[TOTAL]) & (RERUN | DECLINED), (what, "flagged where the model answers", hex(int(row[TOTAL])))
    r, w, k, cnt, total = want
    gr, gw, gk, gc, gt = mdist.grow_groups(row)
    assert gt == total == int(row[CNT]), (what, gt, total)
    assert np.array_equal(gr, r), (what, gr[:8], r[:8])
    assert np.array_equal(gw, w) and np.array_equal(gk, k) and np.array_equal(gc, cnt), (what, gk[:8], k[:8], gc[:8], cnt[:8])
    ar, aw, ak, ac, at = all_groups(*matches, q.group.sort_by, bool(q.group.desc))
    assert np.array_equal(row[:at], make_keys(aw, ar)) and np.array_equal(row[PLANE:PLANE + at], (ak.astype(np.uint64) << np.uint64(32)) | ac.astype(np.uint64)), (what, "all groups")
    assert not row[at:G].any() and not row[PLANE + at:SPEC].any(), (what, "padding")
    return False


def staged(mdist, rows, k):
    """((A + B) + C + ...) by pairwise merges: rows [S, nq, WORDS] -> [nq, WORDS]"""
    acc = rows[0]
    for s in range(1, len(rows)):
        acc = mdist.merge_grows_np(np.stack([acc, rows[s]]), k)
    return acc
