"""GPU: grouped queries WITH aggregates (Query.aggrs) answered across segments and shards through the AGGREGATE rows (MRK_AROW_WORDS).
The yardstick is the group rows': ONE grouping sorter fed with the matches of all segments.  The merge of the shards' exported rows
(mrk_topk_merge_arows) must equal, word for word, the row the unsharded device run exports, group_aggr_expect's model over the whole
match set, and the numpy mirror (dist.merge_arows_np) -- every plane and its zero padding included, into buffers pre-filled with 0xEE
with guard rows in front of and behind the output.  Every comparison is exact, and no case is skipped because the model declines
unless the test designates the decline.

Columns of the edge corpus's rows (dwords): test_gpu_group_aggr's twenty, then  G_MEM one value in every shard of the 8-way cut and
three values in one shard each (first, middle, last) | G_REV one value with ONE doc per shard and one value per shard for the rest |
V_REV 4 on the former's docs, 5 on one doc of each of the latter | V_WRAP 2^29 on the former's docs, 5 likewise | G_64 small groups
over X64, an aligned signed 64 (INT64_MAX + 1 across two shards; only -1; only INT64_MIN; only INT64_MAX) | V_EXT 50 but for a 3 in
shard 2 and a 99 in shard 6 | G_ONE twenty values in shard 3, two elsewhere (K = 4: that list alone declines while it runs)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import aggr_merge_common as amc
import test_gpu_group as tg
import test_gpu_group_aggr as tga
from group_expect import GROUPSORT_COUNT, GROUPSORT_KEY, GROUPSORT_WEIGHT
from test_gpu_group import BITS, C2, C16, C17, C64, C65, N_DOCS, Settings, shapes
from test_gpu_group_aggr import BIG, I64, ONES, UNIT, ZERO, Q, aggr_sets
from test_gpu_group_merge import CUTS, D4, D5, D8, D9, D16, D17, D4096, D4097, Corpus, disjoint_rows
from test_gpu_order_merge import Hip
from test_gpu_sort_merge import L, off

pytestmark = pytest.mark.gpu

RW, G = amc.WORDS, amc.G
EE = np.uint64(0xEEEEEEEEEEEEEEEE)
G_MEM, G_REV, V_REV, V_WRAP, G_64, X64, X64HI, V_EXT, G_ONE = range(tga.STRIDE, tga.STRIDE + 9)
I64_MIN, I64_MAX, M64, M32 = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1, 0xFFFFFFFF


def edge_rows():
    r = np.arange(N_DOCS, dtype=np.uint64)
    rows = np.zeros((N_DOCS, tga.STRIDE + 9), np.uint32)
    rows[:, :tga.STRIDE] = tga.make_rows(N_DOCS)
    lo = CUTS[8][:-1]
    shard = np.searchsorted(np.array(CUTS[8][1:]), r, side="right")
    rows[:, G_MEM] = 100
    for s, v in ((0, 200), (4, 201), (7, 202)):
        rows[lo[s] + 11, G_MEM] = v
    rows[:, G_REV] = 1000 + shard
    rows[:, V_EXT] = 50
    x64 = np.zeros(N_DOCS, np.int64)
    rows[:, G_64] = 11
    for s in range(8):
        rows[lo[s] + 3, G_REV], rows[lo[s] + 3, V_REV], rows[lo[s] + 3, V_WRAP] = 1, 4, 1 << 29
        rows[lo[s] + 4, V_REV] = rows[lo[s] + 4, V_WRAP] = 5
    rows[lo[2] + 20, V_EXT], rows[lo[6] + 20, V_EXT] = 3, 99
    for v, docs in ((7, ((0, I64_MAX), (1, 1))), (8, ((1, -1), (5, -1), (5, -1))), (9, ((2, I64_MIN), (6, I64_MIN))), (10, ((0, I64_MAX), (7, I64_MAX)))):
        for j, (s, x) in enumerate(docs):
            rows[lo[s] + 30 + 3 * v + j, G_64], x64[lo[s] + 30 + 3 * v + j] = v, x
    rows[:, X64], rows[:, X64HI] = (x64.view(np.uint64) & np.uint64(M32)).astype(np.uint32), (x64.view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    rows[:, G_ONE] = np.where(shard == 3, r % 20, r % 2).astype(np.uint32)
    return rows


def limit_rows():
    rows = tga.make_rows(N_DOCS)
    rows[:, :9] = disjoint_rows()[:, :9]
    return rows


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    hip = Hip()
    yield m, ctx, batch, hip
    hip.free()
    batch.close()
    ctx.close()


@pytest.fixture(scope="module")
def corpora(orc, dev):
    m, ctx, _, _ = dev
    cs = {4: Corpus(m, ctx, orc, 4, tga.make_rows(N_DOCS), (1, 2, 3, 8)), 17: Corpus(m, ctx, orc, 17, tga.make_rows(N_DOCS), (1, 2, 3, 8))}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def limits(orc, dev):
    m, ctx, _, _ = dev
    c = Corpus(m, ctx, orc, 4, limit_rows(), (1, 3, 8), seed=11)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edges(orc, dev):
    m, ctx, _, _ = dev
    c = Corpus(m, ctx, orc, 4, edge_rows(), (1, 8), seed=13)
    yield c
    c.close()


def matches(orc, c, q):
    """(rowid, weight, group value, sources) of q over the whole corpus, computed once per (shape, group, aggregates)"""
    cache = c.__dict__.setdefault("acache", {})
    key = (repr(q.root), q.ranker, q.group.bit_offset, q.group.bit_count, q.index_weight, repr(q.aggrs))
    if key not in cache:
        cache[key] = amc.whole_matches(orc, c.oi, q, c.rows, c.n_docs)
    return cache[key]


def export(batch, hip, segs, qs, want_status=None, results=None):
    """every segment's aggregate rows of the batch, exported behind mrk_batch_wait -> device [S][nq][AROW_WORDS] pre-filled with 0xEE"""
    nq, S = len(qs), len(segs)
    dst = hip.malloc(S * nq * RW * 8)
    hip.fill(dst, 0xEE, S * nq * RW * 8)
    for s, seg in enumerate(segs):
        batch.submit(seg, qs)
        batch.wait()
        assert batch.stats()["packed"] == 1
        if want_status is not None:
            assert [r.status for r in batch.results()] == want_status[s], ("shard", s)
        if results is not None:
            results.append(batch.results())
        batch.export_arows(dst.value + s * nq * RW * 8)
    return dst


def merge(ctx, hip, rows_all, n_lists, nq, k=1024, form="sync"):
    """one merge into a 0xEE buffer with a guard row on either side, which must stay untouched"""
    lib, chk = L()
    out = hip.malloc((nq + 2) * RW * 8)
    hip.fill(out, 0xEE, (nq + 2) * RW * 8)
    if form == "async":
        chk(lib.mrk_topk_merge_arows_async(ctx._h, rows_all, n_lists, nq, k, off(out, RW * 8), None, 1))
        chk(lib.mrk_merge_wait(ctx._h, 1))
    else:
        chk(lib.mrk_topk_merge_arows(ctx._h, rows_all, n_lists, nq, k, off(out, RW * 8)))
    got = hip.to_host(out, (nq + 2, RW))
    assert (got[0] == EE).all() and (got[-1] == EE).all(), "the guard rows"
    return got[1:-1]


def merge_host(ctx, hip, rows, k=1024):
    """host rows [S, nq, RW] through the kernel; the result must equal the numpy mirror"""
    from manticoresearch_amd import dist as mdist

    buf = hip.malloc(rows.size * 8)
    hip.to_dev(buf, np.ascontiguousarray(rows))
    got = merge(ctx, hip, buf, rows.shape[0], rows.shape[1], k)
    assert np.array_equal(got, mdist.merge_arows_np(rows, k)), "kernel != numpy mirror"
    return got


def same_as_result(mdist, row, g, what, rowid_base=0):
    """mrk_result / mrk_batch_result_aggrs of a run against the first min(n, max_matches) entries of the row it exported (a row's
    rowids are global, a result's the segment's own)"""
    r, w, k, cnt, total, ag = mdist.arow_groups(row)
    assert g.status == 0 and g.total_found == total, (what, g.status, g.total_found, total)
    assert np.array_equal(g.rowid + np.uint32(rowid_base), r) and np.array_equal(g.weight, w) and np.array_equal(g.group_key, k) and np.array_equal(g.group_count, cnt), what
    assert (g.aggr is None and ag.shape[1] == 0) or np.array_equal(g.aggr, ag), (what, "aggregates")


def sharded_queries(m, c):
    """all seven shapes under all six aggregate sets (1, 3 and 4 aggregates at once; every func over INT, a bit-field, widened and
    INT64 sources), the group orders in turn; then each ordering direction by a 32-bit SUM, MIN and MAX; columns at, under and over
    their limit"""
    S = aggr_sets(m)
    cols = [(C64, 32, 0, 16, True), (C16, 32, 0, 4, True), (C2, 32, 0, 1000, True), (BITS, 7, 9, 32, True), (C65, 32, 0, 16, False), (C17, 32, 0, 1024, True)]
    qs, must = [], []
    for si, sh in enumerate(shapes(m)):
        for ni, name in enumerate(S):
            col, bits, shift, K, ok = cols[(si + ni) % len(cols)]
            by, desc = tg.ORDERS[(si * 5 + ni) % 6]
            qs.append(c.globalize(Q(m, sh, col, S[name], bits=bits, shift=shift, K=K, by=by, desc=desc, index_weight=1 + (si + ni) % 2 * 2)))
            must.append(ok if sh in ("one", "none") or ok else None)  # (keyword 0 is in every doc: every value of the column matches)
    for sh, name, order in (("one", "one", 0), ("and2", "smm", 1), ("prox2", "smm", 2), ("tree", "bits", 0)):
        for desc in (True, False):
            qs.append(c.globalize(Q(m, sh, C64, S[name], K=16, desc=desc, order=order)))
            must.append(True)
    return qs, must


@pytest.mark.parametrize("n_fields", [4, 17])
def test_sharded_equals_unsharded_equals_model(orc, dev, corpora, n_fields):
    """1, 2, 3 and 8 lists: merged == the whole segment's row == the model == the numpy mirror; the whole segment's mrk_result and
    mrk_batch_result_aggrs are the row's first min(n, max_matches) entries"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    c = corpora[n_fields]
    qs, must = sharded_queries(m, c)
    nq = len(qs)
    res = []
    whole = hip.to_host(export(batch, hip, [c.whole], qs, results=res), (1, nq, RW))[0]
    n_decl = 0
    for qi, q in enumerate(qs):
        declined = amc.check_merged(mdist, q, matches(orc, c, q), whole[qi], ("unsharded", n_fields, qi), must[qi])
        n_decl += declined
        if not declined:
            same_as_result(mdist, whole[qi], res[0][qi], ("result", n_fields, qi))
    assert n_decl >= 2 and n_decl == sum(int(r[amc.TOTAL]) == amc.DECLINED for r in whole)
    hip.free()
    for S in (1, 2, 3, 8):
        dev_rows = export(batch, hip, c.segs[S], qs)
        lists = hip.to_host(dev_rows, (S, nq, RW))
        got = merge(ctx, hip, dev_rows, S, nq)
        assert np.array_equal(got, mdist.merge_arows_np(lists, 1024)), ("kernel != numpy mirror", S)
        assert np.array_equal(got, whole), ("merged != the unsharded row", S, [qi for qi in range(nq) if not np.array_equal(got[qi], whole[qi])][:5])
        hip.free()


def run_edge(orc, dev, c, qs, S=8):
    """the S-way cut of c merged == the whole segment's rows == the mirror == the model (every query must answer) -> the merged rows, the lists"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    qs = [c.globalize(q) for q in qs]
    nq = len(qs)
    whole = hip.to_host(export(batch, hip, [c.whole], qs, want_status=[[0] * nq]), (nq, RW))
    dev_rows = export(batch, hip, c.segs[S], qs, want_status=[[0] * nq] * S)
    lists = hip.to_host(dev_rows, (S, nq, RW))
    got = merge(ctx, hip, dev_rows, S, nq)
    assert np.array_equal(got, mdist.merge_arows_np(lists, 1024)) and np.array_equal(got, whole)
    for qi, q in enumerate(qs):
        assert not amc.check_merged(mdist, q, matches(orc, c, q), got[qi], ("edge", qi), True)
    hip.free()
    return got, lists


def group_of(row, value):
    """(entry index, count, [aggregate values]) of group `value` in a row"""
    n = int(row[amc.CNT])
    at = np.flatnonzero((row[amc.PLANE:amc.PLANE + n] >> np.uint64(32)) == np.uint64(value))
    assert len(at) == 1, (value, n)
    i = int(at[0])
    return i, int(row[amc.PLANE + i]) & M32, [int(row[amc.AGGR + a * G + i]) for a in range(amc.MAX_AGGRS)]


def test_edge_sum_wraps_across_lists(orc, dev, edges):
    """group 1 of G_REV holds one doc per shard: every list's 32-bit SUM(ONES) is 0xFFFFFFFF, the merged one wraps; widened it does not"""
    m = dev[0]
    A = m.Aggr
    got, lists = run_edge(orc, dev, edges, [Q(m, "one", G_REV, [A(m.AGGR_SUM, ONES * 32, 32), A(m.AGGR_SUM, ONES * 32, 32, widen=True)], K=4)])
    for l in range(8):
        assert group_of(lists[l, 0], 1)[1:] == (1, [M32, M32, 0, 0]), "below 2^32 in every list"
    assert group_of(got[0], 1)[1:] == (8, [(8 * M32) & M32, 8 * M32, 0, 0])


def test_edge_int64_sums_and_zero_identities(orc, dev, edges):
    """an INT64 SUM across INT64_MAX in two lists; MIN of only 0xFFFFFFFF (mapped 0) and MAX of only 0; signed MAX of INT64_MIN, signed
    MIN of INT64_MAX, a group holding only -1"""
    m = dev[0]
    A, I6 = m.Aggr, m.SORTKEY_INT64
    x = X64 * 32
    got, lists = run_edge(orc, dev, edges, [Q(m, "none", G_64, [A(m.AGGR_SUM, x, 64, kind=I6), A(m.AGGR_MIN, x, 64, kind=I6), A(m.AGGR_MAX, x, 64, kind=I6), A(m.AGGR_MIN, ONES * 32, 32)], K=4),
                                                Q(m, "one", G_64, [A(m.AGGR_MIN, ONES * 32, 32), A(m.AGGR_MAX, ZERO * 32, 32), A(m.AGGR_MIN, ONES * 32, 32, widen=True), A(m.AGGR_MAX, ZERO * 32, 32, widen=True)], K=4)])
    assert group_of(lists[0, 0], 7)[2][0] == I64_MAX and group_of(lists[1, 0], 7)[2][0] == 1
    assert group_of(got[0], 7)[1:] == (2, [(I64_MAX + 1) & M64, 1, I64_MAX, M32]), "the sum crosses INT64_MAX in two's complement"
    assert group_of(got[0], 8)[1:] == (3, [(-3) & M64, M64, M64, M32]), "a group holding only -1"
    assert group_of(got[0], 9)[1:] == (2, [0, I64_MIN & M64, I64_MIN & M64, M32]), "signed MAX of INT64_MIN"
    assert group_of(got[0], 10)[1:] == (2, [(2 * I64_MAX) & M64, I64_MAX, I64_MAX, M32]), "signed MIN of INT64_MAX"
    for v in (7, 8, 9, 10, 11):
        assert group_of(got[1], v)[2] == [M32, 0, M32, 0], "MIN of only 0xFFFFFFFF, MAX of only 0"


def test_edge_group_membership_and_extremes(orc, dev, edges):
    """a group in one list of 8 (first, middle, last) next to a group in all 8; a MIN and a MAX whose extreme sits in exactly one list"""
    m = dev[0]
    A = m.Aggr
    got, lists = run_edge(orc, dev, edges, [Q(m, "one", G_MEM, [A(m.AGGR_SUM, UNIT * 32, 32), A(m.AGGR_MIN, V_EXT * 32, 32), A(m.AGGR_MAX, V_EXT * 32, 32, widen=True), A(m.AGGR_SUM, BIG * 32, 32, widen=True)], K=4, by=GROUPSORT_COUNT)])
    assert [int(x) for x in lists[:, 0, amc.CNT]] == [2, 1, 1, 1, 2, 1, 1, 2]
    assert int(got[0, amc.CNT]) == 4 and group_of(got[0], 100)[1] == N_DOCS - 3 and group_of(got[0], 100)[2][:3] == [N_DOCS - 3, 3, 99]
    for v in (200, 201, 202):
        assert group_of(got[0], v)[1:3] == (1, [1, 50, 50, group_of(got[0], v)[2][3]])
    assert [group_of(lists[l, 0], 100)[2][1] for l in range(8)] == [50, 50, 3, 50, 50, 50, 50, 50] and [group_of(lists[l, 0], 100)[2][2] for l in range(8)] == [50] * 6 + [99, 50]


def test_edge_order_reversed_by_the_merge(orc, dev, edges):
    """group 1 is worst in every list's own order and best after merging: descending by SUM(V_REV), 4 a list against 5, 32 merged;
    ascending by SUM(V_WRAP), 2^29 a list -- the largest -- and 0 after the wrap"""
    m = dev[0]
    A = m.Aggr
    got, lists = run_edge(orc, dev, edges, [Q(m, "one", G_REV, [A(m.AGGR_SUM, V_REV * 32, 32)], K=4, desc=True, order=0),
                                                Q(m, "none", G_REV, [A(m.AGGR_SUM, V_WRAP * 32, 32), A(m.AGGR_SUM, V_WRAP * 32, 32, widen=True)], K=4, desc=False, order=0)])
    for l in range(8):
        assert [group_of(lists[l, qi], 1)[0] for qi in (0, 1)] == [1, 1] and int(lists[l, 0, amc.CNT]) == 2, "last of two in every list"
    assert group_of(got[0], 1)[0] == 0 and group_of(got[0], 1)[2][0] == 32 and int(got[0, amc.CNT]) == 9
    assert group_of(got[1], 1)[0] == 0 and group_of(got[1], 1)[2][:2] == [0, 8 << 29]


def limit_queries(m, c):
    S = aggr_sets(m)
    cases = [(D16, 4, True), (D17, 4, False), (D4, 1, True), (D5, 1, False), (D8, 2, True), (D9, 2, False)]
    qs = [c.globalize(Q(m, sh, col, S[name], K=K, by=by)) for col, K, _ in cases for sh, by, name in (("one", GROUPSORT_COUNT, "four"), ("none", GROUPSORT_KEY, "one"))]
    return qs, [ok for _, _, ok in cases for _ in range(2)]


def test_limit_edges_with_aggregates(orc, dev, limits):
    """shard-disjoint values: exactly 4 * max_matches merged groups answer, one more is MRK_ROW_DECLINED without entries under both
    spec words -- at max_matches 1, 2 and 4 over three lists and at 1024 (8 x 512 = 4096 groups, the full-size table with four planes)"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    c = limits
    qs, must = limit_queries(m, c)
    nq = len(qs)
    dev_rows = export(batch, hip, c.segs[3], qs, want_status=[[0] * nq] * 3)
    lists = hip.to_host(dev_rows, (3, nq, RW))
    assert not (lists[:, :, amc.TOTAL] & np.uint64(amc.RERUN | amc.DECLINED)).any(), "every list alone is inside its limit"
    got = merge(ctx, hip, dev_rows, 3, nq)
    assert np.array_equal(got, mdist.merge_arows_np(lists, 1024))
    for qi, q in enumerate(qs):
        assert amc.check_merged(mdist, q, matches(orc, c, q), got[qi], ("limit", qi), must[qi]) == (not must[qi])
        assert int(got[qi, amc.GSPEC]) == amc.spec_of(q) and int(got[qi, amc.ASPEC]) == amc.aspec_of(q) != 0
    assert [int(x) for x in got[::2, amc.TOTAL]] == [16, amc.DECLINED, 4, amc.DECLINED, 8, amc.DECLINED]
    whole = hip.to_host(export(batch, hip, [c.whole], qs), (nq, RW))
    assert np.array_equal(got, whole), "the unsharded run answers and declines the same"
    hip.free()
    S = aggr_sets(m)
    big = [c.globalize(Q(m, "one", D4096, S["four"], K=1024, by=GROUPSORT_COUNT, desc=False)), c.globalize(Q(m, "one", D4097, S["four"], K=1024)),
           c.globalize(Q(m, "none", D4096, S["one"], K=1024, desc=False, order=0))]
    dev_rows = export(batch, hip, c.segs[8], big, want_status=[[0] * 3] * 8)
    lists = hip.to_host(dev_rows, (8, 3, RW))
    assert [int(x) for x in lists[:, 0, amc.TOTAL]] == [512] * 8 and sorted(int(x) for x in lists[:, 1, amc.TOTAL]) == [512] * 7 + [513]
    got = merge(ctx, hip, dev_rows, 8, 3)
    assert np.array_equal(got, mdist.merge_arows_np(lists, 1024))
    for qi, ok in enumerate((True, False, True)):
        assert amc.check_merged(mdist, big[qi], matches(orc, c, big[qi]), got[qi], ("4096", qi), ok) == (not ok)
    assert int(got[0, amc.CNT]) == 4096 and int(got[2, amc.TOTAL]) == 4096 and amc.is_empty(got[1], amc.DECLINED, amc.spec_of(big[1]), amc.aspec_of(big[1]))
    hip.free()


def test_associativity_of_staged_merges(dev, edges, limits):
    """pairwise staged merges of the 8-way cut -- a left fold and a balanced tree -- equal the one-step merge word for word; G_ONE's
    fourth list declined while it ran (20 values at K = 4) and the merged row says so at every stage it is part of"""
    m, ctx, batch, hip = dev
    S = aggr_sets(m)
    A = m.Aggr
    c = edges
    qs = [Q(m, "one", G_REV, [A(m.AGGR_SUM, V_REV * 32, 32)], K=4, order=0), Q(m, "none", G_REV, [A(m.AGGR_SUM, V_WRAP * 32, 32)], K=4, desc=False, order=0),
          Q(m, "one", G_ONE, S["four"], K=4), Q(m, "and2", C64, S["four"], K=16, by=GROUPSORT_COUNT), Q(m, "prox2", C16, S["edges"], K=8, by=GROUPSORT_WEIGHT, desc=False),
          Q(m, "one", G_MEM, S["smm"], K=1), tg.Q(m, "and2", C64, K=16), m.Query(shapes(m)["and2"][0], ranker=m.SPH_RANK_BM25, max_matches=50), Q(m, "one", G_64, S["wide"], K=2)]
    qs = [c.globalize(q) for q in qs]
    nq = len(qs)
    dev_rows = export(batch, hip, c.segs[8], qs, want_status=[[0] * nq] * 3 + [[0, 0, -2] + [0] * (nq - 3)] + [[0] * nq] * 4)
    lists = hip.to_host(dev_rows, (8, nq, RW))
    assert amc.is_empty(lists[3, 2], amc.DECLINED, amc.spec_of(qs[2]), amc.aspec_of(qs[2])), "declined while it ran, under its own two spec words"
    one_step = merge(ctx, hip, dev_rows, 8, nq)
    assert amc.is_empty(one_step[2], amc.DECLINED, amc.spec_of(qs[2]), amc.aspec_of(qs[2])) and not (np.delete(one_step, 2, 0)[:, amc.TOTAL] & np.uint64(amc.RERUN | amc.DECLINED)).any()
    acc = lists[0]
    for s in range(1, 8):  # ((((0 + 1) + 2) + ...) + 7)
        acc = merge_host(ctx, hip, np.stack([acc, lists[s]]))
    assert np.array_equal(acc, one_step), "left fold"
    hip.free()
    level = list(lists)
    while len(level) > 1:  # ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7))
        level = [merge_host(ctx, hip, np.stack(level[i:i + 2])) for i in range(0, len(level), 2)]
    assert np.array_equal(level[0], one_step), "balanced tree"
    assert np.array_equal(merge_host(ctx, hip, np.stack([merge_host(ctx, hip, lists[:3]), merge_host(ctx, hip, lists[3:])])), one_step), "3 + 5"
    hip.free()


def test_flags_and_mismatches_whichever_list_carries_them(dev, limits):
    """RERUN, declined under spec words 0 and under its own, aggregate spec words that differ in one bit, with aggregates next to
    without, max_matches > k, every hostile row: the same merged row whichever list it is, equal to the mirror, the guards untouched"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    c = limits
    aggrs = [m.Aggr(m.AGGR_SUM, BIG * 32, 32), m.Aggr(m.AGGR_MIN, I64 * 32, 64, kind=m.SORTKEY_INT64)]
    q = c.globalize(Q(m, "one", D16, aggrs, K=4, desc=False, order=0))
    relq = c.globalize(m.Query(shapes(m)["one"][0], ranker=m.SPH_RANK_BM25, max_matches=5))
    base = hip.to_host(export(batch, hip, c.segs[3], [q, relq]), (3, 2, RW))
    spec, aspec, R, D = amc.spec_of(q), amc.aspec_of(q), amc.RERUN, amc.DECLINED
    good = merge_host(ctx, hip, base)
    assert int(good[0, amc.TOTAL]) == 16 and int(good[0, amc.GSPEC]) == spec and int(good[0, amc.ASPEC]) == aspec

    def run(rows, k=1024):
        got = merge_host(ctx, hip, rows, k)
        assert k != 1024 or np.array_equal(got[1], good[1]), "the batch's other query is untouched"
        return got[0]

    def rerun(row):
        row[:amc.GSPEC], row[amc.TOTAL] = 0, R

    def planner_declined(row):
        row[:], row[amc.TOTAL] = 0, D

    def own_declined(row):
        row[:amc.GSPEC], row[amc.TOTAL] = 0, D

    def setw(at, value):
        def f(row):
            row[at] = value
        return f

    g2 = mdist.aggr_spec_word
    hostile = [setw(amc.CNT, G + 1), setw(amc.CNT, 0xFFFFFFFFFFFFFFFF), setw(amc.GSPEC, spec | (1 << 40)), setw(amc.GSPEC, 0), setw(amc.GSPEC, mdist.group_spec_word(GROUPSORT_COUNT, 0, 32, 4)),
               setw(amc.ASPEC, aspec | 0x80), setw(amc.ASPEC, aspec | (1 << 24)), setw(amc.ASPEC, aspec | (1 << 63)), setw(amc.ASPEC, aspec & ~0xE), setw(amc.ASPEC, (aspec & ~0xE) | (5 << 1)),
               setw(amc.ASPEC, aspec & ~(3 << 8)), setw(amc.ASPEC, aspec | (1 << 16)), setw(amc.ASPEC, aspec | (8 << 12)), setw(amc.ASPEC, g2(aggrs, 1)), setw(amc.ASPEC, (aspec & ~0x70) | (3 << 4))]
    for fi, (fault, flags) in enumerate([(rerun, R), (planner_declined, D), (own_declined, D)] + [(h, D) for h in hostile]):
        got = []
        for l in range(3):
            rows = base.copy()
            fault(rows[l, 0])
            got.append(run(rows))
        assert amc.is_empty(got[0], flags, spec, aspec) and np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), fi
        hip.free()
    rows = base.copy()
    rerun(rows[0, 0]), planner_declined(rows[2, 0])
    assert amc.is_empty(run(rows), R | D, spec, aspec)
    for other in (aspec ^ (2 << 8), aspec ^ (1 << 4), g2(aggrs[:1], 0), g2(aggrs + aggrs[:1], 0), 0):  # a func, the order, n; with next to without
        for l in range(3):
            rows = base.copy()
            rows[l, 0, amc.ASPEC] = other
            assert amc.is_empty(run(rows), D, spec, other if l == 0 else aspec), (hex(other), l)
        hip.free()
    rows = base.copy()
    rows[1, 0] = base[1, 1]  # a relevance row among the grouped ones
    assert amc.is_empty(run(rows), D, spec, aspec)
    assert amc.is_empty(run(base.copy(), k=3), D, spec, aspec), "max_matches above the call's k"
    rows = base.copy()  # counts: a sum of exactly 2^32 - 1 is a count; one more declines under both spec words
    v = int(rows[0, 0, amc.PLANE]) >> 32
    rows[0, 0, amc.PLANE] = (v << 32) | 0xFFFFFFFE
    rows[1, 0, amc.PLANE] = (v << 32) | 1
    assert int(run(rows)[amc.TOTAL]) == 15
    rows[1, 0, amc.PLANE] += np.uint64(1)
    assert amc.is_empty(run(rows), D, spec, aspec), "a count of 2^32"
    hip.free()


def test_mixed_batch_one_export_one_merge(orc, dev, corpora):
    """relevance, grouped without aggregates, with 1 and with 4, sorted (declined) and over the limit at run time in one batch; the
    relevance and the no-aggregate rows equal what mrk_topk_merge_grows gives; the _part and _async forms give the same rows"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    c = corpora[4]
    S = aggr_sets(m)
    root2 = shapes(m)["and2"][0]
    qs = [m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10), tg.Q(m, "and2", C64, K=16, by=GROUPSORT_COUNT), Q(m, "prox2", C16, S["one"], K=8), Q(m, "and2", C64, S["four"], K=16, by=GROUPSORT_WEIGHT),
          m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10, sort=m.Sort(C64 * 32, 32)), Q(m, "one", C17, S["smm"], K=4), m.Query(shapes(m)["one"][0], ranker=m.SPH_RANK_BM25, max_matches=1024)]
    qs = [c.globalize(q) for q in qs]
    nq, NS = len(qs), 3
    dev_rows = export(batch, hip, c.segs[NS], qs, want_status=[[0, 0, 0, 0, 0, -2, 0]] * NS)
    lists = hip.to_host(dev_rows, (NS, nq, RW))
    got = merge(ctx, hip, dev_rows, NS, nq)
    assert np.array_equal(got, mdist.merge_arows_np(lists, 1024))
    for qi in (2, 3):
        assert not amc.check_merged(mdist, qs[qi], matches(orc, c, qs[qi]), got[qi], ("mixed", qi), True)
    for row in list(lists[:, 4]) + [got[4]]:  # the sorted query: declined under spec words 0, in every list and merged
        assert amc.is_empty(row, amc.DECLINED, 0, 0)
    for row in list(lists[:, 5]) + [got[5]]:  # over the limit while it ran: declined under its own two spec words
        assert amc.is_empty(row, amc.DECLINED, amc.spec_of(qs[5]), amc.aspec_of(qs[5]))
    # the same batch through GROUP rows: the queries with aggregates decline there; the others' words are these
    GW = m.GROW_WORDS
    grows = hip.malloc(NS * nq * GW * 8)
    for s, seg in enumerate(c.segs[NS]):
        batch.submit(seg, qs)
        batch.wait()
        batch.export_grows(grows.value + s * nq * GW * 8)
    gout = hip.malloc(nq * GW * 8)
    chk(lib.mrk_topk_merge_grows(ctx._h, grows, NS, nq, 1024, gout))
    ghost = hip.to_host(gout, (nq, GW))
    for qi in (0, 1, 4, 6):
        assert np.array_equal(got[qi, :amc.AGGR], ghost[qi, :GW - 1]) and got[qi, amc.GSPEC] == ghost[qi, GW - 1], qi
        assert not got[qi, amc.AGGR:amc.GSPEC].any() and int(got[qi, amc.ASPEC]) == 0, qi
    assert int(got[0, amc.CNT]) == min(1024, int(lists[:, 0, amc.CNT].sum())) >= 10 and int(got[6, amc.CNT]) == 1024 and int(got[1, amc.TOTAL]) == 64 and int(got[1, amc.GSPEC]) != 0
    for qi in (2, 3, 5):
        assert int(ghost[qi, G + 1]) == amc.DECLINED and int(ghost[qi, GW - 1]) == 0, "the group rows decline a query with aggregates"
    assert np.array_equal(merge(ctx, hip, dev_rows, NS, nq, form="async"), got), "_async"
    # _part: lists of stride nq, queries [1, 6) of each -> out rows [2, 7); every other row stays 0xEE
    out = hip.malloc((nq + 2) * RW * 8)
    hip.fill(out, 0xEE, (nq + 2) * RW * 8)
    chk(lib.mrk_topk_merge_arows_part(ctx._h, off(dev_rows, 1 * RW * 8), NS, nq, 2, 5, 1024, out))
    part = hip.to_host(out, (nq + 2, RW))
    assert np.array_equal(part[2:7], got[1:6])
    assert (part[:2] == EE).all() and (part[7:] == EE).all()
    hip.free()


def test_a_rerun_leaves_with_its_repaired_groups_and_aggregates(dev):
    """test_gpu_group_aggr's overflow setup: the match queue overflows, mrk_batch_wait reruns each query alone over a cleared table;
    the row exported after the wait equals the row of a run that did not overflow, and holds what mrk_batch_result_aggrs gives"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    n_docs = 200_000
    hi = m.synth_index(n_docs, [1.0, 0.9, 0.8], seed=31, skiplist_block_size=128, max_pos=12)
    seg = m.Segment(ctx, hi, rowid_base=1000)
    try:
        seg.set_attrs(tga.make_rows(n_docs))
        S = aggr_sets(m)
        hits = [Q(m, "prox2", C16, S["four"], K=8, by=GROUPSORT_COUNT), Q(m, "phrase", C64, S["one"], K=100, order=0), Q(m, "sph04_3", C2, S["smm"], K=2), Q(m, "prox2", C17, S["one"], K=4),
                tg.Q(m, "prox2", C16, K=8), m.Query(shapes(m)["prox2"][0], ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=9)]
        status = [[0, 0, 0, -2, 0, 0]]
        res = []
        with Settings(ctx, mq_max_chunks=1):
            a = hip.to_host(export(batch, hip, [seg], hits, want_status=status), (len(hits), RW))
            assert batch.stats()["n_rerun"] > 0
        b = hip.to_host(export(batch, hip, [seg], hits, want_status=status, results=res), (len(hits), RW))
        assert batch.stats()["n_rerun"] == 0
        assert np.array_equal(a, b)
        assert not (b[[0, 1, 2, 4, 5], amc.TOTAL] & np.uint64(amc.RERUN | amc.DECLINED)).any() and b[:3, amc.CNT].all()
        assert amc.is_empty(b[3], amc.DECLINED, amc.spec_of(hits[3]), amc.aspec_of(hits[3])) and int(b[0, amc.TOTAL]) == 16
        for qi in (0, 1, 2):
            assert int(a[qi, amc.ASPEC]) == amc.aspec_of(hits[qi])
            same_as_result(mdist, a[qi], res[0][qi], ("rerun", qi), rowid_base=1000)
    finally:
        seg.close()
        hip.free()


@pytest.mark.parametrize("part", [1, 0])
def test_shard_exchange_arows_one_rank(part):
    """mrk_shard_exchange_arows at world_size 1 over RCCL (exchange_self_rccl), partitioned and all-gather, in a fresh process"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(here, "dist_aggr_exchange_worker.py"), str(part)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "aggr exchange ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
