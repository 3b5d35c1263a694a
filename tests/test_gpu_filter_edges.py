"""GPU: row_passes_filters / weight_passes_filters (csrc/mrk_dev.h) at their edges -- the crafted rows, blob pool and cases of
filter_edges_common.py, the device against the oracle (which test_filter_edges_cpu.py pins on a plain model of the reference), bit for
bit: rowids, weights, total_found.  max_matches = 1000 >= the docs of the corpus, so every row is compared.  Every case runs through
every route that reaches the filter, one batch per route and segment, on the 8-field corpus N and its 32-field twin W:

    single   keyword A (in every doc), BM25                      and2     A B, BM25
    tree     (A | C) -D, BM25                                     phrase   "A B", PROXIMITY_BM25
    and5     A B C D F, PROXIMITY_BM25: the generic evaluator     order    A, ORDER BY an attribute DESC, weight DESC
    cutoff   A, cutoff 40                                         dead     A, with a dead-row map

The weight-filter cases (negative field weights: weights on both sides of 0) run under BM25 (the weight is final in scan_pk_kernel)
and under PROXIMITY_BM25 (rank_kernel)."""
import dataclasses

import numpy as np
import pytest

import filter_edges_common as C
from sorted_expect import expected_sort
from test_gpu_parity import orc_index_of, to_orc

pytestmark = pytest.mark.gpu

ROUTES = ["single", "and2", "tree", "phrase", "and5", "order", "cutoff", "dead"]
CUTOFF = 40


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    segs = {}
    yield m, ctx, batch, segs
    for seg in segs.values():
        seg.close()
    batch.close()
    ctx.close()


def segment_on(dev, name):
    m, ctx, _, segs = dev
    if name not in segs:
        rows, pool = C.attr_rows()
        seg = segs[name] = m.Segment(ctx, C.segment(name))
        seg.set_attrs(rows)
        seg.set_blobs(pool, C.N_BLOB, rows)
    return segs[name]


_oracle = {}


def oracle_index(orc, name):
    if name not in _oracle:
        oi = _oracle[name] = orc_index_of(orc, C.segment(name))
        oi.attrs, oi.blobs = C.attr_rows()
    return _oracle[name]


def kw(m, t):
    return m.XQNode.keyword(t, t + 1)


def root_of(m, route):
    A, B, Cc, D, F = (kw(m, t) for t in (C.T_A, C.T_B, C.T_C, C.T_D, C.T_F))
    if route in ("and2", "w_prox"):
        return m.XQNode.AND(A, B)
    if route == "tree":
        return m.XQNode(m.SPH_QUERY_ANDNOT, [m.XQNode(m.SPH_QUERY_OR, [A, Cc]), D])
    if route == "phrase":
        return m.XQNode(m.SPH_QUERY_PHRASE, [A, B])
    if route == "and5":
        return m.XQNode.AND(A, B, Cc, D, F)
    return A


def query(m, route, n_fields, filters=None, weight_filters=None):
    hit_ranker = route in ("phrase", "and5", "w_prox")
    q = m.Query(root_of(m, route), ranker=m.SPH_RANK_PROXIMITY_BM25 if hit_ranker else m.SPH_RANK_BM25, max_matches=1000,
                field_weights=C.field_weights(n_fields), filters=[m.Filter(**f) for f in filters] if filters else None,
                weight_filters=[m.Filter(**f) for f in weight_filters] if weight_filters else None)
    if route == "order":
        q.sort = m.Sort(C.LOC["sort"][0], 32, desc=True, then_weight=1)
    if route == "cutoff":
        q.cutoff = CUTOFF
    return q


def compare(orc, oi, q, g, what):
    assert g.status == 0, (what, g.status)
    if q.sort is not None:
        r, w, _, total = expected_sort(orc, oi, q, C.attr_rows()[0], C.N_DOCS)
    else:
        want = to_orc(orc, q).run(oi)
        r, w, total = want.rowid, want.weight, want.total_found
    assert g.total_found == total <= q.max_matches, (what, g.total_found, total)
    assert np.array_equal(g.rowid, r), (what, g.rowid[:8], r[:8])
    assert np.array_equal(g.weight, w), (what, g.weight[:8], w[:8])
    return len(r)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", C.SEGMENT_IDS)
def test_every_case_on_route(orc, dev, name, route):
    m, ctx, batch, _ = dev
    n_fields = dict(C.SEGMENTS)[name]
    seg, oi = segment_on(dev, name), oracle_index(orc, name)
    cases = C.cases()
    qs = [query(m, route, n_fields, filters=c.filters) for c in cases]
    assert len(qs) <= batch.max_queries
    try:
        if route == "dead":
            seg.set_dead_rows(C.dead_map())
            oi.dead_rows = C.dead_map()
        got = batch.search(seg, qs)
        st = batch.stats()
        assert st["packed"] == 1 and st["n_rerun"] == 0, st
        if route == "and5":
            assert st["mq_chunks"][2] > 0, st["mq_chunks"]
        n_rows = [compare(orc, oi, q, g, (name, route, c.name)) for c, q, g in zip(cases, qs, got)]
    finally:
        if route == "dead":
            seg.set_dead_rows(None)
            oi.dead_rows = None
    # the route's own docs hold both answers for nearly every case: the batch compared passing and failing rows
    full = to_orc(orc, dataclasses.replace(query(m, route, n_fields), cutoff=0, sort=None)).run(oi).total_found
    assert sum(1 for n in n_rows if 0 < n < full) >= len(cases) - len(C.TRIVIAL) - 2, (full, n_rows)


@pytest.mark.parametrize("route", ["w_bm25", "w_prox"])
@pytest.mark.parametrize("name", C.SEGMENT_IDS)
def test_weight_filters_on_route(orc, dev, name, route):
    m, ctx, batch, _ = dev
    n_fields = dict(C.SEGMENTS)[name]
    seg, oi = segment_on(dev, name), oracle_index(orc, name)
    full = to_orc(orc, query(m, route, n_fields)).run(oi)
    wcases = C.weight_cases(full.weight)
    qs = [query(m, route, n_fields, filters=fl, weight_filters=wf) for _, fl, wf in wcases]
    got = batch.search(seg, qs)
    st = batch.stats()
    assert st["packed"] == 1 and st["n_rerun"] == 0, st
    if route == "w_prox":
        assert st["mq_chunks"][0] > 0, st["mq_chunks"]  # the weights were made by the rank pass: rank_kernel filtered them
    else:
        assert st["mq_chunks"] == [0, 0, 0], st["mq_chunks"]  # no rank pass: scan_pk_kernel filtered them
    for (wname, _, _), q, g in zip(wcases, qs, got):
        n = compare(orc, oi, q, g, (name, route, wname))
        assert 0 < n < full.total_found, (wname, n)


def test_bad_locators_are_refused_before_a_launch(dev):
    m, ctx, batch, _ = dev
    seg = segment_on(dev, "N")
    A = kw(m, C.T_A)
    last = C.STRIDE * 32
    bad = [m.Filter(C.D_BFA * 32 + 30, 4, values=[1]),            # a bit field across a dword
           m.Filter(C.D_I64 * 32 - 16, 64, min=0, max=1),         # an unaligned 64-bit locator
           m.Filter(last - 32, 64, min=0, max=1),                 # 64 bits that end past the row
           m.Filter(last, 32, values=[1]),                        # a dword past the row
           m.Filter(last - 16, 17, values=[1]),
           m.Filter(C.D_FLT * 32, 16, fmin=0.0, fmax=1.0)]        # a float filter over 16 bits
    for f in bad:
        with pytest.raises(m.MrkError, match="filter locator|float filter") as e:
            batch.search(seg, [m.Query(A, filters=[f])])
        assert e.value.code == -1, (f, e.value)  # MRK_E_INVAL
    ok = batch.search(seg, [m.Query(A, filters=[m.Filter(last - 64, 64, min=0, max=1)])])[0]  # the row's last two dwords are fine
    assert ok.status == 0


def test_the_pool_belongs_to_the_rows_it_was_walked_with(orc, dev):
    """mrk_segment_set_blobs walks the rows the segment holds and refuses other ones; mrk_segment_set_attrs drops the pool.  The second
    row set is a permutation of the first: every blob offset in it was walked, whatever the library does with it."""
    m, ctx, batch, _ = dev
    rows, pool = C.attr_rows()
    perm = np.ascontiguousarray(rows[::-1])
    assert not np.array_equal(perm[:, C.D_BLOB], rows[:, C.D_BLOB]) and sorted(perm[:, C.D_BLOB].tolist()) == sorted(rows[:, C.D_BLOB].tolist())
    oi = orc_index_of(orc, C.segment("N"))
    oi.blobs = pool
    mva = query(m, "single", 8, filters=[C.MV("m64", values=[C.I64_MIN, -1])])
    plain = query(m, "single", 8, filters=[C.F("u32", min=1, max=1 << 31)])
    seg = m.Segment(ctx, C.segment("N"))
    try:
        with pytest.raises(m.MrkError, match="set_attrs"):  # no rows yet
            seg.set_blobs(pool, C.N_BLOB, rows)
        seg.set_attrs(rows)
        with pytest.raises(m.MrkError, match="rows differ"):
            seg.set_blobs(pool, C.N_BLOB, perm)
        with pytest.raises(m.MrkError):
            seg.set_blobs(pool, C.N_BLOB, rows[:, :4])  # another stride
        assert batch.search(seg, [mva])[0].status == -2  # nothing was installed by the refused calls
        seg.set_blobs(pool, C.N_BLOB, rows)
        oi.attrs = rows
        compare(orc, oi, mva, batch.search(seg, [mva])[0], "rows")
        seg.set_attrs(perm)  # the pool leaves with the rows it was walked with
        oi.attrs = perm
        got = batch.search(seg, [mva, plain])
        assert got[0].status == -2
        compare(orc, oi, plain, got[1], "plain filter over the new rows")
        seg.set_blobs(pool, C.N_BLOB, perm)
        compare(orc, oi, mva, batch.search(seg, [mva])[0], "permuted rows")
    finally:
        seg.close()
