"""GPU: the weight in FRONT of the sorter's order (Order.weight_first: ORDER BY weight() DESC, attr | weight() ASC [, attr]) against
the oracle.  The expected answer is the oracle's result for the same query with max_matches = number of docs (every match with its
weight), ordered on the host by numpy -- lexsort over (weight in the asked direction, the parts, rowid ascending) with the parts as
numpy reads the raw rows -- and cut to K (weight_first_expect.py, itself held against the reference's recorded weight-first results by
test_weight_first_cpu.py).  Every comparison is exact: rowids, weights, order_key and total_found."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from helpers import synth_postings
from sorted_expect import all_matches
from test_gpu_order import Hip
from test_gpu_order import check as check_other
from test_gpu_parity import kw, orc_index_of, to_orc
from test_gpu_sort import AUX, BITS, FLT, TS
from test_gpu_sort import make_rows as make_rows4
from test_gpu_sort import random_queries as random_sort_queries
from weight_first_expect import order_of

pytestmark = pytest.mark.gpu

BIG, RID64, STRIDE = 4, 6, 8  # dwords behind test_gpu_sort's four: a bigint of both signs, the rowid as a bigint (low dword first)


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    yield m, ctx, batch
    batch.close()
    ctx.close()


def make_rows(rng, n_docs):
    rows = np.zeros((n_docs, STRIDE), np.uint32)
    rows[:, :4] = make_rows4(rng, n_docs)  # timestamps | bit-fields | floats with -0.0, negatives, infinities | rowid % 10
    big = (rng.integers(-3, 4, n_docs).astype(np.int64) << 32) + rng.integers(0, 1 << 32, n_docs, dtype=np.uint64).astype(np.int64)
    edge = rng.random(n_docs) < 0.02
    big[edge] = rng.choice(np.array([np.iinfo(np.int64).min, -1, 0, 1, np.iinfo(np.int64).max], np.int64), int(edge.sum()))
    rows[:, BIG:BIG + 2] = big.view(np.uint32).reshape(n_docs, 2)
    rows[:, RID64:RID64 + 2] = np.arange(n_docs, dtype=np.int64).view(np.uint32).reshape(n_docs, 2)
    return rows


def orders(m):
    """every accepted shape under both weight directions: uint, timestamp, a 3-bit bit-field, float, INT64 (both directions), two parts
    with mixed directions; and the weight ascending alone"""
    P = m.OrderPart
    shapes = [[P(AUX * 32, 32, desc=False)], [P(TS * 32, 32, desc=True)], [P(BITS * 32 + 3, 3, desc=True)], [P(FLT * 32, 32, desc=False, kind=m.SORTKEY_FLOAT)],
              [P(BIG * 32, 64, desc=True, kind=m.SORTKEY_INT64)], [P(BIG * 32, 64, desc=False, kind=m.SORTKEY_INT64)],
              [P(BITS * 32 + 3, 3, desc=True), P(TS * 32, 32, desc=False)], [P(FLT * 32, 32, desc=True, kind=m.SORTKEY_FLOAT), P(AUX * 32, 32, desc=False)]]
    return [m.Order(s, weight_first=wf) for wf in (1, 2) for s in shapes] + [m.Order([], weight_first=2)]


class Expect:
    """the oracle's full answer per base query, computed once and shared by every order and K asked of it"""

    def __init__(self, orc, oi, rows, n_docs):
        self.orc, self.oi, self.rows, self.n_docs, self.full = orc, oi, rows, n_docs, {}

    def matches(self, q):
        key = (id(q.root), q.ranker, q.index_weight, tuple(q.field_weights or ()), id(q.filters), id(q.weight_filters), id(self.oi.dead_rows) if hasattr(self.oi, "dead_rows") else 0)
        if key not in self.full:
            self.full[key] = (q.root, all_matches(self.orc, self.oi, q, self.n_docs))  # (the root is kept alive: its id is the key)
        return self.full[key][1]

    def check(self, queries, got, what=""):
        for i, (q, g) in enumerate(zip(queries, got)):
            assert g.status == 0, (what, i, q.order, "no query of this test may be declined")
            if q.order is None or not q.order.weight_first:
                check_other(self.orc, self.oi, self.rows, self.n_docs, [q], [g], what)
                continue
            full = self.matches(q)
            order, okey = order_of(full.weight, full.rowid, self.rows, q.order)
            order = order[: q.max_matches]
            assert g.total_found == full.total_found, (what, i, g.total_found, full.total_found)
            assert np.array_equal(g.rowid, full.rowid[order]), (what, i, q.order, q.ranker, q.max_matches, g.rowid[:8], full.rowid[order][:8])
            assert np.array_equal(g.weight, full.weight[order]), (what, i, q.order, g.weight[:8], full.weight[order][:8])
            assert g.sort_key is None
            if okey is None:
                assert g.order_key is None  # (no parts: nothing of the row is part of the order)
            else:
                assert g.order_key is not None and g.order_key.dtype == np.uint64 and np.array_equal(g.order_key, okey[order]), (what, i, q.order)


def same(a, b):
    return a.status == b.status == 0 and a.total_found == b.total_found and np.array_equal(a.rowid, b.rowid) and np.array_equal(a.weight, b.weight)


def test_deep_weight_classes_are_ordered_by_the_attribute(orc, dev):
    """200 000 docs, two keywords in half of them each: under BM25 their IDFs are next to nothing and the weight is the matched fields'
    alone -- a handful of classes thousands of rows deep.  More than 2048 matches share the K-th row's weight (asserted), so the
    selection kernel refills and re-sorts its 2048-candidate buffer with the attribute deciding.  A third, rarer keyword spreads the
    weights over more classes."""
    m, ctx, batch = dev
    n_docs = 200_000
    hi = m.synth_index(n_docs, [0.5, 0.5, 0.3], seed=11, n_fields=2, skiplist_block_size=128, max_pos=16)
    rng = np.random.default_rng(5)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    oi.attrs = rows
    E = Expect(orc, oi, rows, n_docs)
    try:
        seg.set_attrs(rows)
        deep, spread = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2)), m.XQNode.AND(kw(m, 0, 1), kw(m, 2, 2))
        qs = [m.Query(deep, ranker=m.SPH_RANK_BM25, max_matches=K, order=o) for K in (1, 10, 1000) for o in orders(m)]
        full = E.matches(qs[0])
        w = np.sort(full.weight.astype(np.int64))
        for K in (1, 10, 1000):  # the K-th row's weight class, from either end
            for kth in (w[::-1][K - 1], w[K - 1]):
                assert int((w == kth).sum()) > 2048, (K, int(kth), int((w == kth).sum()))
        qs += [m.Query(spread, ranker=m.SPH_RANK_BM25, max_matches=K, order=o) for K in (10, 1000) for o in orders(m)]
        got = batch.search(seg, qs)
        st = batch.stats()
        assert st["packed"] == 1 and st["n_rerun"] == 0
        E.check(qs, got, "deep classes")
    finally:
        seg.close()


@pytest.mark.parametrize("n_fields", [3, 12])
def test_every_sort_instance_vs_oracle(orc, dev, n_fields):
    """Each SORT instance of the scan and rank kernels at least once under a weight-first order: NONE / BM25 over AND and OR trees
    (the weight is final in the scan), PROXIMITY_BM25 / SPH04 over a tree (rank_kernel<0>), a PHRASE (<1>), five keywords (<2>, the
    generic evaluator); 12 fields: the WIDE instances.  Negative field weights, index_weight, an attribute filter, a weight filter,
    dead rows.  Then mixed batches: the relevance and attribute-first queries answer as in a batch without the weight-first ones."""
    m, ctx, batch = dev
    rng = np.random.default_rng(977 + n_fields)
    n_docs, nt = 30000, 8
    W, R, H = synth_postings(rng, n_docs, [0.9, 0.6, 0.6, 0.4, 0.4, 0.3, 0.2, 0.2], n_fields=n_fields, max_pos=10)
    hi = m.index_from_hits(W, R, H, n_terms=nt, total_docs=n_docs, n_fields=n_fields)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    oi.attrs = rows
    try:
        seg.set_attrs(rows)
        X = m.XQNode
        AND2, OR2 = X.AND(kw(m, 1, 1), kw(m, 2, 2)), X(m.SPH_QUERY_OR, [kw(m, 3, 1), kw(m, 5, 2)])
        TREE = X.AND(X(m.SPH_QUERY_OR, [kw(m, 1, 1), kw(m, 4, 2)]), X(m.SPH_QUERY_ANDNOT, [kw(m, 0, 3), kw(m, 6, 4)]))
        PHRASE = X(m.SPH_QUERY_PHRASE, [kw(m, 0, 1), kw(m, 1, 2)])
        FIVE = X.AND(*[kw(m, j, j + 1) for j in range(5)])
        ONE = kw(m, 2, 1)
        neg = [3, -7, 2] + [1, -2] * ((n_fields - 3 + 1) // 2)
        flt = [m.Filter(AUX * 32, 32, values=[1, 3, 5, 7, 8])]
        wflt = [m.Filter(0, 0, min=1500, max=1 << 30)]
        base = [(ONE, m.SPH_RANK_NONE, {}), (AND2, m.SPH_RANK_NONE, {}), (OR2, m.SPH_RANK_NONE, {}), (ONE, m.SPH_RANK_BM25, {}), (AND2, m.SPH_RANK_BM25, {}),
                (OR2, m.SPH_RANK_BM25, {}), (TREE, m.SPH_RANK_BM25, {}), (AND2, m.SPH_RANK_PROXIMITY_BM25, {}), (TREE, m.SPH_RANK_PROXIMITY_BM25, {}),
                (TREE, m.SPH_RANK_SPH04, {}), (PHRASE, m.SPH_RANK_PROXIMITY_BM25, {}), (PHRASE, m.SPH_RANK_BM25, {}), (FIVE, m.SPH_RANK_PROXIMITY_BM25, {}),
                (FIVE, m.SPH_RANK_SPH04, {}), (AND2, m.SPH_RANK_BM25, {"field_weights": neg[:n_fields]}), (TREE, m.SPH_RANK_PROXIMITY_BM25, {"field_weights": neg[:n_fields]}),
                (OR2, m.SPH_RANK_BM25, {"index_weight": 3}), (AND2, m.SPH_RANK_PROXIMITY_BM25, {"index_weight": 3}), (OR2, m.SPH_RANK_BM25, {"filters": flt}),
                (TREE, m.SPH_RANK_SPH04, {"filters": flt}), (OR2, m.SPH_RANK_BM25, {"weight_filters": wflt}), (AND2, m.SPH_RANK_PROXIMITY_BM25, {"weight_filters": wflt})]
        O = orders(m)
        qs = []
        for i, (root, ranker, extra) in enumerate(base):  # three orders per base query, walking through all of them, K walking too
            for j in range(3):
                qs.append(m.Query(root, ranker=ranker, max_matches=[1, 10, 1000][(i + j) % 3], order=O[(3 * i + j) % len(O)], **extra))
        E = Expect(orc, oi, rows, n_docs)
        got = batch.search(seg, qs)
        assert batch.stats()["packed"] == 1 and batch.stats()["n_rerun"] == 0
        E.check(qs, got, f"fields {n_fields}")
        neg_q = [g for q, g in zip(qs, got) if q.field_weights is not None and q.ranker == m.SPH_RANK_BM25]
        assert neg_q and any((g.weight < 0).any() for g in neg_q)  # (the negative field weights did make negative weights)
        # mixed batches: relevance | attribute-first | weight-first
        S = random_sort_queries(m, rng, nt, 12)
        rel = [dataclasses.replace(q, sort=None) for q in random_sort_queries(m, rng, nt, 12)]
        others = rel + S
        mixed = [q for trio in zip(qs[:24], others, others[6:] + others[:6]) for q in trio]
        only_others = batch.search(seg, others)
        first = batch.search(seg, mixed)
        second = batch.search(seg, mixed)  # the same batch again: state carried between submits
        E.check(mixed, first, f"fields {n_fields} mixed")
        solo = {id(q): g for q, g in zip(others, only_others)}
        for q, x, y in zip(mixed, first, second):
            assert same(x, y) and (x.order_key is None or np.array_equal(x.order_key, y.order_key))
            if q.order is None:
                wq = solo[id(q)]
                assert same(x, wq) and (x.sort_key is None) == (wq.sort_key is None) and (x.sort_key is None or np.array_equal(x.sort_key, wq.sort_key))
        for x, y in zip(only_others, batch.search(seg, others)):  # and once more without them
            assert same(x, y)
        # dead rows
        dead = np.zeros((n_docs + 31) // 32, np.uint32)
        killed = rng.choice(n_docs, n_docs // 7, replace=False).astype(np.uint32)
        np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
        seg.set_dead_rows(dead)
        oi.dead_rows = dead
        Expect(orc, oi, rows, n_docs).check(qs[:42], batch.search(seg, qs[:42]), f"fields {n_fields} dead rows")
    finally:
        seg.close()


def test_rowid_column_behind_the_weight_is_relevance(dev):
    """No oracle: weight DESC, then an INT64 column that holds the rowid, ascending, IS the relevance order -- row for row."""
    m, ctx, batch = dev
    rng = np.random.default_rng(41)
    n_docs, nt = 50000, 6
    W, R, H = synth_postings(rng, n_docs, [0.7, 0.5, 0.4, 0.3, 0.2, 0.1], n_fields=3, max_pos=10)
    hi = m.index_from_hits(W, R, H, n_terms=nt, total_docs=n_docs, n_fields=3)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    try:
        seg.set_attrs(rows)
        rel = [dataclasses.replace(q, sort=None) for q in random_sort_queries(m, rng, nt, 36)]
        o = m.Order([m.OrderPart(RID64 * 32, 64, desc=False, kind=m.SORTKEY_INT64)], weight_first=1)
        got_rel, got_wf = batch.search(seg, rel), batch.search(seg, [dataclasses.replace(q, order=o) for q in rel])
        for q, a, b in zip(rel, got_rel, got_wf):
            assert same(a, b), (q.ranker, q.max_matches)
            assert np.array_equal(b.order_key, b.rowid.astype(np.uint64))
    finally:
        seg.close()


def test_overflowing_weight_bin_is_rerun_exactly(orc, dev):
    """Exact or loud: one keyword in ~95 % of 1.2 M docs under ranker NONE -- every match weighs 1 and lands in ONE bin, more than the
    candidate list's 2^20 slots hold.  The query is rerun alone and comes back exact (a 10-valued part decides); through a batch with
    a standing order-row destination too, where its row leaves MRK_ROW_DECLINED."""
    m, ctx, batch = dev
    from manticoresearch_amd import _lib
    from manticoresearch_amd import dist as mdist

    lib, chk = _lib.lib(), _lib.check
    K1 = _lib.MRK_MAX_K
    n_docs = 1_200_000
    hi = m.synth_index(n_docs, [0.95, 0.3], seed=7, skiplist_block_size=128, max_pos=16)
    rng = np.random.default_rng(13)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    oi.attrs = rows
    hip = Hip()
    b2 = m.Batch(ctx, 8)
    try:
        seg.set_attrs(rows)
        q = m.Query(kw(m, 0, 1), ranker=m.SPH_RANK_NONE, max_matches=1000, order=m.Order([m.OrderPart(AUX * 32, 32, desc=True)], weight_first=1))
        plain = m.Query(kw(m, 1, 1), ranker=m.SPH_RANK_BM25, max_matches=100)
        E = Expect(orc, oi, rows, n_docs)
        got = batch.search(seg, [q])
        st = batch.stats()
        print(f"overflow: total_found {got[0].total_found}, n_cands {st['n_cands']}, n_rerun {st['n_rerun']}")
        assert got[0].total_found > 2 ** 20 and st["n_rerun"] == 1 and got[0].status == 0
        E.check([q], got, "overflow")
        dst = hip.malloc(2 * m.OROW_WORDS * 8)
        hip.fill(dst, 0xEE, 2 * m.OROW_WORDS * 8)
        chk(lib.mrk_batch_set_orows_dst(b2._h, dst))
        b2.submit(seg, [plain, q])
        b2.wait()
        got2 = b2.results()
        assert b2.stats()["n_rerun"] == 1
        chk(lib.mrk_batch_set_orows_dst(b2._h, None))
        E.check([plain, q], got2, "overflow, standing order rows")
        orow = hip.to_host(dst, (2, m.OROW_WORDS))
        assert int(orow[1, K1 + 1]) == mdist.ROW_DECLINED and int(orow[1, K1]) == 0 and not orow[1, :K1].any() and not orow[1, K1 + 2:].any()
        assert int(orow[0, K1]) == len(got2[0].rowid) and int(orow[0, K1 + 1]) == got2[0].total_found and int(orow[0, -1]) == 0
    finally:
        hip.free()
        b2.close()
        seg.close()


def test_exchange_rows_decline_a_weight_first_query(dev):
    """No exchange row carries the weight's position yet: a weight-first query leaves in narrow, wide and order rows -- exported and
    through standing destinations -- with MRK_ROW_DECLINED, zero count, zero keys and spec word 0; the other queries' rows equal
    those of the batch without the weight-first queries, word for word."""
    m, ctx, batch = dev
    from manticoresearch_amd import _lib
    from manticoresearch_amd import dist as mdist

    lib, chk = _lib.lib(), _lib.check
    K1 = _lib.MRK_MAX_K
    rng = np.random.default_rng(37)
    n_docs, nt = 20000, 6
    W, R, H = synth_postings(rng, n_docs, [0.7, 0.5, 0.4, 0.3, 0.2, 0.1], n_fields=3, max_pos=10)
    hi = m.index_from_hits(W, R, H, n_terms=nt, total_docs=n_docs, n_fields=3)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    hip = Hip()
    b2 = m.Batch(ctx, 64)
    try:
        seg.set_attrs(rows)
        S = random_sort_queries(m, rng, nt, 6)
        rel = [dataclasses.replace(q, sort=None) for q in random_sort_queries(m, rng, nt, 6)]
        big = [dataclasses.replace(q, sort=None, order=m.Order([m.OrderPart(BIG * 32, 64, kind=m.SORTKEY_INT64)])) for q in random_sort_queries(m, rng, nt, 2)]
        O = orders(m)
        wfq = [dataclasses.replace(q, sort=None, order=O[(5 * i) % len(O)]) for i, q in enumerate(random_sort_queries(m, rng, nt, 7))]
        others = [q for pair in zip(rel, S) for q in pair] + big
        mixed, is_wf = [], []
        for i, q in enumerate(others):
            mixed.append(q), is_wf.append(False)
            if i % 2 == 0:
                mixed.append(wfq[i // 2]), is_wf.append(True)
        n_m = len(mixed)
        widths = {"rows": m.ROW_WORDS, "srows": m.SROW_WORDS, "orows": m.OROW_WORDS}
        bufs = {k: hip.malloc(n_m * wd * 8) for k, wd in widths.items()}

        def rows_of(qs, kind, standing):
            n, wd = len(qs), widths[kind]
            setter = getattr(lib, f"mrk_batch_set_{kind}_dst")
            hip.fill(bufs[kind], 0xEE, n * wd * 8)
            if standing:
                chk(setter(b2._h, bufs[kind]))
            b2.submit(seg, qs)
            b2.wait()
            assert [g.status for g in b2.results()] == [0] * n and b2.stats()["n_rerun"] == 0
            if standing:
                chk(setter(b2._h, None))
            else:
                chk(getattr(lib, f"mrk_batch_export_{kind}")(b2._h, bufs[kind]))
            return hip.to_host(bufs[kind], (n, wd))

        keep = [i for i, w in enumerate(is_wf) if not w]
        for kind in widths:
            for standing in (False, True):
                base, got = rows_of(others, kind, standing), rows_of(mixed, kind, standing)
                assert np.array_equal(got[keep], base), (kind, standing)
                for i, w in enumerate(is_wf):
                    if w:
                        assert int(got[i, K1 + 1]) == mdist.ROW_DECLINED and int(got[i, K1]) == 0 and not got[i, :K1].any(), (kind, standing, i)
                        assert not got[i, K1 + 2:].any(), (kind, standing, i)  # (no mapped keys, spec word 0)
    finally:
        hip.free()
        b2.close()
        seg.close()


def test_refusals_are_loud(dev):
    m, ctx, batch = dev
    from manticoresearch_amd import _lib

    rng = np.random.default_rng(3)
    n_docs = 3000
    W, R, H = synth_postings(rng, n_docs, [0.6, 0.4], n_fields=3, max_pos=8)
    hi = m.index_from_hits(W, R, H, n_terms=2, total_docs=n_docs, n_fields=3)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
    plain = m.Query(root, ranker=m.SPH_RANK_BM25)
    Q = lambda o, **kwa: m.Query(root, ranker=m.SPH_RANK_BM25, order=o, **kwa)
    ts = m.OrderPart(TS * 32, 32)
    try:
        # no attribute rows yet: the weight ascending alone needs none, a part does
        got = batch.search(seg, [plain, Q(m.Order([], weight_first=2)), Q(m.Order([ts], weight_first=1))])
        assert [g.status for g in got] == [0, 0, -2]
        rel = got[0]
        assert rel.total_found == len(rel.rowid) <= 1000 and got[1].total_found == rel.total_found and got[1].order_key is None
        order = np.lexsort((rel.rowid, rel.weight.astype(np.int64)))  # (every match is in the list: the relevance answer, weight ascending)
        assert np.array_equal(got[1].rowid, rel.rowid[order]) and np.array_equal(got[1].weight, rel.weight[order])
        seg.set_attrs(rows)
        got = batch.search(seg, [plain, Q(m.Order([ts], weight_first=1), cutoff=50), Q(m.Order([ts], weight_first=1)), Q(m.Order([m.OrderPart(-1, 0)], weight_first=2))])
        assert [g.status for g in got] == [0, -2, 0, -2]
        # what the marshalling refuses itself: a direction that is none, the weight in front AND behind
        for bad in (m.Order([ts], weight_first=3), m.Order([ts], weight_first=-1), m.Order([ts], weight_first=0x101), m.Order([ts], weight_first=1, then_weight=1),
                    m.Order([ts], weight_first=2, then_weight=2)):
            with pytest.raises(ValueError):
                batch.search(seg, [plain, Q(bad)])
        # what the library refuses: MRK_E_INVAL fails the submit
        for bad in (m.Order([], weight_first=1), m.Order([], weight_first=0), m.Order([ts] * 3, weight_first=1),
                    m.Order([m.OrderPart(BIG * 32, 64, kind=m.SORTKEY_INT64), ts], weight_first=1), m.Order([ts], then_weight=0x100), m.Order([ts], then_weight=0x103)):
            with pytest.raises(_lib.MrkError) as e:
                batch.search(seg, [plain, Q(bad)])
            assert e.value.code == _lib.MRK_E_INVAL, e.value
        assert batch.search(seg, [plain])[0].status == 0
    finally:
        seg.close()
