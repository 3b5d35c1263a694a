"""GPU: aggregates of a grouped query (Query.aggrs; mrk_batch_submit_aggr) against group_aggr_expect -- group_expect's numpy model of
the reference's grouping sorter plus per-group SUM / MIN / MAX over the oracle's full match set, itself pinned on the reference's
recorded results (tests/test_group_aggr_cpu.py).  Every comparison is bit for bit: head rowid, head weight, group key, @count,
total_found, order and every aggregate value.  A query whose model answer is DECLINED (more than 4 * max_matches distinct keys) must
come back MRK_E_UNSUPPORTED with the limit in the message; any other decline is a failure.

Columns of a row (dwords): test_gpu_group's fourteen, then  BIG values >= 0xF0000000 (a 32-bit sum wraps within a group, the widened
sum passes 2^32) | ONES all 0xFFFFFFFF | ZERO all 0 (MIN / MAX whose mapped value equals the accumulator's empty word) | I64 an aligned
signed 64 with negatives, INT64_MIN (row 5) and INT64_MAX (row 6: another group of every column grouped by here) | UNIT all 1 (SUM =
@count: sums tie wherever counts do, and the head's rowid decides)."""
import dataclasses

import numpy as np
import pytest

import test_gpu_group as tg
from group_aggr_expect import expected_group_aggr
from group_expect import DECLINED, GROUPSORT_COUNT, GROUPSORT_KEY, GROUPSORT_WEIGHT
from helpers import synth_postings
from test_gpu_group import AUX, BITS, C1, C2, C16, C17, C64, C65, C4096, C4097, E_UNSUPPORTED, N_DOCS, PROBS, Settings, last_error, scr, shapes
from test_gpu_parity import orc_index_of, to_orc

pytestmark = pytest.mark.gpu

BIG, ONES, ZERO, I64, I64HI, UNIT = range(tg.STRIDE, tg.STRIDE + 6)
STRIDE = tg.STRIDE + 6
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def make_rows(n_docs):
    r = np.arange(n_docs, dtype=np.uint64)
    rows = np.zeros((n_docs, STRIDE), np.uint32)
    rows[:, : tg.STRIDE] = tg.make_rows(n_docs)
    rows[:, BIG] = np.uint32(0xF0000000) | (scr(r) >> np.uint32(5))
    rows[:, ONES] = 0xFFFFFFFF
    v = (r * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)).astype(np.uint64)  # (wraps: about half are negative)
    if n_docs > 6:
        v[5], v[6] = np.uint64(1 << 63), np.uint64((1 << 63) - 1)
    rows[:, I64], rows[:, I64HI] = (v & np.uint64(0xFFFFFFFF)).astype(np.uint32), (v >> np.uint64(32)).astype(np.uint32)
    rows[:, UNIT] = 1
    return rows


class Corpus:
    def __init__(self, m, ctx, orc, n_fields, rowid_base=0, seed=5, hi=None):
        if hi is None:
            rng = np.random.default_rng(seed + n_fields)
            W, R, H = synth_postings(rng, N_DOCS, PROBS, n_fields=n_fields, max_pos=6)
            hi = m.index_from_hits(W, R, H, n_terms=len(PROBS), total_docs=N_DOCS, n_fields=n_fields)
        self.hi, self.n_docs = hi, hi.total_docs
        self.rows = make_rows(self.n_docs)
        self.seg = m.Segment(ctx, self.hi, rowid_base=rowid_base)
        self.seg.set_attrs(self.rows)
        self.oi = orc_index_of(orc, self.hi)
        self.oi.attrs = self.rows

    def close(self):
        self.seg.close()


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    yield m, ctx, batch
    batch.close()
    ctx.close()


@pytest.fixture(scope="module")
def corpora(orc, dev):
    m, ctx, _ = dev
    cs = {4: Corpus(m, ctx, orc, 4), 17: Corpus(m, ctx, orc, 17)}
    yield cs
    for c in cs.values():
        c.close()


def aggr_sets(m):
    """name -> aggregate list: one; four of every source kind; SUM + MIN + MAX of one attribute; the edge columns"""
    A, S, MI, MA, I6 = m.Aggr, m.AGGR_SUM, m.AGGR_MIN, m.AGGR_MAX, m.SORTKEY_INT64
    return {"one": [A(S, BIG * 32, 32)],
            "four": [A(S, BIG * 32, 32, widen=True), A(MI, BIG * 32, 32), A(MA, I64 * 32, 64, kind=I6), A(S, I64 * 32, 64, kind=I6)],
            "smm": [A(S, BIG * 32, 32), A(MI, BIG * 32, 32), A(MA, BIG * 32, 32)],
            "edges": [A(MI, ONES * 32, 32), A(MA, ZERO * 32, 32), A(MI, I64 * 32, 64, kind=I6), A(MA, ONES * 32, 32, widen=True)],
            "bits": [A(S, BITS * 32 + 9, 7), A(MI, BITS * 32 + 9, 7), A(MA, BITS * 32 + 9, 7, widen=True), A(S, BITS * 32 + 5, 1)],
            "wide": [A(MI, ZERO * 32, 32, widen=True), A(S, ONES * 32, 32), A(S, ONES * 32, 32, widen=True), A(S, ZERO * 32, 32)]}


def Q(m, shape, col, aggrs, bits=32, shift=0, K=20, by=GROUPSORT_KEY, desc=True, order=-1, **kwa):
    root, ranker = shapes(m)[shape]
    return m.Query(root, ranker=ranker, max_matches=K, group=m.Group(col * 32 + shift, bits, sort_by=by, desc=desc), aggrs=aggrs, aggr_order=order, **kwa)


def check(orc, c, queries, got, what="", must=None):
    """must: per query True = the model must answer, False = must decline, None = whatever the model says.  Returns the declines."""
    n_decl = 0
    for i, (q, g) in enumerate(zip(queries, got)):
        if q.group is None:
            want = to_orc(orc, q).run(c.oi)
            assert g.status == 0 and g.group_key is None and g.aggr is None, (what, i)
            assert g.total_found == want.total_found and np.array_equal(g.rowid, want.rowid) and np.array_equal(g.weight, want.weight), (what, i)
            continue
        if q.aggrs is None:
            assert tg.check(orc, c, [q], [g], what) in (0, 1) and g.aggr is None, (what, i)
            n_decl += g.status != 0
            continue
        want = expected_group_aggr(orc, c.oi, q, c.rows, c.n_docs)
        if must is not None and must[i] is not None:
            assert (want is not DECLINED) == must[i], (what, i, "the case is not what the test designates")
        if want is DECLINED:
            n_decl += 1
            assert g.status == E_UNSUPPORTED and len(g.rowid) == 0 and g.total_found == 0 and g.group_key is None and g.aggr is None, (what, i, g.status)
            continue
        assert g.status == 0, (what, i, q.group, q.max_matches, "a device decline where the model answers")
        r, w, k, cnt, total, ag = want
        assert g.total_found == total, (what, i, g.total_found, total)
        assert np.array_equal(g.rowid, r), (what, i, q.group, q.max_matches, g.rowid[:8], r[:8])
        assert np.array_equal(g.weight, w), (what, i, g.weight[:8], w[:8])
        assert np.array_equal(g.group_key, k) and np.array_equal(g.group_count, cnt), (what, i)
        assert g.aggr is not None and g.aggr.dtype == np.uint64 and g.aggr.shape == (len(r), len(q.aggrs)), (what, i, None if g.aggr is None else g.aggr.shape)
        bad = np.argwhere(g.aggr != ag)
        assert len(bad) == 0, (what, i, "aggregate (row, column)", bad[:4].tolist(), [hex(int(g.aggr[x, y])) for x, y in bad[:4]], [hex(int(ag[x, y])) for x, y in bad[:4]])
    return n_decl


def same(x, y):
    for f in ("rowid", "weight", "sort_key", "order_key", "group_key", "group_count", "aggr"):
        a, b = getattr(x, f), getattr(y, f)
        if (a is None) != (b is None) or (a is not None and not np.array_equal(a, b)):
            return False
    return x.status == y.status and x.total_found == y.total_found


def test_cardinalities_and_the_limit(orc, dev, corpora):
    """1 group (a whole wave reduces into one slot), 64 and 65, 4096 groups with K = 1024; 4 K + 1 still decline with the limit's message"""
    m, ctx, batch = dev
    c = corpora[4]
    S = aggr_sets(m)
    qs, must = [], []
    for col in (C1, C2, C64, C65):
        for name in ("one", "four", "edges"):
            qs.append(Q(m, "one", col, S[name], K=20)), must.append(True)
    qs.append(Q(m, "one", C16, S["smm"], K=4)), must.append(True)
    qs.append(Q(m, "one", C17, S["smm"], K=4)), must.append(False)
    qs.append(Q(m, "one", C4096, S["four"], K=1024)), must.append(True)
    qs.append(Q(m, "and2", C4096, S["one"], K=1024)), must.append(True)
    qs.append(Q(m, "one", C4097, S["four"], K=1024)), must.append(False)
    qs.append(Q(m, "one", C4096, S["one"], K=1023)), must.append(False)
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, "cardinalities", must) == 3
    assert "%d distinct groups" % (4 * 1023) in last_error() and "GROUPBY_FACTOR" in last_error(), last_error()
    # the sums do what the columns were built for: the 32-bit sum wrapped, the widened one passed 2^32; MIN == MAX == key on the group column
    one_group = got[1]  # C1, "four"
    assert int(one_group.aggr[0, 0]) > 1 << 32 and int(one_group.group_count[0]) == N_DOCS
    assert int(got[0].aggr[0, 0]) == int(one_group.aggr[0, 0]) & 0xFFFFFFFF
    self_q = [Q(m, "one", C64, [m.Aggr(m.AGGR_MIN, C64 * 32, 32), m.Aggr(m.AGGR_MAX, C64 * 32, 32, widen=True)], K=100)]
    g = batch.search(c.seg, self_q)[0]
    assert check(orc, c, self_q, [g], "group column") == 0
    assert np.array_equal(g.aggr[:, 0], g.group_key.astype(np.uint64)) and np.array_equal(g.aggr[:, 1], g.group_key.astype(np.uint64))


@pytest.mark.parametrize("n_fields", [4, 17])
def test_every_instance(orc, dev, corpora, n_fields):
    """one keyword, AND, a boolean tree (scan_pk_kernel); a phrase and ANDs under hit rankers (rank_kernel); <= 8 and 9-32 fields;
    1 aggregate, 4 aggregates, SUM + MIN + MAX of one attribute, the bit-fields and the edge columns"""
    m, ctx, batch = dev
    c = corpora[n_fields]
    S = aggr_sets(m)
    qs = []
    for sh in shapes(m):
        for name in S:
            qs.append(Q(m, sh, C64, S[name], K=16, by=GROUPSORT_COUNT, desc=name != "bits"))
        qs.append(Q(m, sh, BITS, S["four"], bits=7, shift=9, K=200, by=GROUPSORT_WEIGHT, index_weight=3))
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, f"instances {n_fields}", [True] * len(qs)) == 0
    assert batch.stats()["packed"] == 1


def test_order_by_an_aggregate(orc, dev, corpora):
    """ascending and descending, more groups than K; UNIT's sum is @count, so sums tie and the head's rowid decides"""
    m, ctx, batch = dev
    c = corpora[4]
    A = m.Aggr
    qs = []
    for sh in ("one", "and2", "prox2"):
        for desc in (True, False):
            qs.append(Q(m, sh, C64, [A(m.AGGR_SUM, UNIT * 32, 32), A(m.AGGR_SUM, BIG * 32, 32, widen=True)], K=16, desc=desc, order=0))
            qs.append(Q(m, sh, C64, [A(m.AGGR_MIN, I64 * 32, 64, kind=m.SORTKEY_INT64), A(m.AGGR_SUM, BIG * 32, 32)], K=16, desc=desc, order=1))
            qs.append(Q(m, sh, BITS, [A(m.AGGR_MAX, AUX * 32, 32)], bits=7, shift=9, K=32, desc=desc, order=0))  # MAX of rowid % 10: 9 nearly everywhere
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, "order by an aggregate", [True] * len(qs)) == 0
    g = got[0]
    assert g.total_found == 64 and len(g.rowid) == 16 and np.array_equal(g.aggr[:, 0], g.group_count.astype(np.uint64))
    assert len(set(g.aggr[:, 0].tolist())) < 16, "the sums were to tie"
    # the same order as by @count (the rule the aggregate's order restates)
    by_count = batch.search(c.seg, [dataclasses.replace(qs[0], group=dataclasses.replace(qs[0].group, sort_by=GROUPSORT_COUNT), aggr_order=-1)])[0]
    assert same(g, by_count)


def test_in_front_of_the_sorter(orc, dev, corpora):
    """an attribute filter, a weight filter and dead rows: the rejected rows are absent from every aggregate"""
    m, ctx, batch = dev
    c = corpora[4]
    S = aggr_sets(m)
    rng = np.random.default_rng(3)
    flt = [m.Filter(AUX * 32, 32, values=[1, 3, 5, 7, 8])]
    wf = [m.Filter(0, 0, min=1600, max=1 << 30)]
    qs = []
    for sh in ("one", "and2", "tree", "prox2", "phrase"):
        qs += [Q(m, sh, C16, S["four"], K=20, filters=flt), Q(m, sh, C64, S["smm"], K=100, by=GROUPSORT_WEIGHT, weight_filters=wf), Q(m, sh, C16, S["one"], K=20, filters=flt, weight_filters=wf)]
    plain = batch.search(c.seg, qs)
    assert check(orc, c, qs, plain, "filters", [True] * len(qs)) == 0
    unfiltered = batch.search(c.seg, [dataclasses.replace(qs[0], filters=None)])[0]
    assert np.array_equal(plain[0].group_key, unfiltered.group_key) and (plain[0].aggr[:, 0] < unfiltered.aggr[:, 0]).all(), "a filtered sum equals the unfiltered one"
    dead = np.zeros((N_DOCS + 31) // 32, np.uint32)
    killed = rng.choice(N_DOCS, N_DOCS // 5, replace=False).astype(np.uint32)
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    c.seg.set_dead_rows(dead)
    c.oi.dead_rows = dead
    try:
        live = batch.search(c.seg, qs)
        assert check(orc, c, qs, live, "dead rows", [True] * len(qs)) == 0
        assert (live[0].aggr[:, 0] < plain[0].aggr[:, 0]).all()
    finally:
        c.seg.set_dead_rows(None)
        c.oi.dead_rows = None


def test_rowid_base(orc, dev):
    """the flush reads the rows again at global rowid - rowid_base: a base near 2^32"""
    m, ctx, batch = dev
    c = Corpus(m, ctx, orc, 4, rowid_base=0xFFFF0000 - N_DOCS, seed=9)
    try:
        S = aggr_sets(m)
        qs = [Q(m, sh, C64, S[name], K=16, by=by, desc=desc) for sh in ("one", "prox2") for name in ("four", "bits") for by, desc in tg.ORDERS[:4]]
        qs.append(Q(m, "and2", C64, S["one"], K=16, order=0))
        assert check(orc, c, qs, batch.search(c.seg, qs), "rowid_base", [True] * len(qs)) == 0
    finally:
        c.close()


def test_race_on_first_sight(orc, dev):
    """item_bytes at its least: many work items race on the first sight of a group and on its accumulators; two runs are identical"""
    m, ctx, batch = dev
    K = 64
    c = Corpus(m, ctx, orc, 4, seed=21)
    try:
        r = np.arange(N_DOCS, dtype=np.uint64)
        c.rows[:, C64] = scr(r * (4 * K) // N_DOCS)          # 256 values in rowid order
        c.rows[:, C65] = scr(r * (4 * K + 1) // N_DOCS)      # 257
        c.seg.set_attrs(c.rows)
        c.oi.attrs = c.rows
        S = aggr_sets(m)
        qs, must = [], []
        for sh in ("one", "none", "and2", "prox2"):
            qs += [Q(m, sh, C64, S["four"], K=K, by=GROUPSORT_COUNT), Q(m, sh, C65, S["one"], K=K), Q(m, sh, C2, S["smm"], K=K)]
            must += [True, False if sh in ("one", "none") else None, True]
        with Settings(ctx, item_bytes=4096):
            a = batch.search(c.seg, qs)
            assert batch.stats()["n_items"] > 2 * len(qs)
            b = batch.search(c.seg, qs)
        check(orc, c, qs, a, "race", must)
        assert all(same(x, y) for x, y in zip(a, b))
    finally:
        c.close()


def test_batch_state_mixed_and_resubmit(orc, dev, corpora):
    m, ctx, batch = dev
    c = corpora[4]
    S = aggr_sets(m)
    root2 = shapes(m)["and2"][0]
    others = [m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10), m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10, sort=m.Sort(C64 * 32, 32)),
              m.Query(shapes(m)["prox2"][0], ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=7), tg.Q(m, "and2", C64, K=16, by=GROUPSORT_COUNT), tg.Q(m, "prox2", C16, K=8)]
    with_aggr = [Q(m, "and2", C64, S["four"], K=16, by=GROUPSORT_COUNT), Q(m, "prox2", C16, S["one"], K=8), Q(m, "one", C17, S["smm"], K=4), Q(m, "one", C2, S["edges"], K=4, order=1)]
    alone = batch.search(c.seg, others)
    assert all(g.aggr is None for g in alone)
    mixed_q = [with_aggr[0], others[0], others[1], with_aggr[1], others[2], with_aggr[2], others[3], with_aggr[3], others[4]]
    mixed = batch.search(c.seg, mixed_q)
    idx = [i for i, q in enumerate(mixed_q) if q.aggrs is not None]
    assert check(orc, c, [mixed_q[i] for i in idx], [mixed[i] for i in idx], "mixed", [True, True, False, True]) == 1
    for a, i in zip(alone, (1, 2, 4, 6, 8)):  # word for word as when submitted without them
        assert same(a, mixed[i]) and mixed[i].aggr is None, i
    # the same batch again with other aggregates on the same groups: the accumulators were cleared
    again = [Q(m, "and2", C64, S["smm"], K=16, by=GROUPSORT_COUNT), Q(m, "prox2", C16, S["four"], K=8), Q(m, "one", C2, S["wide"], K=4)]
    assert check(orc, c, again, batch.search(c.seg, again), "resubmit", [True] * 3) == 0
    assert check(orc, c, again[::-1], batch.search(c.seg, again[::-1]), "resubmit reversed", [True] * 3) == 0


def test_rerun_after_a_match_queue_overflow(orc, dev):
    """mq_max_chunks = 1 under 180 K matches of hit-ranked queries: the match queue overflows and mrk_batch_wait reruns each query
    alone over a CLEARED table -- sums are those of one run, not of one and a half"""
    m, ctx, batch = dev
    n_docs = 200_000
    hi = m.synth_index(n_docs, [1.0, 0.9, 0.8], seed=31, skiplist_block_size=128, max_pos=12)
    c = Corpus(m, ctx, orc, 2, hi=hi)
    try:
        S = aggr_sets(m)
        hits = [Q(m, "prox2", C16, S["four"], K=8, by=GROUPSORT_COUNT), Q(m, "phrase", C64, S["one"], K=100, order=0), Q(m, "sph04_3", C2, S["smm"], K=2), Q(m, "prox2", C17, S["one"], K=4)]
        with Settings(ctx, mq_max_chunks=1):
            got = batch.search(c.seg, hits)
            n_rerun = batch.stats()["n_rerun"]
        assert n_rerun > 0
        assert check(orc, c, hits, got, "rerun", [True, True, True, False]) == 1
        again = batch.search(c.seg, hits)
        assert batch.stats()["n_rerun"] == 0 and all(same(x, y) for x, y in zip(got, again))
    finally:
        c.close()


def test_declines(orc, dev, corpora):
    m, ctx, batch = dev
    from manticoresearch_amd import _lib
    from manticoresearch_amd._lib import MrkError

    c = corpora[4]
    root, ranker = shapes(m)["and2"]
    A, G, I6 = m.Aggr, m.Group(C16 * 32, 32), m.SORTKEY_INT64
    ok = A(m.AGGR_SUM, BIG * 32, 32)
    base = lambda **kwa: m.Query(root, ranker=ranker, max_matches=10, **kwa)
    unsupported = [(base(group=G, aggrs=[A(m.AGGR_SUM, BIG * 32, 32, kind=m.SORTKEY_FLOAT)]), "SUM of a float"), (base(group=G, aggrs=[ok, A(m.AGGR_MAX, -1, 0)]), "MAX of a blob-stored"),
                   (base(group=G, aggrs=[A(m.AGGR_SUM, I64 * 32, 64, kind=I6)], aggr_order=0), "64-bit result"), (base(group=G, aggrs=[A(m.AGGR_MIN, BIG * 32, 32, widen=True)], aggr_order=0), "64-bit result"),
                   (base(group=G, aggrs=[ok], sort=m.Sort(C64 * 32, 32)), "next to mrk_query.sort"), (base(group=G, aggrs=[ok], cutoff=5), "cutoff"), (base(group=m.Group(-1, 0), aggrs=[ok]), "group by a blob-stored")]
    for q, msg in unsupported:  # one at a time: the message of a decline names what was declined
        g = batch.search(c.seg, [q, base(group=G, aggrs=[ok])])
        assert [x.status for x in g] == [E_UNSUPPORTED, 0] and g[0].aggr is None and g[0].group_key is None and len(g[0].rowid) == 0 and g[1].aggr is not None, msg
    for q, msg in unsupported:
        batch.submit(c.seg, [q])
        assert msg in last_error(), (msg, last_error())
        batch.wait()
    bad = [base(aggrs=[ok]), base(group=G, aggrs=[]), base(group=G, aggrs=[ok] * 5), base(group=G, aggrs=[A(0, BIG * 32, 32)]), base(group=G, aggrs=[A(4, BIG * 32, 32)]),
           base(group=G, aggrs=[A(m.AGGR_SUM, BIG * 32, 32, kind=3)]), base(group=G, aggrs=[A(m.AGGR_SUM, BIG * 32, 32, widen=2)]), base(group=G, aggrs=[A(m.AGGR_SUM, I64 * 32, 64, kind=I6, widen=True)]),
           base(group=G, aggrs=[A(m.AGGR_SUM, STRIDE * 32, 32)]), base(group=G, aggrs=[A(m.AGGR_SUM, BIG * 32 + 30, 7)]), base(group=G, aggrs=[A(m.AGGR_SUM, BIG * 32, 0)]), base(group=G, aggrs=[A(m.AGGR_SUM, BIG * 32, 33)]),
           base(group=G, aggrs=[A(m.AGGR_SUM, I64 * 32 + 8, 64, kind=I6)]), base(group=G, aggrs=[A(m.AGGR_SUM, (STRIDE - 1) * 32, 64, kind=I6)]), base(group=G, aggrs=[ok], aggr_order=1), base(group=G, aggrs=[ok], aggr_order=-2),
           base(group=m.Group(C16 * 32, 32, sort_by=GROUPSORT_COUNT), aggrs=[ok], aggr_order=0)]
    for q in bad:
        with pytest.raises(MrkError):
            batch.search(c.seg, [base(), q])
    # mrk_batch_submit_aggr with aggrs == NULL is mrk_batch_submit_grouped
    qs = [tg.Q(m, "and2", C64, K=16, by=GROUPSORT_COUNT), base(), tg.Q(m, "one", C17, K=4)]
    want = batch.search(c.seg, qs)
    cq = m.api._CQueries(qs)
    _lib.check(_lib.lib().mrk_batch_submit_aggr(batch._h, c.seg._h, cq.arr, cq.groups, None, len(qs)))
    batch._cq, batch._n = cq, len(qs)
    batch.wait()
    assert all(same(x, y) for x, y in zip(want, batch.results()))
    # a segment without attribute rows
    bare = m.Segment(ctx, c.hi)
    try:
        assert batch.search(bare, [base(group=G, aggrs=[ok])])[0].status == E_UNSUPPORTED
    finally:
        bare.close()


@pytest.mark.parametrize("kind", ["rows", "srows", "orows", "grows"])
def test_exchange_rows_decline_a_query_with_aggregates(dev, corpora, kind):
    m, ctx, batch = dev
    from test_gpu_order_merge import Hip
    from manticoresearch_amd import _lib

    hip = Hip()
    c = corpora[4]
    words = {"rows": m.ROW_WORDS, "srows": m.SROW_WORDS, "orows": m.OROW_WORDS, "grows": m.GROW_WORDS}[kind]
    at = m.GROW_GROUPS if kind == "grows" else 1024  # the count word; the total word follows it

    def export(n):
        buf = hip.malloc(n * words * 8)
        hip.fill(buf, 0xEE, n * words * 8)
        _lib.check(getattr(_lib.lib(), f"mrk_batch_export_{kind}")(batch._h, buf))
        return hip.to_host(buf, (n, words))

    S = aggr_sets(m)
    alone_q = [m.Query(shapes(m)["and2"][0], ranker=m.SPH_RANK_BM25, max_matches=10), tg.Q(m, "and2", C16, K=10)]  # a relevance query and a group without aggregates
    batch.search(c.seg, alone_q)
    want = export(2)
    qs = [alone_q[0], Q(m, "and2", C16, S["four"], K=10), alone_q[1], Q(m, "one", C17, S["one"], K=4)]  # an answered query with aggregates and a run-time decline
    got = batch.search(c.seg, qs)
    assert [g.status for g in got] == [0, 0, 0, E_UNSUPPORTED] and got[1].aggr is not None
    rows = export(4)
    for i in (1, 3):  # MRK_ROW_DECLINED, no entries, spec word 0
        assert int(rows[i, at + 1]) == 1 << 62 and int(rows[i, at]) == 0 and not rows[i, :at].any() and not rows[i, at + 2:].any(), (kind, i)
    assert np.array_equal(rows[0], want[0]) and np.array_equal(rows[2], want[1]), (kind, "the batch's other rows")
    if kind == "grows":
        assert int(rows[2, at]) == 16 and int(rows[2, -1]) != 0, "the group without aggregates exports its groups under its spec word"


def test_seeded_fuzz(orc, dev, corpora):
    m, ctx, batch = dev
    rng = np.random.default_rng(20261021)
    names = list(shapes(m))
    cols = [(C1, 32, 0, 1), (C2, 32, 0, 2), (C16, 32, 0, 16), (C17, 32, 0, 17), (C64, 32, 0, 64), (C65, 32, 0, 65), (BITS, 7, 9, 128), (BITS, 1, 5, 2), (C4096, 32, 0, 4096)]
    srcs = [(BIG, 32, 0), (ONES, 32, 0), (ZERO, 32, 0), (UNIT, 32, 0), (AUX, 32, 0), (BITS, 7, 9), (BITS, 1, 5), (C64, 32, 0), (I64, 64, 0)]
    for n_fields in (4, 17):
        c = corpora[n_fields]
        qs, must = [], []
        for i in range(50):
            col, bits, shift, card = cols[int(rng.integers(0, len(cols)))]
            over = i % 10 == 9  # the designated over-limit cases: K below card / 4 on the keyword every doc holds
            if over:
                col, bits, shift, card = [(C17, 32, 0, 17), (C65, 32, 0, 65), (C4097, 32, 0, 4097)][int(rng.integers(0, 3))]
                K, sh = (card - 1) // 4, "one"
            else:
                K, sh = int(rng.choice([k for k in (1, 2, 5, 16, 17, 100, 1000, 1024) if 4 * k >= card])), names[int(rng.integers(0, len(names)))]
            aggrs = []
            for _ in range(int(rng.integers(1, 5))):
                scol, sbits, sshift = srcs[int(rng.integers(0, len(srcs)))]
                func = int(rng.integers(1, 4))
                aggrs.append(m.Aggr(func, scol * 32 + sshift, sbits, kind=m.SORTKEY_INT64) if sbits == 64 else m.Aggr(func, scol * 32 + sshift, sbits, widen=bool(rng.integers(0, 2))))
            narrow = [j for j, a in enumerate(aggrs) if a.kind == m.SORTKEY_INT and not a.widen]
            order = narrow[int(rng.integers(0, len(narrow)))] if narrow and rng.random() < 0.4 else -1
            by, desc = tg.ORDERS[int(rng.integers(0, 6))]
            q = Q(m, sh, col, aggrs, bits=bits, shift=shift, K=K, by=GROUPSORT_KEY if order >= 0 else by, desc=desc, order=order, index_weight=int(rng.choice([1, 1, 3])))
            if rng.random() < 0.25 and not over:
                q.filters = [m.Filter(AUX * 32, 32, values=[0, 2, 4, 9])]
            qs.append(q), must.append(not over)
        got = batch.search(c.seg, qs)
        assert check(orc, c, qs, got, f"fuzz {n_fields}", must) == 5
