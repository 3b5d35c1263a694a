"""GPU: GROUP BY an integer attribute (Query.group; mrk_batch_submit_grouped) against group_expect -- the numpy model of the
reference's grouping sorter over the oracle's full match set, itself pinned on the reference's recorded results
(tests/test_group_cpu.py).  Every comparison is bit for bit: head rowid, head weight, group key, @count, total_found, order.
A query whose model answer is DECLINED (more than 4 * max_matches distinct keys) must come back MRK_E_UNSUPPORTED with the limit in
the message; any other decline is a failure.

Columns of a row (dwords): a constant; {0, 0xFFFFFFFF}; 64 / 65 / 16 / 17 / 4096 / 4097 scrambled values (rowid % C through an odd
multiplier); a dword of all ones but a 1-bit field at bit 5 and a 7-bit field at bit 9; rowid % 10 (filters); four columns of the
seeded generator (group_expect.seeded_value) whose seeds tests/cpp/group_table.cpp found to collide / wrap in the 16- and 32-slot
tables of K = 1 and K = 2 (test_group_cpu.py checks that the seeds named here are the ones it prints)."""
import dataclasses

import numpy as np
import pytest

from group_expect import DECLINED, GROUPSORT_COUNT, GROUPSORT_KEY, GROUPSORT_WEIGHT, expected_group, seeded_value
from helpers import synth_postings
from test_gpu_parity import kw, orc_index_of, to_orc

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -2
N_DOCS = 9000
PROBS = [1.0, 0.6, 0.4, 0.3, 0.2]
C1, C2, C64, C65, C16, C17, C4096, C4097, BITS, AUX, S1C, S1W, S2C, S2W = range(14)
STRIDE = 14
# seeds of group_expect.seeded_value: (K, seed, what) -- as tests/cpp/group_table.cpp prints them
SEEDS = {S1C: (1, 0, "collide"), S1W: (1, 8, "wrap"), S2C: (2, 3, "collide"), S2W: (2, 8, "wrap")}
ORDERS = [(by, desc) for by in (GROUPSORT_KEY, GROUPSORT_COUNT, GROUPSORT_WEIGHT) for desc in (True, False)]


def scr(j):
    return ((j.astype(np.uint64) * 0x9E3779B1 + 12345) & 0xFFFFFFFF).astype(np.uint32)


def make_rows(n_docs):
    r = np.arange(n_docs, dtype=np.uint64)
    rows = np.zeros((n_docs, STRIDE), np.uint32)
    rows[:, C1] = 7
    rows[:, C2] = np.where((r * 7 // 3) % 2 == 0, 0, 0xFFFFFFFF).astype(np.uint32)
    for col, c in ((C64, 64), (C65, 65), (C16, 16), (C17, 17), (C4096, 4096), (C4097, 4097)):
        rows[:, col] = scr(r % c)
    one = ((r * 5 // 3) & 1).astype(np.uint32)
    seven = ((r * 37) % 128).astype(np.uint32)
    rows[:, BITS] = (np.uint32(0xFFFFFFFF) & ~np.uint32((1 << 5) | (127 << 9))) | (one << np.uint32(5)) | (seven << np.uint32(9))
    rows[:, AUX] = (r % 10).astype(np.uint32)
    for col, (k, seed, _) in SEEDS.items():
        rows[:, col] = np.array([seeded_value(seed, int(j)) for j in range(4 * k)], np.uint32)[(r % (4 * k)).astype(np.int64)]
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
        self.cache = {}

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


def shapes(m):
    X = m.XQNode
    return {"one": (kw(m, 0, 1), m.SPH_RANK_BM25), "none": (kw(m, 0, 1), m.SPH_RANK_NONE), "and2": (X.AND(kw(m, 0, 1), kw(m, 1, 2)), m.SPH_RANK_BM25),
            "tree": (X.AND(X(m.SPH_QUERY_OR, [kw(m, 1, 1), kw(m, 2, 2)]), X(m.SPH_QUERY_ANDNOT, [kw(m, 0, 3), kw(m, 3, 4)])), m.SPH_RANK_BM25),
            "phrase": (X(m.SPH_QUERY_PHRASE, [kw(m, 1, 1), kw(m, 2, 2)]), m.SPH_RANK_PROXIMITY_BM25),
            "prox2": (X.AND(kw(m, 1, 1), kw(m, 2, 2)), m.SPH_RANK_PROXIMITY_BM25),
            "sph04_3": (X.AND(kw(m, 0, 1), kw(m, 1, 2), kw(m, 2, 3)), m.SPH_RANK_SPH04)}


def Q(m, shape, col, bits=32, shift=0, K=20, by=GROUPSORT_KEY, desc=True, **kwa):
    root, ranker = shapes(m)[shape]
    return m.Query(root, ranker=ranker, max_matches=K, group=m.Group(col * 32 + shift, bits, sort_by=by, desc=desc), **kwa)


def check(orc, c, queries, got, what="", must=None):
    """must: per query True = the model must answer, False = must decline, None = whatever the model says"""
    n_decl = 0
    for i, (q, g) in enumerate(zip(queries, got)):
        if q.group is None:
            want = to_orc(orc, q).run(c.oi)
            assert g.status == 0 and g.group_key is None and g.group_count is None, (what, i)
            assert g.total_found == want.total_found and np.array_equal(g.rowid, want.rowid) and np.array_equal(g.weight, want.weight), (what, i)
            continue
        want = expected_group(orc, c.oi, q, c.rows, c.n_docs)
        if must is not None and must[i] is not None:
            assert (want is not DECLINED) == must[i], (what, i, "the case is not what the test designates")
        if want is DECLINED:
            n_decl += 1
            assert g.status == E_UNSUPPORTED and len(g.rowid) == 0 and g.total_found == 0 and g.group_key is None, (what, i, g.status)
            continue
        assert g.status == 0, (what, i, q.group, q.max_matches, "a device decline where the model answers")
        r, w, k, cnt, total = want
        assert g.total_found == total, (what, i, g.total_found, total)
        assert np.array_equal(g.rowid, r), (what, i, q.group, q.max_matches, g.rowid[:8], r[:8])
        assert np.array_equal(g.weight, w), (what, i, g.weight[:8], w[:8])
        assert np.array_equal(g.group_key, k), (what, i, g.group_key[:8], k[:8])
        assert np.array_equal(g.group_count, cnt), (what, i, g.group_count[:8], cnt[:8])
        assert g.sort_key is None and g.order_key is None
    return n_decl


class Settings:
    """ctx.set() for the block, the defaults (mrk_host_int.h) back afterwards whatever happens"""
    DEFAULTS = {"item_bytes": 128 << 10, "mq_max_chunks": 1 << 22}

    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set(k, self.DEFAULTS[k])


def last_error():
    from manticoresearch_amd import _lib

    return _lib.lib().mrk_last_error().decode()


def test_cardinalities_and_the_limit(orc, dev, corpora):
    m, ctx, batch = dev
    c = corpora[4]
    qs, must = [], []
    for col in (C1, C2, C64, C65):  # 1: a whole wave on one key; 64 / 65: a wave's worth of distinct keys and one more
        for sh in ("one", "none"):
            qs.append(Q(m, sh, col, K=20)), must.append(True)
    for sh in ("one", "and2"):
        qs.append(Q(m, sh, C16, K=4)), must.append(True)     # 16 = 4 K: the limit, answered
        qs.append(Q(m, sh, C17, K=4)), must.append(False)    # 17: declined
    qs.append(Q(m, "one", C4096, K=1024)), must.append(True)
    qs.append(Q(m, "one", C4097, K=1024)), must.append(False)
    qs.append(Q(m, "one", C4096, K=1023)), must.append(False)
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, "cardinalities", must) == 4
    for q, g in zip(qs, got):  # the run-time decline names the limit (the last one's message stands)
        if g.status != 0:
            assert g.status == E_UNSUPPORTED
    assert "%d distinct groups" % (4 * 1023) in last_error() and "GROUPBY_FACTOR" in last_error(), last_error()


def test_key_values_bit_fields_and_probe_seeds(orc, dev, corpora):
    m, ctx, batch = dev
    c = corpora[4]
    qs = [Q(m, "one", C2, K=5), Q(m, "and2", C2, K=1, by=GROUPSORT_COUNT),
          Q(m, "one", BITS, bits=1, shift=5, K=3), Q(m, "one", BITS, bits=7, shift=9, K=32), Q(m, "and2", BITS, bits=7, shift=9, K=200, by=GROUPSORT_COUNT, desc=False)]
    for col, (k, seed, _) in SEEDS.items():
        for sh in ("one", "and2", "prox2"):
            qs.append(Q(m, sh, col, K=k, by=GROUPSORT_COUNT))
            qs.append(Q(m, sh, col, K=k, by=GROUPSORT_KEY, desc=False))
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, "key values", [True] * len(qs)) == 0
    assert set(got[0].group_key.tolist()) == {0, 0xFFFFFFFF}


@pytest.mark.parametrize("n_fields", [4, 17])
def test_every_instance_all_orders_heads(orc, dev, corpora, n_fields):
    """one keyword, AND, a boolean tree, a phrase and an AND under hit rankers (rank_kernel), on <= 8 and on 9-32 fields; all six
    orders with groups > K (64 groups, K = 16, the limit: ties in count and in head weight fall to the head's rowid); NONE: head = lowest rowid"""
    m, ctx, batch = dev
    c = corpora[n_fields]
    qs = []
    for sh in shapes(m):
        for by, desc in ORDERS:
            qs.append(Q(m, sh, C64, K=16, by=by, desc=desc))
        qs.append(Q(m, sh, C2, K=1000, by=GROUPSORT_WEIGHT, index_weight=3))
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, f"instances {n_fields}", [True] * len(qs)) == 0
    assert batch.stats()["packed"] == 1
    none = [g for q, g in zip(qs, got) if q.ranker == m.SPH_RANK_NONE][0]
    assert (none.weight == 1).all() and none.total_found == 64


def test_rowid_base(orc, dev):
    m, ctx, batch = dev
    c = Corpus(m, ctx, orc, 4, rowid_base=0xFFFF0000 - N_DOCS, seed=9)
    try:
        qs = [Q(m, sh, C64, K=16, by=by, desc=desc) for sh in ("one", "prox2") for by, desc in ORDERS]
        assert check(orc, c, qs, batch.search(c.seg, qs), "rowid_base", [True] * len(qs)) == 0
    finally:
        c.close()


def test_in_front_of_the_sorter(orc, dev, corpora):
    """dead rows, an attribute filter and a weight filter next to a group: rejected matches are absent from the counts"""
    m, ctx, batch = dev
    c = corpora[4]
    rng = np.random.default_rng(3)
    flt = [m.Filter(AUX * 32, 32, values=[1, 3, 5, 7, 8])]
    wf = [m.Filter(0, 0, min=1600, max=1 << 30)]
    qs = []
    for sh in ("one", "and2", "tree", "prox2", "phrase"):
        qs += [Q(m, sh, C16, K=20, by=GROUPSORT_COUNT, filters=flt), Q(m, sh, C64, K=100, by=GROUPSORT_WEIGHT, weight_filters=wf),
               Q(m, sh, C16, K=20, filters=flt, weight_filters=wf)]
    plain = batch.search(c.seg, qs)
    assert check(orc, c, qs, plain, "filters", [True] * len(qs)) == 0
    unfiltered = batch.search(c.seg, [dataclasses.replace(qs[0], filters=None)])[0]
    assert int(plain[0].group_count.sum()) < int(unfiltered.group_count.sum())
    dead = np.zeros((N_DOCS + 31) // 32, np.uint32)
    killed = rng.choice(N_DOCS, N_DOCS // 5, replace=False).astype(np.uint32)
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    c.seg.set_dead_rows(dead)
    c.oi.dead_rows = dead
    try:
        assert check(orc, c, qs, batch.search(c.seg, qs), "dead rows", [True] * len(qs)) == 0
    finally:
        c.seg.set_dead_rows(None)
        c.oi.dead_rows = None


def test_mva_filter_next_to_a_group(orc, dev):
    """an MVA filter (any / all over the blob pool) in front of the sorter: the rows it rejects are absent from the counts"""
    m, ctx, batch = dev
    from helpers import build_blob_pool

    c = Corpus(m, ctx, orc, 4, seed=33)
    try:
        vals = [[np.array(sorted({r % 5, (r * 3) % 7, 9 if r % 4 == 0 else r % 5}), "<u4").tobytes()] for r in range(N_DOCS)]
        pool, offs = build_blob_pool(vals)
        c.rows[:, 2] = np.array(offs, np.uint64).astype(np.uint32)  # the blob row offset is the row's second attribute (dwords 2, 3)
        c.rows[:, 3] = 0
        c.seg.set_attrs(c.rows)
        c.seg.set_blobs(pool, 1, c.rows)
        c.oi.attrs, c.oi.blobs = c.rows, pool
        F = m.Filter
        qs = []
        for sh in ("one", "and2", "prox2"):
            qs += [Q(m, sh, C16, K=16, by=GROUPSORT_COUNT, filters=[F(0, 0, values=[1, 3], mva_bits=32, blob_attr_id=0, n_blob_attrs=1)]),
                   Q(m, sh, C16, K=16, filters=[F(0, 0, values=[0, 1, 2, 9], mva_bits=32, mva_all=True, blob_attr_id=0, n_blob_attrs=1)])]
        got = batch.search(c.seg, qs)
        assert check(orc, c, qs, got, "mva", [True] * len(qs)) == 0
        everything = batch.search(c.seg, [dataclasses.replace(qs[0], filters=None)])[0]
        assert 0 < int(got[0].group_count.sum()) < int(everything.group_count.sum())
    finally:
        c.close()


def test_race_on_first_sight(orc, dev):
    """item_bytes at its least: one query runs as many work items; a sorted column: the first blocks of every item hold only values no
    other item has seen.  Exactly 4 K distinct values answer, 4 K + 1 decline; two runs on one batch are identical."""
    m, ctx, batch = dev
    K = 64
    c = Corpus(m, ctx, orc, 4, seed=21)
    try:
        r = np.arange(N_DOCS, dtype=np.uint64)
        c.rows[:, C64] = scr(r * (4 * K) // N_DOCS)          # 256 values in rowid order
        c.rows[:, C65] = scr(r * (4 * K + 1) // N_DOCS)      # 257
        c.seg.set_attrs(c.rows)
        c.oi.attrs = c.rows
        qs, must = [], []
        for sh in ("one", "none", "and2", "prox2"):
            qs += [Q(m, sh, C64, K=K, by=GROUPSORT_COUNT), Q(m, sh, C65, K=K)]
            must += [True, False if sh in ("one", "none") else None]  # (keyword 0 is in every doc: all 257 values match)
        with Settings(ctx, item_bytes=4096):
            a = batch.search(c.seg, qs)
            assert batch.stats()["n_items"] > 2 * len(qs)
            b = batch.search(c.seg, qs)
        check(orc, c, qs, a, "race", must)
        for x, y in zip(a, b):
            assert x.status == y.status and x.total_found == y.total_found and np.array_equal(x.rowid, y.rowid) and np.array_equal(x.weight, y.weight)
            assert (x.group_key is None) == (y.group_key is None)
            if x.group_key is not None:
                assert np.array_equal(x.group_key, y.group_key) and np.array_equal(x.group_count, y.group_count)
    finally:
        c.close()


def test_batch_state_mixed_resubmit_and_rerun(orc, dev, corpora):
    m, ctx, batch = dev
    c = corpora[4]
    root2 = shapes(m)["and2"][0]
    others = [m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10), m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10, sort=m.Sort(C64 * 32, 32)),
              m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10, order=m.Order([m.OrderPart(C16 * 32, 32), m.OrderPart(AUX * 32, 32, desc=False)])),
              m.Query(shapes(m)["prox2"][0], ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=7)]
    grouped = [Q(m, "and2", C64, K=16, by=GROUPSORT_COUNT), Q(m, "prox2", C16, K=8), Q(m, "one", C17, K=4)]
    alone = batch.search(c.seg, others)
    mixed_q = [grouped[0], others[0], others[1], grouped[1], others[2], grouped[2], others[3]]
    mixed = batch.search(c.seg, mixed_q)
    check(orc, c, [q for q in mixed_q if q.group is not None], [g for q, g in zip(mixed_q, mixed) if q.group is not None], "mixed", [True, True, False])
    for a, g in zip(alone, [mixed[1], mixed[2], mixed[4], mixed[6]]):  # word for word as without the grouped ones
        assert a.status == g.status == 0 and a.total_found == g.total_found and np.array_equal(a.rowid, g.rowid) and np.array_equal(a.weight, g.weight)
        for f in ("sort_key", "order_key", "group_key"):
            assert (getattr(a, f) is None) == (getattr(g, f) is None) and (getattr(a, f) is None or np.array_equal(getattr(a, f), getattr(g, f)))
    # a second submit on the same batch with other groups: the tables were cleared
    again = [Q(m, "and2", C16, K=10, by=GROUPSORT_COUNT), Q(m, "prox2", C64, K=80), Q(m, "one", C2, K=4)]
    assert check(orc, c, again, batch.search(c.seg, again), "resubmit", [True] * 3) == 0


def test_rerun_after_a_match_queue_overflow(orc, dev):
    """mq_max_chunks = 1 (64 chunks per shard) under 180 K matches of hit-ranked grouped queries: the match queue overflows,
    mrk_batch_wait reruns each query alone over a CLEARED table -- the first run's partial counts are not added to"""
    m, ctx, batch = dev
    n_docs = 200_000
    hi = m.synth_index(n_docs, [1.0, 0.9, 0.8], seed=31, skiplist_block_size=128, max_pos=12)
    c = Corpus(m, ctx, orc, 2, hi=hi)
    try:
        hits = [Q(m, "prox2", C16, K=8, by=GROUPSORT_COUNT), Q(m, "phrase", C64, K=100), Q(m, "sph04_3", C2, K=2), Q(m, "prox2", C17, K=4)]
        with Settings(ctx, mq_max_chunks=1):
            got = batch.search(c.seg, hits)
            n_rerun = batch.stats()["n_rerun"]
        assert n_rerun > 0
        assert check(orc, c, hits, got, "rerun", [True, True, True, False]) == 1
        assert check(orc, c, hits, batch.search(c.seg, hits), "no rerun", [True, True, True, False]) == 1 and batch.stats()["n_rerun"] == 0
    finally:
        c.close()


def test_plan_time_declines(orc, dev, corpora):
    m, ctx, batch = dev
    from manticoresearch_amd._lib import MrkError

    c = corpora[4]
    root, ranker = shapes(m)["and2"]
    G = m.Group
    base = lambda **kwa: m.Query(root, ranker=ranker, max_matches=10, **kwa)
    unsupported = [base(group=G(C16 * 32, 32), sort=m.Sort(C64 * 32, 32)), base(group=G(C16 * 32, 32), order=m.Order([m.OrderPart(C64 * 32, 32), m.OrderPart(AUX * 32, 32)])),
                   base(group=G(C16 * 32, 32), cutoff=5), base(group=G(-1, 0)), base(group=G(C16 * 32, 64))]
    got = batch.search(c.seg, unsupported + [base(group=G(C16 * 32, 32))])
    assert [g.status for g in got] == [E_UNSUPPORTED] * len(unsupported) + [0]
    assert all(g.group_key is None and len(g.rowid) == 0 for g in got[:-1])
    for bad in (G(STRIDE * 32, 32), G(C16 * 32 + 30, 7), G(C16 * 32, 0), G(C16 * 32, 33), G(C16 * 32 + 32, 64 + 1), G(C16 * 32, 32, sort_by=3), G(C16 * 32, 32, sort_by=-1), G(C16 * 32, 32, desc=2)):
        with pytest.raises(MrkError):
            batch.search(c.seg, [base(), base(group=bad)])
    # a segment without attribute rows; the VLB-direct path
    bare = m.Segment(ctx, c.hi)
    try:
        assert batch.search(bare, [base(group=G(C16 * 32, 32))])[0].status == E_UNSUPPORTED
    finally:
        bare.close()
    ctx.set("path", 1)
    try:
        assert batch.search(c.seg, [base(group=G(C16 * 32, 32))])[0].status == E_UNSUPPORTED
    finally:
        ctx.set("path", 0)


@pytest.mark.parametrize("kind", ["rows", "srows", "orows"])
def test_exchange_rows_decline_a_grouped_query(dev, corpora, kind):
    m, ctx, batch = dev
    from test_gpu_order_merge import Hip
    from test_gpu_row_kinds import export, words

    hip = Hip()
    c = corpora[4]
    root2 = shapes(m)["and2"][0]
    rel = [m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10), m.Query(shapes(m)["one"][0], ranker=m.SPH_RANK_BM25, max_matches=30)]
    batch.search(c.seg, rel)
    want = export(m, hip, batch, kind, 2)
    qs = [rel[0], Q(m, "and2", C16, K=10), rel[1], Q(m, "one", C17, K=4)]  # an answered group and a run-time decline
    got = batch.search(c.seg, qs)
    assert [g.status for g in got] == [0, 0, 0, E_UNSUPPORTED]
    rows = export(m, hip, batch, kind, 4)
    K1 = 1024
    for i in (1, 3):
        assert int(rows[i, K1 + 1]) == 1 << 62 and int(rows[i, K1]) == 0 and not rows[i, :K1].any() and not rows[i, K1 + 2:].any(), (kind, i)
    assert np.array_equal(rows[0], want[0]) and np.array_equal(rows[2], want[1]), (kind, "the batch's other rows")
    assert rows.shape[1] == words(m, kind)


def test_seeded_fuzz(orc, dev, corpora):
    m, ctx, batch = dev
    rng = np.random.default_rng(20261020)
    names = list(shapes(m))
    cols = [(C1, 32, 0, 1), (C2, 32, 0, 2), (C16, 32, 0, 16), (C17, 32, 0, 17), (C64, 32, 0, 64), (C65, 32, 0, 65), (BITS, 7, 9, 128), (BITS, 1, 5, 2), (C4096, 32, 0, 4096)]
    for n_fields in (4, 17):
        c = corpora[n_fields]
        qs, must = [], []
        for i in range(60):
            col, bits, shift, card = cols[int(rng.integers(0, len(cols)))]
            over = i % 10 == 9  # the designated over-limit cases: K below card / 4 on the keyword every doc holds
            if over:
                col, bits, shift, card = [(C17, 32, 0, 17), (C65, 32, 0, 65), (C4097, 32, 0, 4097)][int(rng.integers(0, 3))]
                K, sh = (card - 1) // 4, "one"
            else:
                K, sh = int(rng.choice([k for k in (1, 2, 5, 16, 17, 100, 1000, 1024) if 4 * k >= card])), names[int(rng.integers(0, len(names)))]
            by, desc = ORDERS[int(rng.integers(0, 6))]
            q = Q(m, sh, col, bits=bits, shift=shift, K=K, by=by, desc=desc, index_weight=int(rng.choice([1, 1, 3])))
            if rng.random() < 0.25 and not over:
                q.filters = [m.Filter(AUX * 32, 32, values=[0, 2, 4, 9])]
            qs.append(q), must.append(not over)
        got = batch.search(c.seg, qs)
        assert check(orc, c, qs, got, f"fuzz {n_fields}", must) == 6
