"""GPU: sorted queries (Query.sort) answered across segments and shards through the WIDE exchange rows (MRK_SROW_WORDS): the
shards' exported rows merged by mrk_topk_merge_srows must equal the unsharded device result bit for bit, ties at rank K
included; the kernel must equal its numpy mirror (dist.merge_srows_np) word for word; a relevance-only batch must come out as
the narrow merge gives it; and whatever cannot be answered must be loud.  Every comparison is exact."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import sort_merge_common as smc
from test_gpu_parity import kw, orc_index_of, to_orc
from test_gpu_sort import BITS, FLT, check, expected, make_rows, random_queries, sorts

pytestmark = pytest.mark.gpu

K1 = 1024
N_DOCS, CUTS = 700_001, [0, 131_072, 400_003, 700_001]
PROBS = [0.35, 0.2, 0.1, 0.05, 0.04, 0.02, 0.01, 0.006]


class Hip:
    """Device buffers of the test.  Every fill and copy is finished before it returns: hipMemset and a device-to-device hipMemcpy on
    the null stream may return before the device has done them, and the library's merge stream is non-blocking -- nothing else would
    order a 0xEE fill, or the copies that stand in for the all-to-all, before the merge kernel that reads and writes the same rows."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.bufs = []

    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0

    def malloc(self, n):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(n, 8))) == 0
        self.bufs.append(p)
        return p

    def to_host(self, p, shape):
        a = np.zeros(shape, np.uint64)
        assert self.hip.hipMemcpy(C.c_void_p(a.ctypes.data), p, C.c_size_t(a.nbytes), 2) == 0
        return a

    def to_dev(self, p, a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        assert self.hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        self.sync()

    def d2d(self, dst, src, n):
        assert self.hip.hipMemcpy(dst, src, C.c_size_t(n), 3) == 0
        self.sync()

    def fill(self, p, byte, n):
        assert self.hip.hipMemset(p, byte, C.c_size_t(n)) == 0
        self.sync()

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(p)
        self.bufs = []


def off(p, nbytes):
    return C.c_void_p(p.value + nbytes)


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
def corpus():
    import manticoresearch_amd as m

    c = smc.Corpus(m, make_rows, N_DOCS, CUTS, PROBS, seed=2026, rows_seed=41)
    assert all(CUTS[i + 1] - CUTS[i] < 2 ** 20 for i in range(3))  # no candidate list can overflow
    return c


def L():
    from manticoresearch_amd import _lib

    return _lib.lib(), _lib.check


def unsharded(m, ctx, batch, corpus, qs):
    seg = m.Segment(ctx, corpus.whole)
    try:
        seg.set_attrs(corpus.rows)
        want = batch.search(seg, qs)
        assert batch.stats()["packed"] == 1
    finally:
        seg.close()
    return want


def shard_srows(m, ctx, batch, hip, corpus, qs, shard_rows=None, allow_declined=False):
    """Every shard's wide rows of the batch, exported behind mrk_batch_wait -> device [3][nq][SROW_WORDS]; the per-shard statuses."""
    lib, chk = L()
    nq, RW = len(qs), m.SROW_WORDS
    srows_all = hip.malloc(3 * nq * RW * 8)
    hip.fill(srows_all, 0xEE, 3 * nq * RW * 8)
    statuses = []
    for s in range(3):
        seg = m.Segment(ctx, corpus.shards[s], rowid_base=corpus.cuts[s])
        try:
            seg.set_attrs((shard_rows or corpus.shard_rows)[s])
            batch.submit(seg, qs)
            batch.wait()
            assert batch.stats()["n_rerun"] == 0
            st = [r.status for r in batch.results()]
            if not allow_declined:
                assert st == [0] * nq, ("no query may be declined on a shard", s, st)
            statuses.append(st)
            batch.export_srows(srows_all.value + s * nq * RW * 8)
        finally:
            seg.close()
    return srows_all, statuses


def merge(m, ctx, hip, srows_all, n_lists, nq, k=1024):
    lib, chk = L()
    out = hip.malloc(nq * m.SROW_WORDS * 8)
    hip.fill(out, 0xEE, nq * m.SROW_WORDS * 8)
    chk(lib.mrk_topk_merge_srows(ctx._h, srows_all, n_lists, nq, k, out))
    return hip.to_host(out, (nq, m.SROW_WORDS))


def assert_equals_unsharded(mdist, qs, want, host, what):
    for qi, (q, w) in enumerate(zip(qs, want)):
        row = host[qi]
        assert w.status == 0
        assert not int(row[K1 + 1]) & (mdist.ROW_RERUN | mdist.ROW_DECLINED), (what, qi, hex(int(row[K1 + 1])))
        smc.assert_padding(mdist, row)
        docid, weight, sk, total = smc.decode_srow(mdist, row, q.max_matches)
        assert total == w.total_found, (what, qi, total, w.total_found)
        assert np.array_equal(docid, w.rowid), (what, qi, q.sort, q.max_matches, docid[:8], w.rowid[:8])
        assert np.array_equal(weight, w.weight), (what, qi)
        if q.sort is None:
            assert sk is None and w.sort_key is None and int(row[mdist.SROW_SPEC]) == 0
        else:
            assert int(row[mdist.SROW_SPEC]) == mdist.sort_spec_word(q.sort.kind, q.sort.desc, q.sort.then_weight, q.sort.bit_count)
            assert np.array_equal(sk, smc.fold_zero(w.sort_key, q.sort.kind)), (what, qi, q.sort)


def mixed_queries(m, corpus, n, seed):
    """random_queries' shapes with every sort column, both directions and the three tie rules laid over them in turn, relevance
    queries in between."""
    rng = np.random.default_rng(seed)
    S = sorts(m)
    names = list(S)
    qs = []
    for i, q in enumerate(random_queries(m, rng, corpus.nt, n)):
        o, cnt, kind = S[names[i % 5]]
        q = dataclasses.replace(q, sort=m.Sort(o, cnt, desc=bool((i // 5) % 2), then_weight=(i // 10) % 3, kind=kind))
        qs.append(corpus.globalize(q))
        if i % 4 == 3:
            qs.append(corpus.globalize(dataclasses.replace(q, sort=None)))
    return qs


def test_sharded_sorted_equals_unsharded(orc, dev, corpus):
    """Items 4 and 5: three uneven shards of 700 001 docs; the unsharded device result is checked against the oracle on a subset,
    then the merge of the shards' wide rows must equal it for every query; the kernel equals merge_srows_np word for word, and so
    does the partitioned form."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    RW = m.SROW_WORDS
    for rnd in range(2):
        qs = mixed_queries(m, corpus, 90, 4100 + rnd)
        nq = len(qs)
        assert nq <= 256
        assert {(q.sort.bit_offset, q.sort.desc, q.sort.then_weight) for q in qs if q.sort} >= {(o, d, t) for o, _, _ in sorts(m).values() for d in (False, True) for t in (0, 1, 2)}
        want = unsharded(m, ctx, batch, corpus, qs)
        if rnd == 0:  # the unsharded device result against the oracle, on a subset the oracle can afford
            oi = orc_index_of(orc, corpus.whole)
            oi.attrs = corpus.rows
            sub = [i for i, q in enumerate(qs) if q.sort is not None][:4] + [i for i, q in enumerate(qs) if q.sort is None][:2]
            check(orc, oi, corpus.rows, N_DOCS, [qs[i] for i in sub], [want[i] for i in sub], "unsharded")
        srows_all, _ = shard_srows(m, ctx, batch, hip, corpus, qs)
        host = merge(m, ctx, hip, srows_all, 3, nq)
        assert_equals_unsharded(mdist, qs, want, host, f"round {rnd}")
        # the kernel equals its mirror
        host_in = hip.to_host(srows_all, (3, nq, RW))
        assert np.array_equal(mdist.merge_srows_np(host_in, 1024), host)
        assert np.array_equal(mdist.merge_srows_np(host_in, 10), merge(m, ctx, hip, srows_all, 3, nq, k=10))
        # the partitioned form, emulated on one device: device copies stand in for the all-to-all
        part = hip.malloc(nq * RW * 8)
        hip.fill(part, 0xEE, nq * RW * 8)
        per = (nq + 2) // 3
        recv = hip.malloc(3 * per * RW * 8)
        covered = 0
        for r in range(3):
            f, c = C.c_uint32(), C.c_uint32()
            chk(lib.mrk_shard_slice(nq, 3, r, C.byref(f), C.byref(c)))
            assert f.value == covered and c.value <= per
            covered += c.value
            for s in range(3):
                hip.d2d(off(recv, s * per * RW * 8), off(srows_all, (s * nq + f.value) * RW * 8), c.value * RW * 8)
            chk(lib.mrk_topk_merge_srows_part(ctx._h, recv, 3, per, f.value, c.value, 1024, part))
        assert covered == nq
        assert np.array_equal(hip.to_host(part, (nq, RW)), host)
        hip.free()


def test_relevance_batches_merge_as_the_narrow_rows_do(dev, corpus):
    """Item 6: spec 0 parity -- words 0..1025 of the wide merge are the narrow rows mrk_topk_merge_rows gives for the same shards."""
    m, ctx, batch, hip = dev
    lib, chk = L()
    qs = [dataclasses.replace(q, sort=None) for q in mixed_queries(m, corpus, 60, 99)]
    nq, RW, NW = len(qs), m.SROW_WORDS, m.ROW_WORDS
    srows_all, rows_all = hip.malloc(3 * nq * RW * 8), hip.malloc(3 * nq * NW * 8)
    for s in range(3):
        seg = m.Segment(ctx, corpus.shards[s], rowid_base=corpus.cuts[s])
        try:
            seg.set_attrs(corpus.shard_rows[s])
            batch.submit(seg, qs)
            batch.wait()
            assert [r.status for r in batch.results()] == [0] * nq
            batch.export_srows(srows_all.value + s * nq * RW * 8)
            chk(lib.mrk_batch_export_rows(batch._h, off(rows_all, s * nq * NW * 8)))
        finally:
            seg.close()
    for k in (1024, 37):
        wide = merge(m, ctx, hip, srows_all, 3, nq, k=k)
        out = hip.malloc(nq * NW * 8)
        chk(lib.mrk_topk_merge_rows(ctx._h, rows_all, 3, nq, k, out))
        narrow = hip.to_host(out, (nq, NW))
        assert np.array_equal(wide[:, :NW], narrow)
        assert not wide[:, NW:].any()  # no mapped keys, spec 0
        assert narrow[:, K1].max() > 0
    hip.free()


def test_low_cardinality_columns_across_shards(orc, dev, corpus):
    """Item 7: the 4-valued category and the bool column under BM25 with K = 1000: most of the top K shares one key on every shard;
    the order is by weight, then global docid."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    S = sorts(m)
    qs = []
    for name in ("cat", "bool"):
        o, cnt, kind = S[name]
        for root in (kw(m, 0, 1), m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))):
            for d, t in ((True, 1), (False, 2), (True, 0), (False, 1)):
                qs.append(corpus.globalize(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=1000, sort=m.Sort(o, cnt, desc=d, then_weight=t, kind=kind))))
    want = unsharded(m, ctx, batch, corpus, qs)
    for w in want:  # the premise: (nearly) the whole top K sits on one key
        vals, counts = np.unique(w.sort_key, return_counts=True)
        assert len(w.rowid) == 1000 and counts.max() >= 900
    oi = orc_index_of(orc, corpus.whole)
    oi.attrs = corpus.rows
    check(orc, oi, corpus.rows, N_DOCS, qs[:2] + qs[-1:], want[:2] + want[-1:], "low cardinality, unsharded")
    srows_all, _ = shard_srows(m, ctx, batch, hip, corpus, qs)
    host = merge(m, ctx, hip, srows_all, 3, len(qs))
    assert_equals_unsharded(mdist, qs, want, host, "low cardinality")
    hip.free()


def test_loud_cases(dev, corpus):
    """Item 8: (a) a NaN in one shard's float column: that shard declines the float-sorted query, the merged row carries
    MRK_ROW_DECLINED and no keys, the batch's other queries are exact; (b) a narrow standing destination still declines a sorted
    query; (c) narrow and wide standing destinations together are MRK_E_INVAL."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    S = sorts(m)
    root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
    mk = lambda name, **kwa: corpus.globalize(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=100,
                                                      sort=m.Sort(S[name][0], S[name][1], kind=S[name][2], **kwa)))
    qs = [mk("float", desc=True, then_weight=1), mk("ts", desc=False, then_weight=2), corpus.globalize(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=100)),
          mk("float", desc=False, then_weight=0)]
    nq = len(qs)
    want = unsharded(m, ctx, batch, corpus, qs)
    nan_rows = [r.copy() for r in corpus.shard_rows]
    nan_rows[1][17, FLT] = 0x7FC00000
    srows_all, statuses = shard_srows(m, ctx, batch, hip, corpus, qs, shard_rows=nan_rows, allow_declined=True)
    assert statuses == [[0, 0, 0, 0], [-2, 0, 0, -2], [0, 0, 0, 0]]
    host = merge(m, ctx, hip, srows_all, 3, nq)
    for qi in (0, 3):
        assert int(host[qi, K1 + 1]) & mdist.ROW_DECLINED and int(host[qi, K1]) == 0
        assert not host[qi, :K1].any() and not host[qi, mdist.SROW_MKEYS:mdist.SROW_SPEC].any()
    assert_equals_unsharded(mdist, qs[1:3], want[1:3], host[1:3], "next to declined ones")
    assert np.array_equal(mdist.merge_srows_np(hip.to_host(srows_all, (3, nq, m.SROW_WORDS)), 1024), host)
    # (b) + (c) on a batch of its own
    b2 = m.Batch(ctx, nq)
    narrow, wide = hip.malloc(nq * m.ROW_WORDS * 8), hip.malloc(nq * m.SROW_WORDS * 8)
    seg = m.Segment(ctx, corpus.shards[0], rowid_base=0)
    try:
        seg.set_attrs(corpus.shard_rows[0])
        chk(lib.mrk_batch_set_rows_dst(b2._h, narrow))
        assert lib.mrk_batch_set_srows_dst(b2._h, wide) == -1  # MRK_E_INVAL
        b2.submit(seg, qs)
        b2.wait()
        rows = hip.to_host(narrow, (nq, m.ROW_WORDS))
        for qi in (0, 1, 3):
            assert int(rows[qi, K1 + 1]) == mdist.ROW_DECLINED and int(rows[qi, K1]) == 0 and not rows[qi, :K1].any()
        assert not int(rows[2, K1 + 1]) & mdist.ROW_DECLINED and int(rows[2, K1]) == 100
        # ... while the same results exported as wide rows answer the sorted queries
        b2.export_srows(wide.value)
        w = hip.to_host(wide, (nq, m.SROW_WORDS))
        assert all(int(w[qi, K1]) == 100 and not int(w[qi, K1 + 1]) & mdist.ROW_DECLINED for qi in range(nq))
        chk(lib.mrk_batch_set_rows_dst(b2._h, None))
        chk(lib.mrk_batch_set_srows_dst(b2._h, wide))
        assert lib.mrk_batch_set_rows_dst(b2._h, narrow) == -1
        # a standing wide destination writes what the export writes
        hip.fill(wide, 0xEE, nq * m.SROW_WORDS * 8)
        b2.submit(seg, qs)
        b2.wait()
        assert np.array_equal(hip.to_host(wide, (nq, m.SROW_WORDS)), w)
        chk(lib.mrk_batch_set_srows_dst(b2._h, None))
    finally:
        seg.close()
        b2.close()
    hip.free()


def test_overflowed_shard_is_rerun_and_merged_exactly(dev):
    """Item 9: one shard of 3 M docs whose bool column puts half of ~2.4 M matches on the best key (the candidate list overflows)
    plus one small shard, with a standing wide destination: the big shard's row leaves with MRK_ROW_RERUN; after mrk_batch_wait +
    mrk_batch_export_srows the merge equals the unsharded result."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    n_big, n_small = 3_000_000, 50_001
    n_docs, cuts = n_big + n_small, [0, n_big, n_big + n_small]
    c = smc.Corpus(m, make_rows, n_docs, cuts, [0.8, 0.3], seed=5, rows_seed=21, max_pos=16)
    o, cnt, kind = sorts(m)["bool"]
    qs = [c.globalize(m.Query(kw(m, 0, 1), ranker=m.SPH_RANK_BM25, max_matches=1000, sort=m.Sort(o, cnt, desc=True, then_weight=1, kind=kind))),
          c.globalize(m.Query(m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2)), ranker=m.SPH_RANK_BM25, max_matches=1000))]
    nq, RW = len(qs), m.SROW_WORDS
    want = unsharded(m, ctx, batch, c, qs)
    assert want[0].total_found > 2 * 2 ** 20 and want[0].status == 0
    srows_all = hip.malloc(2 * nq * RW * 8)
    hip.fill(srows_all, 0xEE, 2 * nq * RW * 8)
    b2 = m.Batch(ctx, nq)
    for s in range(2):
        seg = m.Segment(ctx, c.shards[s], rowid_base=cuts[s])
        try:
            seg.set_attrs(c.shard_rows[s])
            chk(lib.mrk_batch_set_srows_dst(b2._h, off(srows_all, s * nq * RW * 8)))
            b2.submit(seg, qs)
            b2.wait()
            n_rerun = b2.stats()["n_rerun"]
            row = hip.to_host(off(srows_all, s * nq * RW * 8), (nq, RW))
            if s == 0:
                assert n_rerun >= 1  # the overflow must happen, else this test shows nothing
                assert int(row[0, K1 + 1]) == mdist.ROW_RERUN and int(row[0, K1]) == 0 and not row[0, :K1].any()
                first = merge(m, ctx, hip, srows_all, 1, nq)
                assert int(first[0, K1 + 1]) & mdist.ROW_RERUN
                b2.export_srows(srows_all.value)  # the rerun's result, mapped keys included
                row = hip.to_host(srows_all, (nq, RW))
                assert int(row[0, K1]) == 1000 and not int(row[0, K1 + 1]) & mdist.ROW_RERUN
            else:
                assert n_rerun == 0
            assert not int(row[1, K1 + 1]) & (mdist.ROW_RERUN | mdist.ROW_DECLINED)
        finally:
            seg.close()
    chk(lib.mrk_batch_set_srows_dst(b2._h, None))
    b2.close()
    host = merge(m, ctx, hip, srows_all, 2, nq)
    assert_equals_unsharded(mdist, qs, want, host, "rerun")
    hip.free()


@pytest.mark.parametrize("mode", ["lib-comm", "torch"])
def test_sorted_exchange_chain_one_rank(mode):
    """Item 10: ShardMerger(sorted_rows=True) with one rank, through the library's communicator and through torch.distributed."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(here, "dist_sort_chain_worker.py")] + (["--lib-comm"] if mode == "lib-comm" else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sorted dist chain ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
