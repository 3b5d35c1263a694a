"""GPU: weight-first orders (Order.weight_first: ORDER BY weight() DESC, attr | weight() ASC [, attr]) answered across segments and
shards through ORDER rows whose spec word carries OSPEC_WFIRST -- opt-in per batch (mrk_batch_orows_weight_first), off by default.
The merge kernel must equal the order's definition (a lexsort in weight_first_merge_common.py) and dist.merge_orows_np word for word;
the shards' rows merged must equal the unsharded device answer, itself checked against the oracle; a standing destination writes what
the export writes; an overflowed query leaves MRK_ROW_RERUN and comes back repaired; whatever cannot be answered is loud.  Every
comparison is exact."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import order_merge_common as omc
import sort_merge_common as smc
import weight_first_merge_common as wmc
from test_gpu_order_merge import Hip
from test_gpu_parity import kw, orc_index_of
from test_gpu_sort import AUX, BITS, TS
from test_gpu_sort import random_queries as random_sort_queries
from test_gpu_sort_merge import L, unsharded
from test_gpu_weight_first import BIG, Expect, make_rows, orders

pytestmark = pytest.mark.gpu

K1 = 1024
N_DOCS, CUTS = 60_001, [0, 16_385, 40_003, 60_001]  # no cut is a multiple of 128
PROBS = [0.5, 0.5, 0.3, 0.5, 0.5]
KS = (1, 10, 1000, 1024)


class Corpus2(smc.Corpus):
    """smc.Corpus over two fields: under BM25 the weight is then the matched fields' alone -- a handful of classes thousands of rows deep"""

    def __init__(self, m, n_docs, cuts, probs, seed, rows_seed):
        self.n_docs, self.cuts, self.nt = n_docs, list(cuts), len(probs)
        mk = lambda n, base: m.synth_index(n, probs, seed=seed, n_fields=2, skiplist_block_size=128, max_pos=16, rowid_base=base)
        self.whole = mk(n_docs, 0)
        self.shards = [mk(cuts[i + 1] - cuts[i], cuts[i]) for i in range(len(cuts) - 1)]
        self.gdocs = {t: int(self.whole.dict[t]["docs"]) for t in range(self.nt)}
        assert all(self.gdocs[t] == sum(int(sh.dict[t]["docs"]) for sh in self.shards) for t in range(self.nt))
        self.rows = make_rows(np.random.default_rng(rows_seed), n_docs)
        self.shard_rows = [np.ascontiguousarray(self.rows[cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1)]


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

    return Corpus2(m, N_DOCS, CUTS, PROBS, seed=2027, rows_seed=47)


def merge(m, ctx, hip, orows_all, n_lists, nq, k=1024):
    lib, chk = L()
    out = hip.malloc(nq * m.OROW_WORDS * 8)
    hip.fill(out, 0xEE, nq * m.OROW_WORDS * 8)
    chk(lib.mrk_topk_merge_orows(ctx._h, orows_all, n_lists, nq, k, out))
    return hip.to_host(out, (nq, m.OROW_WORDS))


def is_wf(q):
    return q.order is not None and bool(q.order.weight_first)


def assert_declined_row(mdist, row, what):
    assert int(row[K1 + 1]) == mdist.ROW_DECLINED and int(row[K1]) == 0 and not row[:K1].any() and not row[K1 + 2:].any(), what  # (no mapped keys, spec word 0)


def check_wf_row(mdist, q, row, rid, w, okey, total, what):
    """A weight-first query's order row against an answer (global docids, weights, raw order keys or None, total_found)"""
    assert not int(row[K1 + 1]) & (mdist.ROW_RERUN | mdist.ROW_DECLINED), (what, "flagged")
    omc.assert_padding(mdist, row)
    spec = int(row[mdist.OROW_SPEC])
    assert spec == wmc.query_spec(q) and spec & mdist.OSPEC_WFIRST, (what, hex(spec))
    docid, weight, tot = omc.decode_orow(row, q.max_matches)
    assert tot == total, (what, tot, total)
    assert len(docid) == len(rid) and np.array_equal(docid, rid), (what, q.order, q.max_matches, docid[:8], rid[:8])
    assert np.array_equal(weight, w), (what, weight[:8], w[:8])
    vals = mdist.unmap_order_keys(spec, mdist.orow_mkeys(row)[:len(docid)])
    if okey is None:
        assert not q.order.parts and not vals.any() and not mdist.orow_mkeys(row).any(), what
    else:
        assert np.array_equal(vals, omc.fold_order_zero(okey, q.order)), (what, q.order, vals[:4], okey[:4])


def test_merge_kernel_equals_the_definition(dev):
    """The synthetic lists of test_weight_first_merge_cpu.py through mrk_topk_merge_orows into a 0xEE-filled destination: whole rows
    equal the definition's and merge_orows_np's; mrk_topk_merge_orows_part on a query slice; the loud cases."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    RW, NQ = m.OROW_WORDS, wmc.NQ
    dev_in, out, recv, part = hip.malloc(8 * NQ * RW * 8), hip.malloc(NQ * RW * 8), hip.malloc(8 * 2 * RW * 8), hip.malloc(NQ * RW * 8)

    def run(rows, k):
        hip.to_dev(dev_in, rows)
        hip.fill(out, 0xEE, NQ * RW * 8)
        chk(lib.mrk_topk_merge_orows(ctx._h, dev_in, rows.shape[0], NQ, k, out))
        return hip.to_host(out, (NQ, RW))

    levels = {fl: set() for fl in wmc.FLAVORS}
    for (f, wf, n, k), (rows, want) in wmc.size_references().items():
        got = run(rows, k)
        assert np.array_equal(got, want), (f, wf, n, k)
        assert np.array_equal(got, mdist.merge_orows_np(rows, k)), (f, wf, n, k)
        if n > 1:
            levels[(f, wf)] |= wmc.levels_decided(rows, k)
        if k == 7:  # the partitioned form on the query slice [1, 3): lists [l][2 rows]; row 0 of the destination is not touched
            hip.to_dev(recv, np.ascontiguousarray(rows[:, 1:3]))
            hip.fill(part, 0xEE, NQ * RW * 8)
            chk(lib.mrk_topk_merge_orows_part(ctx._h, recv, n, 2, 1, 2, k, part))
            hp = hip.to_host(part, (NQ, RW))
            assert np.array_equal(hp[1:], want[1:]) and (hp[0] == np.uint64(0xEEEEEEEEEEEEEEEE)).all(), (f, wf, n)
    for (f, wf), seen in levels.items():  # ties decided by the weight, the mapped key, the docid -- between entries of different lists
        assert seen == ({1, 3} if f == "none" else {1, 2, 3}), (f, wf, seen)
    for name, rows in wmc.loud_cases():
        for k in (7, 1024):
            got = run(rows, k)
            wmc.assert_loud(mdist, rows, got, name)
            assert np.array_equal(got, mdist.merge_orows_np(rows, k)), (name, k)
        if name.startswith("declined-spec0"):  # the same row whichever list declined
            assert np.array_equal(run(rows[::-1].copy(), 1024), got), name
    hip.free()


def shard_rows_of(m, ctx, batch, hip, corpus, qs, on):
    """every shard's exported order rows of the batch with the switch `on` -> host [S][nq][OROW_WORDS]"""
    nq, RW, S = len(qs), m.OROW_WORDS, len(corpus.shards)
    buf = hip.malloc(S * nq * RW * 8)
    hip.fill(buf, 0xEE, S * nq * RW * 8)
    batch.orows_weight_first(on)
    for s in range(S):
        seg = m.Segment(ctx, corpus.shards[s], rowid_base=corpus.cuts[s])
        try:
            seg.set_attrs(corpus.shard_rows[s])
            batch.submit(seg, qs)
            batch.wait()
            st = batch.stats()
            assert st["n_rerun"] == 0 and st["packed"] == 1  # a rerun or a decline would be a bug, not a limit: the premise is asserted by the caller
            assert [r.status for r in batch.results()] == [0] * nq, ("no query may be declined on a shard", s)
            batch.export_orows(buf.value + s * nq * RW * 8)
        finally:
            seg.close()
    batch.orows_weight_first(False)
    return buf, hip.to_host(buf, (S, nq, RW))


def test_sharded_weight_first_equals_unsharded(orc, dev, corpus):
    """60 001 docs in three uneven shards.  The premise, from the oracle's full answer: the K-th row's weight class is deeper than K and
    spans at least two shards at every K asked, from either end; every shard's match count stays below 2^20."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    X = m.XQNode
    deep = X.AND(kw(m, 0, 1), kw(m, 1, 2))
    PHRASE, FIVE = X(m.SPH_QUERY_PHRASE, [kw(m, 0, 1), kw(m, 1, 2)]), X.AND(*[kw(m, j, j + 1) for j in range(5)])
    O = orders(m)
    qs = []
    for r, ranker in enumerate((m.SPH_RANK_NONE, m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25)):
        for i, o in enumerate(O):
            qs.append(m.Query(deep, ranker=ranker, max_matches=KS[(i + r) % 4], order=o))
    qs += [m.Query(deep, ranker=m.SPH_RANK_BM25, max_matches=K, order=O[(5 * j) % len(O)]) for j, K in enumerate(KS + KS)]
    qs += [m.Query(PHRASE, ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=1000, order=O[1]), m.Query(FIVE, ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=1000, order=O[14]),
           m.Query(PHRASE, ranker=m.SPH_RANK_BM25, max_matches=10, order=O[16])]
    rng = np.random.default_rng(8)
    S = random_sort_queries(m, rng, corpus.nt, 6)
    rel = [dataclasses.replace(q, sort=None) for q in random_sort_queries(m, rng, corpus.nt, 6)]
    att = [m.Query(deep, ranker=m.SPH_RANK_BM25, max_matches=1000, order=m.Order([m.OrderPart(BITS * 32 + 3, 3, desc=True), m.OrderPart(TS * 32, 32, desc=False)], then_weight=t)) for t in (0, 1, 2)]
    att.append(m.Query(deep, ranker=m.SPH_RANK_BM25, max_matches=100, order=m.Order([m.OrderPart(BIG * 32, 64, desc=True, kind=m.SORTKEY_INT64)], then_weight=1)))
    others = [q for trio in zip(rel, S) for q in trio] + att
    step = len(qs) // len(others)
    for j, q in enumerate(others):  # in between
        qs.insert(j * (step + 1), q)
    qs = [corpus.globalize(q) for q in qs]
    nq = len(qs)
    assert nq <= 256 and sum(is_wf(q) for q in qs) >= 60
    oi = orc_index_of(orc, corpus.whole)
    oi.attrs = corpus.rows
    E = Expect(orc, oi, corpus.rows, N_DOCS)
    # ---- the premise
    bm = next(q for q in qs if is_wf(q) and q.ranker == m.SPH_RANK_BM25 and q.root is deep)
    full = E.matches(bm)
    shard_of = np.searchsorted(np.array(CUTS[1:]), full.rowid, side="right")
    ws = np.sort(full.weight.astype(np.int64))
    for K in KS:
        for kth in (ws[::-1][K - 1], ws[K - 1]):
            cls = full.weight == kth
            assert int(cls.sum()) > K and len(np.unique(shard_of[cls])) >= 2, (K, int(kth), int(cls.sum()))
    assert full.total_found < 2 ** 20 and max(CUTS[i + 1] - CUTS[i] for i in range(3)) < 2 ** 20
    # ---- the unsharded device answer against the oracle
    want = unsharded(m, ctx, batch, corpus, qs)
    assert batch.stats()["n_rerun"] == 0
    E.check(qs, want, "unsharded")
    # ---- the shards' rows, switch on and off
    buf_on, rows_on = shard_rows_of(m, ctx, batch, hip, corpus, qs, True)
    _, rows_off = shard_rows_of(m, ctx, batch, hip, corpus, qs, False)
    for qi, q in enumerate(qs):
        if is_wf(q):
            for s in range(3):
                assert_declined_row(mdist, rows_off[s, qi], ("switch off", s, qi))
        else:
            assert np.array_equal(rows_on[:, qi], rows_off[:, qi]), ("a row of another query changed with the switch", qi)
    for k in (1024, 10):
        host = merge(m, ctx, hip, buf_on, 3, nq, k=k)
        assert np.array_equal(host, mdist.merge_orows_np(rows_on, k)), k
        if k != 1024:
            continue
        for qi, (q, w) in enumerate(zip(qs, want)):
            if is_wf(q):
                check_wf_row(mdist, q, host[qi], w.rowid, w.weight, w.order_key, w.total_found, ("merged", qi))
                assert (w.order_key is None) == (not q.order.parts)
            else:
                raw = w.order_key if q.order is not None else w.sort_key
                omc.check_merged_orow(mdist, (w.rowid, w.weight, None, raw, w.total_found), q, host[qi], ("merged", qi))
    hip.free()


def test_standing_destination_equals_export(dev, corpus):
    """Switch on: a standing order-row destination holds what mrk_batch_export_orows writes after the wait, for a mixed batch and for
    the same batch submitted again; switched off again on the same batch the weight-first rows are declined as ever; switched on,
    narrow and wide destinations still decline them."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    rng = np.random.default_rng(21)
    O = orders(m)
    S = random_sort_queries(m, rng, corpus.nt, 8)
    rel = [dataclasses.replace(q, sort=None) for q in random_sort_queries(m, rng, corpus.nt, 8)]
    big = [dataclasses.replace(q, sort=None, order=m.Order([m.OrderPart(BIG * 32, 64, kind=m.SORTKEY_INT64)])) for q in random_sort_queries(m, rng, corpus.nt, 3)]
    wfq = [dataclasses.replace(q, sort=None, order=O[i % len(O)]) for i, q in enumerate(random_sort_queries(m, rng, corpus.nt, len(O)))]
    others = [q for pair in zip(rel, S) for q in pair] + big
    qs = [corpus.globalize(q) for pair in zip(others, wfq) for q in pair] + [corpus.globalize(q) for q in others[len(wfq):] + wfq[len(others):]]
    nq, RW = len(qs), m.OROW_WORDS
    wf = [is_wf(q) for q in qs]
    assert sum(wf) == len(O) and nq == len(O) + len(others)
    b2 = m.Batch(ctx, nq)
    standing_buf, exported = hip.malloc(nq * RW * 8), hip.malloc(nq * RW * 8)
    seg = m.Segment(ctx, corpus.shards[1], rowid_base=CUTS[1])
    try:
        seg.set_attrs(corpus.shard_rows[1])

        def run(standing):
            """(the standing destination's rows or None, the exported rows, the batch's own answer)"""
            st = None
            if standing:
                hip.fill(standing_buf, 0xEE, nq * RW * 8)
                chk(lib.mrk_batch_set_orows_dst(b2._h, standing_buf))
            b2.submit(seg, qs)
            b2.wait()
            assert b2.stats()["n_rerun"] == 0
            if standing:
                st = hip.to_host(standing_buf, (nq, RW))
                chk(lib.mrk_batch_set_orows_dst(b2._h, None))
            res = b2.results()
            assert [r.status for r in res] == [0] * nq
            hip.fill(exported, 0xEE, nq * RW * 8)
            b2.export_orows(exported.value)
            return st, hip.to_host(exported, (nq, RW)), res

        _, off_rows, _ = run(False)  # the default: off
        b2.orows_weight_first(True)
        st1, exp1, res = run(True)
        assert np.array_equal(st1, exp1)
        st2, exp2, _ = run(True)  # the same batch again
        assert np.array_equal(st2, exp1) and np.array_equal(exp2, exp1)
        _, exp3, _ = run(False)  # and without a standing destination the export is the same
        assert np.array_equal(exp3, exp1)
        for qi, (q, g) in enumerate(zip(qs, res)):  # the rows hold the batch's own answer
            if wf[qi]:
                check_wf_row(mdist, q, exp1[qi], g.rowid.astype(np.int64) + CUTS[1], g.weight, g.order_key, g.total_found, ("standing", qi))
                assert_declined_row(mdist, off_rows[qi], ("default off", qi))
            else:
                assert np.array_equal(exp1[qi], off_rows[qi]), qi
        # switched off again on the same batch: declined exactly as ever, standing and exported
        b2.orows_weight_first(False)
        st4, exp4, _ = run(True)
        assert np.array_equal(st4, off_rows) and np.array_equal(exp4, off_rows)
        # switched on: narrow and wide rows still decline a weight-first query, standing and exported
        b2.orows_weight_first(True)
        for kind, W in (("rows", m.ROW_WORDS), ("srows", m.SROW_WORDS)):
            dst = hip.malloc(nq * W * 8)
            hip.fill(dst, 0xEE, nq * W * 8)
            chk(getattr(lib, f"mrk_batch_set_{kind}_dst")(b2._h, dst))
            b2.submit(seg, qs)
            b2.wait()
            chk(getattr(lib, f"mrk_batch_set_{kind}_dst")(b2._h, None))
            st_rows = hip.to_host(dst, (nq, W))
            hip.fill(dst, 0xEE, nq * W * 8)
            chk(getattr(lib, f"mrk_batch_export_{kind}")(b2._h, dst))
            ex_rows = hip.to_host(dst, (nq, W))
            assert np.array_equal(st_rows, ex_rows), kind
            for qi in range(nq):
                if wf[qi]:
                    assert_declined_row(mdist, st_rows[qi], (kind, qi))
    finally:
        seg.close()
        b2.close()
    hip.free()


def test_overflowed_weight_first_row_is_rerun_and_repaired(orc, dev):
    """One keyword in ~95 % of 1.2 M docs under ranker NONE: every match weighs 1 and lands in one bin, more than the candidate list's
    2^20 slots (the smallest size that overflows).  Switch on, standing order-row destination: the standing row leaves MRK_ROW_RERUN
    with no keys; after the wait the exported row is the repaired one and equals the oracle's expectation."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    n_docs = 1_200_000
    hi = m.synth_index(n_docs, [0.95, 0.3], seed=7, skiplist_block_size=128, max_pos=16)
    rows = make_rows(np.random.default_rng(13), n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    oi.attrs = rows
    b2 = m.Batch(ctx, 8)
    RW = m.OROW_WORDS
    try:
        seg.set_attrs(rows)
        q = m.Query(kw(m, 0, 1), ranker=m.SPH_RANK_NONE, max_matches=1000, order=m.Order([m.OrderPart(AUX * 32, 32, desc=True)], weight_first=1))
        plain = m.Query(kw(m, 1, 1), ranker=m.SPH_RANK_BM25, max_matches=100)
        dst = hip.malloc(2 * RW * 8)
        hip.fill(dst, 0xEE, 2 * RW * 8)
        b2.orows_weight_first(True)
        chk(lib.mrk_batch_set_orows_dst(b2._h, dst))
        b2.submit(seg, [plain, q])
        b2.wait()
        assert b2.stats()["n_rerun"] == 1
        got = b2.results()
        chk(lib.mrk_batch_set_orows_dst(b2._h, None))
        assert got[1].status == 0 and got[1].total_found > 2 ** 20
        standing = hip.to_host(dst, (2, RW))
        assert int(standing[1, K1 + 1]) == mdist.ROW_RERUN and int(standing[1, K1]) == 0 and not standing[1, :K1].any() and not standing[1, K1 + 2:mdist.OROW_SPEC].any()
        assert int(standing[0, K1]) == len(got[0].rowid) and int(standing[0, K1 + 1]) == got[0].total_found and int(standing[0, -1]) == 0
        hip.fill(dst, 0xEE, 2 * RW * 8)
        b2.export_orows(dst.value)
        row = hip.to_host(dst, (2, RW))
        assert np.array_equal(row[0], standing[0])
        from weight_first_expect import expected_weight_first

        rid, w, okey, total = expected_weight_first(orc, oi, q, rows, n_docs)
        check_wf_row(mdist, q, row[1], rid, w, okey, total, "repaired")
    finally:
        seg.close()
        b2.close()
    hip.free()


@pytest.mark.parametrize("mode", ["lib-comm", "torch"])
def test_weight_first_exchange_chain_one_rank(mode):
    """ShardMerger(order_rows=True, weight_first=True) with one rank, through the library's communicator and through torch.distributed."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(here, "dist_weight_first_chain_worker.py")] + (["--lib-comm"] if mode == "lib-comm" else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "weight-first dist chain ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_the_switch_refuses_what_it_cannot_mean(dev):
    m, ctx, batch, hip = dev
    from manticoresearch_amd import _lib

    lib = _lib.lib()
    for bad in (2, -1, 256):
        assert lib.mrk_batch_orows_weight_first(batch._h, bad) == _lib.MRK_E_INVAL, bad
    assert lib.mrk_batch_orows_weight_first(None, 1) == _lib.MRK_E_INVAL
    assert lib.mrk_batch_orows_weight_first(batch._h, 1) == 0 and lib.mrk_batch_orows_weight_first(batch._h, 0) == 0
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mrk.h")).read()
    assert "int mrk_batch_orows_weight_first(mrk_batch* b, int on);" in hdr
