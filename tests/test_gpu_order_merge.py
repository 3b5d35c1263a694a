"""GPU: queries ordered by a 64-bit key (Query.order: a bigint, or two attributes) answered across segments and shards through the
ORDER rows (MRK_OROW_WORDS): the shards' exported rows merged by mrk_topk_merge_orows must equal the unsharded device result bit
for bit, ties at rank K included; the kernel must equal its numpy mirror (dist.merge_orows_np) word for word; a relevance-only
batch must come out as the narrow merge gives it; a standing order-row destination writes what the export writes; and whatever
cannot be answered must be loud.  Every comparison is exact."""
import copy
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import order_merge_common as omc
import sort_merge_common as smc
from test_gpu_order import BIG, CONST, FLT, ID, TS, all_orders, check, make_rows, part_specs, random_queries
from test_gpu_parity import kw, orc_index_of
from test_gpu_sort import random_queries as random_sort_queries
from test_gpu_sort_merge import Hip as _Hip
from test_gpu_sort_merge import L, off, unsharded

pytestmark = pytest.mark.gpu

K1 = 1024
N_DOCS, CUTS = 700_001, [0, 131_072, 400_003, 700_001]
PROBS = [0.35, 0.2, 0.1, 0.05, 0.04, 0.02, 0.01, 0.006]


class Hip(_Hip):
    """test_gpu_sort_merge's helper with every fill and copy finished before it returns.  hipMemset and a device-to-device hipMemcpy
    on the null stream may return before the device has done them, and a batch's stream is non-blocking: nothing else would order a
    0xEE fill before the kernels that write the rows the test then reads."""

    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0

    def fill(self, p, byte, n):
        super().fill(p, byte, n)
        self.sync()

    def d2d(self, dst, src, n):
        super().d2d(dst, src, n)
        self.sync()

    def to_dev(self, p, a):
        super().to_dev(p, a)
        self.sync()


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

    c = smc.Corpus(m, make_rows, N_DOCS, CUTS, PROBS, seed=2026, rows_seed=43)
    assert all(CUTS[i + 1] - CUTS[i] < 2 ** 20 for i in range(3))  # below the candidate list's 2^20 slots: a decline or a rerun is a bug
    return c


def shard_orows(m, ctx, batch, hip, corpus, qs, shard_rows=None, allow_declined=False):
    """Every shard's order rows of the batch, exported behind mrk_batch_wait -> device [S][nq][OROW_WORDS]; the per-shard statuses."""
    nq, RW, S = len(qs), m.OROW_WORDS, len(corpus.shards)
    orows_all = hip.malloc(S * nq * RW * 8)
    hip.fill(orows_all, 0xEE, S * nq * RW * 8)
    statuses = []
    for s in range(S):
        seg = m.Segment(ctx, corpus.shards[s], rowid_base=corpus.cuts[s])
        try:
            seg.set_attrs((shard_rows or corpus.shard_rows)[s])
            batch.submit(seg, qs)
            batch.wait()
            assert batch.stats()["n_rerun"] == 0 and batch.stats()["packed"] == 1
            st = [r.status for r in batch.results()]
            if not allow_declined:
                assert st == [0] * nq, ("no query may be declined on a shard", s, st)
            statuses.append(st)
            batch.export_orows(orows_all.value + s * nq * RW * 8)
        finally:
            seg.close()
    return orows_all, statuses


def merge(m, ctx, hip, orows_all, n_lists, nq, k=1024):
    lib, chk = L()
    out = hip.malloc(nq * m.OROW_WORDS * 8)
    hip.fill(out, 0xEE, nq * m.OROW_WORDS * 8)
    chk(lib.mrk_topk_merge_orows(ctx._h, orows_all, n_lists, nq, k, out))
    return hip.to_host(out, (nq, m.OROW_WORDS))


def assert_equals_unsharded(mdist, qs, want, host, what):
    """rowids, weights, unmapped order_key / sort_key, totals, zero padding, spec words; no row flagged"""
    for qi, (q, w) in enumerate(zip(qs, want)):
        assert w.status == 0, (what, qi, "no query of this test may be declined")
        raw = w.order_key if q.order is not None else w.sort_key
        assert (raw is not None) == (q.order is not None or q.sort is not None)
        omc.check_merged_orow(mdist, (w.rowid, w.weight, None, raw, w.total_found), q, host[qi], (what, qi))


def mixed_queries(m, corpus, n, seed, every=False):
    """test_gpu_order.random_queries' shapes under random orders (+ every column and pair once), relevance and Sort queries in between"""
    rng = np.random.default_rng(seed)
    qs = []
    sorts_ = random_sort_queries(m, rng, corpus.nt, n // 3 + 1)
    for i, q in enumerate(random_queries(m, rng, corpus.nt, n)):
        qs.append(q)
        if i % 3 == 1:
            qs.append(dataclasses.replace(q, order=None))
        if i % 3 == 2:
            qs.append(sorts_[i // 3])
    if every:
        root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
        qs += [m.Query(root, ranker=[m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25][i % 2], max_matches=[10, 1000][i % 2], order=o) for i, o in enumerate(all_orders(m))]
        qs.append(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=100, order=m.Order([m.OrderPart(TS * 32, 32, desc=False)], then_weight=2)))  # one part: a sort
    return [corpus.globalize(q) for q in qs]


def test_sharded_ordered_equals_unsharded(orc, dev, corpus):
    """Three uneven shards of 700 001 docs; the unsharded device result is checked against the oracle on a subset, then the merge of
    the shards' order rows must equal it for every query; the kernel equals merge_orows_np word for word, and so does the partitioned
    form.  No query is declined, rerun or skipped."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    RW = m.OROW_WORDS
    for rnd in range(2):
        qs = mixed_queries(m, corpus, 120 if rnd == 0 else 150, 5100 + rnd, every=rnd == 0)
        nq = len(qs)
        assert nq <= 256
        kinds = [("order" if q.order is not None else "sort" if q.sort is not None else "rel") for q in qs]
        assert kinds.count("order") >= 100 and kinds.count("sort") >= 20 and kinds.count("rel") >= 20
        want = unsharded(m, ctx, batch, corpus, qs)
        assert batch.stats()["n_rerun"] == 0 and [w.status for w in want] == [0] * nq
        if rnd == 0:  # the unsharded device result against the oracle, on a subset the oracle can afford
            oi = orc_index_of(orc, corpus.whole)
            oi.attrs = corpus.rows
            sub = [i for i, k_ in enumerate(kinds) if k_ == "order"][:4] + [i for i, k_ in enumerate(kinds) if k_ == "sort"][:1] + [i for i, k_ in enumerate(kinds) if k_ == "rel"][:1]
            check(orc, oi, corpus.rows, N_DOCS, [qs[i] for i in sub], [want[i] for i in sub], "unsharded")
        orows_all, _ = shard_orows(m, ctx, batch, hip, corpus, qs)
        host = merge(m, ctx, hip, orows_all, 3, nq)
        assert_equals_unsharded(mdist, qs, want, host, f"round {rnd}")
        # the kernel equals its mirror
        host_in = hip.to_host(orows_all, (3, nq, RW))
        assert np.array_equal(mdist.merge_orows_np(host_in, 1024), host)
        assert np.array_equal(mdist.merge_orows_np(host_in, 10), merge(m, ctx, hip, orows_all, 3, nq, k=10))
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
                hip.d2d(off(recv, s * per * RW * 8), off(orows_all, (s * nq + f.value) * RW * 8), c.value * RW * 8)
            chk(lib.mrk_topk_merge_orows_part(ctx._h, recv, 3, per, f.value, c.value, 1024, part))
        assert covered == nq
        assert np.array_equal(hip.to_host(part, (nq, RW)), host)
        hip.free()


def test_relevance_batches_merge_as_the_narrow_rows_do(dev, corpus):
    """Spec 0 parity: words 0..1025 of the order-row merge are the narrow rows mrk_topk_merge_rows gives for the same shards."""
    m, ctx, batch, hip = dev
    lib, chk = L()
    qs = [dataclasses.replace(q, order=None, sort=None) for q in mixed_queries(m, corpus, 45, 99)]
    nq, RW, NW = len(qs), m.OROW_WORDS, m.ROW_WORDS
    orows_all, rows_all = hip.malloc(3 * nq * RW * 8), hip.malloc(3 * nq * NW * 8)
    for s in range(3):
        seg = m.Segment(ctx, corpus.shards[s], rowid_base=corpus.cuts[s])
        try:
            seg.set_attrs(corpus.shard_rows[s])
            batch.submit(seg, qs)
            batch.wait()
            assert [r.status for r in batch.results()] == [0] * nq
            batch.export_orows(orows_all.value + s * nq * RW * 8)
            chk(lib.mrk_batch_export_rows(batch._h, off(rows_all, s * nq * NW * 8)))
        finally:
            seg.close()
    for k in (1024, 37):
        wide = merge(m, ctx, hip, orows_all, 3, nq, k=k)
        out = hip.malloc(nq * NW * 8)
        chk(lib.mrk_topk_merge_rows(ctx._h, rows_all, 3, nq, k, out))
        narrow = hip.to_host(out, (nq, NW))
        assert np.array_equal(wide[:, :NW], narrow)
        assert not wide[:, NW:].any()  # no mapped keys, spec 0
        assert narrow[:, K1].max() > 0
    hip.free()


def test_ties_at_rank_k_across_shards(orc, dev, corpus):
    """A bool first part plus a constant second part at K = 1000: (nearly) the whole top K shares one 64-bit key on every shard, the
    order is the tie rule's, then global docid.  And an `id` bigint whose values differ only in the low dword within a shard and only
    in the high dword across shards (high dwords -1, 0, 1): both dwords of the mapped key must decide in the merge."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    rows = corpus.rows.copy()
    for s in range(3):
        n = CUTS[s + 1] - CUTS[s]
        ids = (np.int64(s - 1) << np.int64(32)) + np.arange(n, dtype=np.int64) * 3
        rows[CUTS[s]:CUTS[s + 1], ID:ID + 2] = ids.view(np.uint32).reshape(n, 2)
    c2 = copy.copy(corpus)  # (the corpus object is shared: a shallow copy with the other rows)
    c2.rows = rows
    c2.shard_rows = [np.ascontiguousarray(rows[CUTS[i]:CUTS[i + 1]]) for i in range(3)]
    P = part_specs(m)
    o, cnt, kind = P["bool"]
    qs = []
    for root in (kw(m, 0, 1), m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))):
        for d, t in ((True, 1), (False, 2), (True, 0), (False, 1)):
            qs.append(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=1000, order=m.Order([m.OrderPart(o, cnt, desc=d, kind=kind), m.OrderPart(CONST * 32, 32, desc=not d)], then_weight=t)))
        for d in (True, False):
            for t in (0, 1):
                qs.append(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=1000, order=m.Order([m.OrderPart(ID * 32, 64, desc=d, kind=m.SORTKEY_INT64)], then_weight=t)))
    qs = [c2.globalize(q) for q in qs]
    want = unsharded(m, ctx, batch, c2, qs)
    for q, w in zip(qs, want):
        assert len(w.rowid) == 1000 and w.status == 0
        if len(q.order.parts) == 2:  # the premise: the whole top K sits on one key
            assert len(np.unique(w.order_key)) == 1
        else:  # all of one shard: one high dword, distinct low dwords
            assert len(np.unique(w.order_key >> np.uint64(32))) == 1 and len(np.unique(w.order_key)) == 1000
    oi = orc_index_of(orc, c2.whole)
    oi.attrs = rows
    check(orc, oi, rows, N_DOCS, [qs[0], qs[4], qs[-1]], [want[0], want[4], want[-1]], "ties, unsharded")
    orows_all, _ = shard_orows(m, ctx, batch, hip, c2, qs)
    host = merge(m, ctx, hip, orows_all, 3, len(qs))
    assert_equals_unsharded(mdist, qs, want, host, "ties")
    assert np.array_equal(mdist.merge_orows_np(hip.to_host(orows_all, (3, len(qs), m.OROW_WORDS)), 1024), host)
    # across the id's shards the merged top K comes from one shard only although every shard handed in K rows
    in_rows = hip.to_host(orows_all, (3, len(qs), m.OROW_WORDS))
    assert (in_rows[:, :, K1] == 1000).all()
    hip.free()


def test_standing_destinations(dev, corpus):
    """A standing order-row destination writes what the export writes; the three kinds of standing destination are mutually
    MRK_E_INVAL; with a narrow or a wide standing destination an Order query still leaves declined."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    qs = mixed_queries(m, corpus, 30, 7)
    nq = len(qs)
    is_wide = [q.order is not None for q in qs]  # (random_queries' orders are all 64-bit keys)
    assert sum(is_wide) >= 20 and any(q.sort is not None for q in qs) and any(q.sort is None and q.order is None for q in qs)
    b2 = m.Batch(ctx, nq)
    narrow, wide, orow, exported = (hip.malloc(nq * W * 8) for W in (m.ROW_WORDS, m.SROW_WORDS, m.OROW_WORDS, m.OROW_WORDS))
    dsts = {"rows": narrow, "srows": wide, "orows": orow}
    setter = {k_: getattr(lib, f"mrk_batch_set_{k_}_dst") for k_ in dsts}
    seg = m.Segment(ctx, corpus.shards[1], rowid_base=CUTS[1])
    try:
        seg.set_attrs(corpus.shard_rows[1])
        for a in dsts:  # every pair, in both orders
            chk(setter[a](b2._h, dsts[a]))
            for b in dsts:
                if b != a:
                    assert setter[b](b2._h, dsts[b]) == -1, (a, b)  # MRK_E_INVAL
                    chk(setter[b](b2._h, None))  # (cancelling what does not stand is no error)
            chk(setter[a](b2._h, dsts[a]))  # the same kind again: replaced
            chk(setter[a](b2._h, None))
        # the standing order-row destination
        hip.fill(orow, 0xEE, nq * m.OROW_WORDS * 8)
        chk(lib.mrk_batch_set_orows_dst(b2._h, orow))
        b2.submit(seg, qs)
        b2.wait()
        assert b2.stats()["n_rerun"] == 0
        standing = hip.to_host(orow, (nq, m.OROW_WORDS))
        chk(lib.mrk_batch_set_orows_dst(b2._h, None))
        assert [r.status for r in b2.results()] == [0] * nq
        hip.fill(exported, 0xEE, nq * m.OROW_WORDS * 8)
        b2.export_orows(exported.value)
        exp = hip.to_host(exported, (nq, m.OROW_WORDS))
        assert np.array_equal(standing, exp)
        b2.submit(seg, qs)  # and without a standing destination the export is the same
        b2.wait()
        hip.fill(exported, 0xEE, nq * m.OROW_WORDS * 8)
        b2.export_orows(exported.value)
        assert np.array_equal(hip.to_host(exported, (nq, m.OROW_WORDS)), exp)
        got = b2.results()
        for qi, (q, g) in enumerate(zip(qs, got)):  # the rows hold the batch's own answer
            assert int(exp[qi, K1]) == len(g.rowid) and int(exp[qi, K1 + 1]) == g.total_found and int(exp[qi, mdist.OROW_SPEC]) == omc.spec_of(mdist, q)
            docid, weight, _ = omc.decode_orow(exp[qi], 1024)
            assert np.array_equal(docid, g.rowid + CUTS[1]) and np.array_equal(weight, g.weight)
            omc.assert_padding(mdist, exp[qi])
            if q.order is not None:
                assert np.array_equal(mdist.unmap_order_keys(int(exp[qi, mdist.OROW_SPEC]), mdist.orow_mkeys(exp[qi])[:len(docid)]), omc.fold_order_zero(g.order_key, q.order))
        # a narrow or a wide standing destination: an Order query still leaves declined, zero count, zero keys
        for kind_, W in (("rows", m.ROW_WORDS), ("srows", m.SROW_WORDS)):
            hip.fill(dsts[kind_], 0xEE, nq * W * 8)
            chk(setter[kind_](b2._h, dsts[kind_]))
            b2.submit(seg, qs)
            b2.wait()
            chk(setter[kind_](b2._h, None))
            rows = hip.to_host(dsts[kind_], (nq, W))
            for qi, q in enumerate(qs):
                if is_wide[qi]:
                    assert int(rows[qi, K1 + 1]) == mdist.ROW_DECLINED and int(rows[qi, K1]) == 0 and not rows[qi, :K1].any() and not rows[qi, K1 + 2:].any(), (kind_, qi)
                elif q.sort is None or kind_ == "srows":
                    assert not int(rows[qi, K1 + 1]) & mdist.ROW_DECLINED and np.array_equal(rows[qi, :K1 + 2], exp[qi, :K1 + 2]), (kind_, qi)
        # ... and exported as narrow and wide rows too
        chk(lib.mrk_batch_export_rows(b2._h, narrow))
        b2.export_srows(wide.value)
        for rows in (hip.to_host(narrow, (nq, m.ROW_WORDS)), hip.to_host(wide, (nq, m.SROW_WORDS))):
            for qi in range(nq):
                if is_wide[qi]:
                    assert int(rows[qi, K1 + 1]) == mdist.ROW_DECLINED and int(rows[qi, K1]) == 0 and not rows[qi, :K1].any()
    finally:
        seg.close()
        b2.close()
    hip.free()


def test_loud_cases(dev, corpus):
    """(a) a NaN in one shard's float column: that shard declines the queries ordered by it, the merged rows carry MRK_ROW_DECLINED
    and no keys, the batch's other queries are exact; (b) lists whose spec words differ: the same."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    P = part_specs(m)
    root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
    part = lambda name, desc: m.OrderPart(P[name][0], P[name][1], desc=desc, kind=P[name][2])
    Q = lambda **kwa: corpus.globalize(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=100, **kwa))
    qs = [Q(order=m.Order([part("cat", True), part("float", False)], then_weight=1)), Q(order=m.Order([part("cat", True), part("ts", False)], then_weight=2)), Q(),
          Q(order=m.Order([part("float", True), part("bits5", True)], then_weight=0)), Q(order=m.Order([m.OrderPart(BIG * 32, 64, desc=False, kind=m.SORTKEY_INT64)])),
          Q(sort=m.Sort(P["ts"][0], P["ts"][1], desc=True, then_weight=1, kind=P["ts"][2]))]
    nq = len(qs)
    want = unsharded(m, ctx, batch, corpus, qs)
    nan_rows = [r.copy() for r in corpus.shard_rows]
    nan_rows[1][17, FLT] = 0x7FC00000
    orows_all, statuses = shard_orows(m, ctx, batch, hip, corpus, qs, shard_rows=nan_rows, allow_declined=True)
    assert statuses == [[0] * 6, [-2, 0, 0, -2, 0, 0], [0] * 6]
    host = merge(m, ctx, hip, orows_all, 3, nq)
    host_in = hip.to_host(orows_all, (3, nq, m.OROW_WORDS))
    for qi in (0, 3):
        assert int(host_in[1, qi, K1 + 1]) == mdist.ROW_DECLINED and not host_in[1, qi, :K1 + 1].any() and not host_in[1, qi, K1 + 2:].any()
        assert int(host[qi, K1 + 1]) & mdist.ROW_DECLINED and int(host[qi, K1]) == 0
        assert int(host[qi, K1 + 1]) & ~mdist.ROW_DECLINED == int(host_in[0, qi, K1 + 1]) + int(host_in[2, qi, K1 + 1])  # totals are carried
        assert not host[qi, :K1].any() and not host[qi, mdist.OROW_MKEYS:mdist.OROW_SPEC].any()
        # the declining shard sent spec 0; the merged row stands under the answering shards' spec word ...
        assert int(host_in[1, qi, mdist.OROW_SPEC]) == 0 and int(host[qi, mdist.OROW_SPEC]) == omc.spec_of(mdist, qs[qi]) != 0
    keep = [1, 2, 4, 5]
    assert_equals_unsharded(mdist, [qs[i] for i in keep], [want[i] for i in keep], host[keep], "next to declined ones")
    assert np.array_equal(mdist.merge_orows_np(host_in, 1024), host)
    perm_in = hip.malloc(3 * nq * m.OROW_WORDS * 8)  # ... and is the same whichever list declined
    for perm in ([1, 0, 2], [0, 2, 1]):
        hip.to_dev(perm_in, host_in[perm])
        assert np.array_equal(merge(m, ctx, hip, perm_in, 3, nq), host), perm
    # (b) the good shards' rows with one list's spec word changed: a bit of the second part, the tie rule, a sort next to an order, a
    # relevance row next to an order, an order row next to relevance rows
    good_in = host_in.copy()
    good_in[1] = hip.to_host(shard_orows(m, ctx, batch, hip, corpus, qs)[0], (3, nq, m.OROW_WORDS))[1]
    good = mdist.merge_orows_np(good_in, 1024)
    assert_equals_unsharded(mdist, qs, want, good, "good rows")
    spec, sort_spec = int(good_in[0, 1, mdist.OROW_SPEC]), int(good_in[0, 5, mdist.OROW_SPEC])
    cases = [(1, 2, spec ^ (mdist.OSPEC_PART_DESC << 24)), (1, 0, spec ^ (1 << 4)), (1, 1, sort_spec), (1, 2, 0), (2, 1, spec), (5, 0, spec), (4, 2, int(good_in[0, 4, mdist.OROW_SPEC]) ^ (mdist.OSPEC_PART_DESC << 8))]
    dev_in = hip.malloc(3 * nq * m.OROW_WORDS * 8)
    for qi, which, other in cases:
        rows = good_in.copy()
        rows[which, qi, mdist.OROW_SPEC] = other
        hip.to_dev(dev_in, rows)
        got = merge(m, ctx, hip, dev_in, 3, nq)
        assert int(got[qi, K1 + 1]) == int(good[qi, K1 + 1]) | mdist.ROW_DECLINED and int(got[qi, K1]) == 0, (qi, which, hex(other))
        assert not got[qi, :K1].any() and not got[qi, mdist.OROW_MKEYS:mdist.OROW_SPEC].any()
        others = [i for i in range(nq) if i != qi]
        assert np.array_equal(got[others], good[others])  # the batch's other queries are untouched
        assert np.array_equal(mdist.merge_orows_np(rows, 1024), got)
    hip.free()


def test_overflowed_shard_is_rerun_and_merged_exactly(dev):
    """One shard of 3 M docs ordered by (bool, a constant second column) -- half of ~2.4 M matches share the best 64-bit key, the
    candidate list overflows -- plus one small shard, with a standing order-row destination: the big shard's row leaves with
    MRK_ROW_RERUN; after mrk_batch_wait + mrk_batch_export_orows the repaired row holds its mapped keys and the merge equals the
    unsharded result."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    n_big, n_small = 3_000_000, 50_001
    n_docs, cuts = n_big + n_small, [0, n_big, n_big + n_small]
    c = smc.Corpus(m, make_rows, n_docs, cuts, [0.8, 0.3], seed=5, rows_seed=21, max_pos=16)
    o, cnt, kind = part_specs(m)["bool"]
    qs = [c.globalize(m.Query(kw(m, 0, 1), ranker=m.SPH_RANK_BM25, max_matches=1000, order=m.Order([m.OrderPart(o, cnt, desc=True, kind=kind), m.OrderPart(CONST * 32, 32, desc=False)], then_weight=1))),
          c.globalize(m.Query(m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2)), ranker=m.SPH_RANK_BM25, max_matches=1000))]
    nq, RW = len(qs), m.OROW_WORDS
    want = unsharded(m, ctx, batch, c, qs)
    assert want[0].total_found > 2 * 2 ** 20 and want[0].status == 0
    orows_all = hip.malloc(2 * nq * RW * 8)
    hip.fill(orows_all, 0xEE, 2 * nq * RW * 8)
    b2 = m.Batch(ctx, nq)
    for s in range(2):
        seg = m.Segment(ctx, c.shards[s], rowid_base=cuts[s])
        try:
            seg.set_attrs(c.shard_rows[s])
            chk(lib.mrk_batch_set_orows_dst(b2._h, off(orows_all, s * nq * RW * 8)))
            b2.submit(seg, qs)
            b2.wait()
            n_rerun = b2.stats()["n_rerun"]
            row = hip.to_host(off(orows_all, s * nq * RW * 8), (nq, RW))
            if s == 0:
                assert n_rerun >= 1  # the overflow must happen, else this test shows nothing
                assert int(row[0, K1 + 1]) == mdist.ROW_RERUN and int(row[0, K1]) == 0 and not row[0, :K1].any() and not row[0, K1 + 2:mdist.OROW_SPEC].any()
                first = merge(m, ctx, hip, orows_all, 1, nq)
                assert int(first[0, K1 + 1]) & mdist.ROW_RERUN
                b2.export_orows(orows_all.value)  # the rerun's result, mapped keys included
                row = hip.to_host(orows_all, (nq, RW))
                assert int(row[0, K1]) == 1000 and not int(row[0, K1 + 1]) & mdist.ROW_RERUN
                g = b2.results()[0]
                assert np.array_equal(mdist.unmap_order_keys(int(row[0, mdist.OROW_SPEC]), mdist.orow_mkeys(row[0])[:1000]), g.order_key) and g.order_key.all()
            else:
                assert n_rerun == 0
            assert not int(row[1, K1 + 1]) & (mdist.ROW_RERUN | mdist.ROW_DECLINED)
        finally:
            seg.close()
    chk(lib.mrk_batch_set_orows_dst(b2._h, None))
    b2.close()
    host = merge(m, ctx, hip, orows_all, 2, nq)
    assert_equals_unsharded(mdist, qs, want, host, "rerun")
    hip.free()


@pytest.mark.parametrize("mode", ["lib-comm", "torch"])
def test_ordered_exchange_chain_one_rank(mode):
    """ShardMerger(order_rows=True) with one rank, through the library's communicator and through torch.distributed."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(here, "dist_order_chain_worker.py")] + (["--lib-comm"] if mode == "lib-comm" else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ordered dist chain ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
