"""GPU: queries ordered by a row attribute (Query.sort: ORDER BY attr [, weight()]) against the oracle.  The oracle ranks with any
max_matches, so the expected answer is its result for the same query with max_matches = number of docs (every match with its
weight), ordered on the host by numpy -- lexsort over (attribute as numpy reads it, weight per the tie rule, rowid) -- cut to K
(sorted_expect.expected_sort, itself pinned on the reference's recorded results by test_sorted_golden_cpu.py).
The attribute key is computed by numpy from the raw rows (unsigned compare for integers, float32 compare for floats), not by the
library's map.  Every comparison is exact."""
import dataclasses
import os
import threading

import numpy as np
import pytest

from helpers import synth_postings
from sorted_expect import expected_sort as expected  # (shared with test_gpu_order.py and the recorded-result tests)
from test_gpu_parity import kw, orc_index_of, to_orc

pytestmark = pytest.mark.gpu

TS, BITS, FLT, AUX = 0, 1, 2, 3  # dwords of a row
STRIDE = 4


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    yield m, ctx, batch
    batch.close()
    ctx.close()


def make_rows(rng, n_docs):
    """[TS] timestamps in a narrow band of the 32-bit range; [BITS] a 5-bit field at bit 3, a 4-valued category at bits 10..11,
    a bool at bit 31, noise elsewhere; [FLT] floats with negatives, both zeros, denormals and infinities; [AUX] rowid % 10."""
    rows = np.zeros((n_docs, STRIDE), np.uint32)
    rows[:, TS] = np.uint32(1_700_000_000) + rng.integers(0, 5_000_000, n_docs).astype(np.uint32)
    rows[:, BITS] = rng.integers(0, 1 << 32, n_docs, dtype=np.uint64).astype(np.uint32)
    f = (rng.standard_normal(n_docs) * 100).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, np.inf, -np.inf, 3.4e38, -3.4e38, 1.0, -1.0], np.float32)
    pick = rng.random(n_docs) < 0.3
    f[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    rows[:, FLT] = f.view(np.uint32)
    rows[:, AUX] = np.arange(n_docs, dtype=np.uint32) % 10
    return rows


def sorts(m):
    return {"ts": (TS * 32, 32, m.SORTKEY_INT), "bits5": (BITS * 32 + 3, 5, m.SORTKEY_INT), "bool": (BITS * 32 + 31, 1, m.SORTKEY_INT),
            "cat": (BITS * 32 + 10, 2, m.SORTKEY_INT), "float": (FLT * 32, 32, m.SORTKEY_FLOAT)}


def check(orc, oi, rows, n_docs, queries, got, what=""):
    for i, (q, g) in enumerate(zip(queries, got)):
        assert g.status == 0, (what, i, q.sort, "no query of this test may be declined")
        if q.sort is None:
            want = to_orc(orc, q).run(oi)
            assert g.total_found == want.total_found and np.array_equal(g.rowid, want.rowid) and np.array_equal(g.weight, want.weight), (what, i)
            assert g.sort_key is None
            continue
        r, w, k, total = expected(orc, oi, q, rows, n_docs)
        assert g.total_found == total, (what, i, g.total_found, total)
        assert len(g.rowid) == len(r), (what, i, len(g.rowid), len(r))
        assert np.array_equal(g.rowid, r), (what, i, q.sort, q.ranker, q.max_matches, g.rowid[:8], r[:8])
        assert np.array_equal(g.weight, w), (what, i, g.weight[:8], w[:8])
        assert np.array_equal(g.sort_key, k), (what, i, g.sort_key[:8], k[:8])


def random_queries(m, rng, nt, n):
    S = sorts(m)
    rankers = [m.SPH_RANK_NONE, m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_SPH04]
    qs = []
    for i in range(n):
        shape = i % 6
        ts = [int(t) for t in rng.permutation(nt)]
        if shape == 0:
            root = kw(m, ts[0], 1)
        elif shape == 1:
            k = int(rng.integers(2, 9))
            root = m.XQNode.AND(*[kw(m, ts[j % nt], j + 1) for j in range(k)]) if k <= nt else m.XQNode.AND(*[kw(m, ts[j], j + 1) for j in range(nt)])
        elif shape == 2:  # boolean tree
            root = m.XQNode.AND(m.XQNode(m.SPH_QUERY_OR, [kw(m, ts[0], 1), kw(m, ts[1], 2)]), m.XQNode(m.SPH_QUERY_ANDNOT, [kw(m, ts[2], 3), kw(m, ts[3], 4)]))
        elif shape == 3:
            root = m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, ts[0], 1), kw(m, ts[1], 2)])
        elif shape == 4:  # five keywords under a hit ranker: the generic evaluator
            root = m.XQNode.AND(*[kw(m, ts[j], j + 1) for j in range(5)])
        else:
            root = m.XQNode.AND(kw(m, ts[0], 1), kw(m, ts[1], 2))
        ranker = rankers[int(rng.integers(0, 4))] if shape != 4 else [m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_SPH04][int(rng.integers(0, 2))]
        name = list(S)[int(rng.integers(0, len(S)))]
        off, cnt, kind = S[name]
        q = m.Query(root, ranker=ranker, max_matches=int(rng.choice([1, 10, 1000, 1024])), index_weight=int(rng.choice([1, 1, 3])),
                    sort=m.Sort(off, cnt, desc=bool(rng.integers(0, 2)), then_weight=int(rng.integers(0, 3)), kind=kind))
        if rng.random() < 0.25:
            q.filters = [m.Filter(AUX * 32, 32, values=[1, 3, 5, 7, 8])]
        if rng.random() < 0.2 and ranker != m.SPH_RANK_NONE:
            q.weight_filters = [m.Filter(0, 0, min=1500, max=1 << 30)]
        qs.append(q)
    return qs


@pytest.mark.parametrize("n_fields", [4, 17])
def test_sorted_queries_vs_oracle(orc, dev, n_fields):
    m, ctx, batch = dev
    rng = np.random.default_rng(int(os.environ.get("MRK_FUZZ_SEED", 20260611)) + n_fields)
    for trial in range(int(os.environ.get("MRK_FUZZ_TRIALS", 4))):
        n_docs = int(rng.choice([700, 5000, 30000]))
        assert n_docs < 2 ** 20  # below the candidate list's 2^20 slots nothing overflows: a decline would be a bug, not a limit
        nt = 8
        probs = [float(rng.choice([0.9, 0.6, 0.4, 0.2])) for _ in range(nt)]
        W, R, H = synth_postings(rng, n_docs, probs, n_fields=n_fields, max_pos=int(rng.choice([6, 14])))
        hi = m.index_from_hits(W, R, H, n_terms=nt, total_docs=n_docs, skiplist_block_size=int(rng.choice([32, 128])), hit_format=int(rng.integers(0, 2)),
                               n_fields=n_fields)
        rows = make_rows(rng, n_docs)
        seg = m.Segment(ctx, hi)
        oi = orc_index_of(orc, hi)
        oi.attrs = rows
        try:
            seg.set_attrs(rows)
            qs = random_queries(m, rng, nt, 48)
            check(orc, oi, rows, n_docs, qs, batch.search(seg, qs), f"fields {n_fields} trial {trial}")
            assert batch.stats()["packed"] == 1
            if trial % 2 == 1:  # the same with a dead-row map
                dead = np.zeros((n_docs + 31) // 32, np.uint32)
                killed = rng.choice(n_docs, n_docs // 7, replace=False).astype(np.uint32)
                np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
                seg.set_dead_rows(dead)
                oi.dead_rows = dead
                check(orc, oi, rows, n_docs, qs, batch.search(seg, qs), f"fields {n_fields} trial {trial} dead rows")
        finally:
            seg.close()


def test_low_cardinality_column_is_exact(orc, dev):
    """A 4-valued category under BM25: a quarter of the matches share the K-th row's key; all of them are ordered by weight and rowid."""
    m, ctx, batch = dev
    n_docs = 400_000
    assert n_docs <= 500_000 and n_docs < 2 ** 20
    hi = m.synth_index(n_docs, [0.5, 0.4, 0.1], seed=11, skiplist_block_size=128, max_pos=16)
    rng = np.random.default_rng(5)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    oi.attrs = rows
    try:
        seg.set_attrs(rows)
        off, cnt, kind = sorts(m)["cat"]
        qs = [m.Query(m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2)), ranker=rk, max_matches=K, sort=m.Sort(off, cnt, desc=d, then_weight=t, kind=kind))
              for rk in (m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25) for K, d, t in ((1000, True, 1), (1024, False, 2), (10, True, 0))]
        qs.append(m.Query(kw(m, 0, 1), ranker=m.SPH_RANK_BM25, max_matches=1000, sort=m.Sort(BITS * 32 + 31, 1, desc=True, then_weight=1)))
        check(orc, oi, rows, n_docs, qs, batch.search(seg, qs), "category")
    finally:
        seg.close()


def test_three_million_docs_prunes_on_the_attribute(orc, dev):
    m, ctx, batch = dev
    n_docs = 3_000_000
    hi = m.synth_index(n_docs, [0.3, 0.2], seed=3, skiplist_block_size=128, max_pos=16)
    rng = np.random.default_rng(9)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    try:
        seg.set_attrs(rows)
        q = m.Query(m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2)), ranker=m.SPH_RANK_BM25, max_matches=1000, sort=m.Sort(TS * 32, 32, desc=True, then_weight=1))
        got = batch.search(seg, [q])
        st = batch.stats()
        print(f"3M docs ORDER BY ts DESC: total_found {got[0].total_found}, n_cands {st['n_cands']}, n_rerun {st['n_rerun']}")
        check(orc, oi, rows, n_docs, [q], got, "3M")
        if got[0].total_found >= 65536:
            assert st["n_cands"] < got[0].total_found  # pruning on the attribute is alive
    finally:
        seg.close()


def test_overflowing_candidate_list_is_rerun_exactly(orc, dev):
    """Exact or loud: a keyword in ~80 % of 3 M docs ordered by a bool column puts ~1.2 M rows on the K-th row's key, more than the
    2^20 slots of the candidate list: the query is rerun alone with a list for every driver doc and must come back exact."""
    m, ctx, batch = dev
    n_docs = 3_000_000
    hi = m.synth_index(n_docs, [0.8, 0.3], seed=5, skiplist_block_size=128, max_pos=16)
    rng = np.random.default_rng(21)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    try:
        seg.set_attrs(rows)
        off, cnt, kind = sorts(m)["bool"]
        for ranker in (m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25):
            # a single keyword, and a hit-ranked OR that matches ~86 % of the docs
            root = kw(m, 0, 1) if ranker == m.SPH_RANK_BM25 else m.XQNode(m.SPH_QUERY_OR, [kw(m, 0, 1), kw(m, 1, 2)])
            q = m.Query(root, ranker=ranker, max_matches=1000, sort=m.Sort(off, cnt, desc=True, then_weight=1, kind=kind))
            got = batch.search(seg, [q])
            st = batch.stats()
            print(f"overflow case ranker {ranker}: total_found {got[0].total_found}, n_cands {st['n_cands']}, n_rerun {st['n_rerun']}")
            assert got[0].total_found > 2 * 2 ** 20  # half of them share the best key: the list of 2^20 cannot hold them
            assert st["n_rerun"] == 1 and got[0].status == 0
            check(orc, oi, rows, n_docs, [q], got, f"overflow ranker {ranker}")
    finally:
        seg.close()


def test_batch_state_and_mixed_batches(orc, dev):
    m, ctx, batch = dev
    rng = np.random.default_rng(77)
    n_docs, nt = 20000, 6
    W, R, H = synth_postings(rng, n_docs, [0.7, 0.5, 0.4, 0.3, 0.2, 0.1], n_fields=3, max_pos=10)
    hi = m.index_from_hits(W, R, H, n_terms=nt, total_docs=n_docs, n_fields=3)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    oi.attrs = rows
    try:
        seg.set_attrs(rows)
        S = random_queries(m, rng, nt, 18)
        rel = [dataclasses.replace(q, sort=None) for q in random_queries(m, rng, nt, 12)]
        mixed = [q for pair in zip(S, rel + rel) for q in pair][: len(S) + len(rel)]
        only_rel = batch.search(seg, rel)
        first = batch.search(seg, mixed)
        second = batch.search(seg, mixed)  # the same batch again: state carried between submits
        check(orc, oi, rows, n_docs, mixed, first, "mixed")
        for a, b in zip(first, second):
            assert a.total_found == b.total_found and np.array_equal(a.rowid, b.rowid) and np.array_equal(a.weight, b.weight)
            assert (a.sort_key is None) == (b.sort_key is None) and (a.sort_key is None or np.array_equal(a.sort_key, b.sort_key))
        again_rel = batch.search(seg, rel)  # the second candidate plane gone again
        for a, b in zip(only_rel, again_rel):
            assert a.total_found == b.total_found and np.array_equal(a.rowid, b.rowid) and np.array_equal(a.weight, b.weight)
        got_rel = [g for q, g in zip(mixed, first) if q.sort is None]
        want_rel = batch.search(seg, [q for q in mixed if q.sort is None])
        for a, b in zip(got_rel, want_rel):
            assert a.total_found == b.total_found and np.array_equal(a.rowid, b.rowid) and np.array_equal(a.weight, b.weight)
        for q, g in zip(mixed, first):  # the sorted ones equal their solo results
            if q.sort is not None:
                solo = batch.search(seg, [q])[0]
                assert solo.total_found == g.total_found and np.array_equal(solo.rowid, g.rowid) and np.array_equal(solo.weight, g.weight) and np.array_equal(solo.sort_key, g.sort_key)
        # Batcher.search from 4 threads equals the direct result
        bt = m.Batcher(ctx, max_batch=16)
        out = {}

        def work(t):
            out[t] = [bt.search(seg, q) for q in S[t::4]]

        th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        [t.start() for t in th]
        [t.join() for t in th]
        bt.close()
        direct = batch.search(seg, S)
        for t in range(4):
            for g, d in zip(out[t], direct[t::4]):
                assert g.status == 0 and g.total_found == d.total_found and np.array_equal(g.rowid, d.rowid) and np.array_equal(g.weight, d.weight) and np.array_equal(g.sort_key, d.sort_key)
    finally:
        seg.close()


def test_declines_are_per_query(orc, dev):
    m, ctx, batch = dev
    rng = np.random.default_rng(3)
    n_docs = 4000
    W, R, H = synth_postings(rng, n_docs, [0.6, 0.4], n_fields=3, max_pos=8)
    hi = m.index_from_hits(W, R, H, n_terms=2, total_docs=n_docs, n_fields=3)
    rows = make_rows(rng, n_docs)
    nan_rows = rows.copy()
    nan_rows[17, FLT] = 0x7FC00000
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    oi.attrs = rows
    root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
    good = m.Query(root, ranker=m.SPH_RANK_BM25, sort=m.Sort(TS * 32, 32))
    plain = m.Query(root, ranker=m.SPH_RANK_BM25)
    try:
        got = batch.search(seg, [plain, good])  # no attribute rows yet
        assert got[0].status == 0 and got[1].status == -2  # MRK_E_UNSUPPORTED
        seg.set_attrs(nan_rows)
        fl = m.Query(root, ranker=m.SPH_RANK_BM25, sort=m.Sort(FLT * 32, 32, kind=m.SORTKEY_FLOAT))
        qs = [plain, dataclasses.replace(good, cutoff=50), good, m.Query(root, ranker=m.SPH_RANK_BM25, sort=m.Sort(TS * 32, 64)), fl]
        got = batch.search(seg, qs)
        assert [g.status for g in got] == [0, -2, 0, -2, -2]
        check(orc, oi, rows, n_docs, [plain, good], [got[0], got[2]], "next to declined ones")
        seg.set_attrs(rows)  # new rows: the cached column range (and its NaN) is dropped
        got = batch.search(seg, [fl])
        check(orc, oi, rows, n_docs, [fl], got, "after set_attrs")
    finally:
        seg.close()
