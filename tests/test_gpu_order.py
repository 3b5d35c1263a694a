"""GPU: queries ordered by a 64-bit attribute or by two attributes (Query.order: ORDER BY big | ORDER BY a, b [, weight()]) against
the oracle.  As in test_gpu_sort.py the expected answer is the oracle's result for the same query with max_matches = number of docs
(every match with its weight), ordered on the host by numpy -- lexsort over (first part, second part, weight per the tie rule,
rowid) with the parts as numpy reads the raw rows (int64 view for a 64-bit attribute, float32 compare for floats, unsigned for
integers) -- and cut to K (sorted_expect.expected_order).  Every comparison is exact: rowids, weights, order_key and total_found."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

from helpers import synth_postings
from sorted_expect import expected_order as expected  # (shared with test_gpu_sort.py and the recorded-result tests)
from sorted_expect import part_key, raw_of  # noqa: F401
from test_gpu_parity import kw, orc_index_of, to_orc
from test_gpu_sort import AUX, BITS, FLT, TS
from test_gpu_sort import check as check_sort
from test_gpu_sort import make_rows as make_rows4
from test_gpu_sort import random_queries as random_sort_queries
from test_gpu_sort import sorts

pytestmark = pytest.mark.gpu

# dwords of a row behind test_gpu_sort's four: 64-bit attributes (low dword first), then a constant
BIG, BIGHI, BIGLO, ID, CONST = 4, 6, 8, 10, 12
STRIDE = 13
BIGS = {"big": BIG, "bighi": BIGHI, "biglo": BIGLO, "id": ID}


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    yield m, ctx, batch
    batch.close()
    ctx.close()


def make_rows(rng, n_docs, const_second=False):
    """test_gpu_sort's columns, then [BIG] a bigint of both signs with few distinct high dwords (so that both dwords decide),
    [BIGHI] one whose low dword is 0, [BIGLO] one whose high dword is 0, [ID] a unique ascending id beyond 32 bits, [CONST] 42."""
    rows = np.zeros((n_docs, STRIDE), np.uint32)
    rows[:, :4] = make_rows4(rng, n_docs)
    big = (rng.integers(-3, 4, n_docs).astype(np.int64) << 32) + rng.integers(0, 1 << 32, n_docs, dtype=np.uint64).astype(np.int64)
    edge = rng.random(n_docs) < 0.02
    big[edge] = rng.choice(np.array([np.iinfo(np.int64).min, -1, 0, 1, np.iinfo(np.int64).max], np.int64), int(edge.sum()))
    rows[:, BIG:BIG + 2] = big.view(np.uint32).reshape(n_docs, 2)
    rows[:, BIGHI + 1] = rng.integers(-5, 6, n_docs).astype(np.int32).view(np.uint32)
    rows[:, BIGLO] = rng.integers(0, 1 << 32, n_docs, dtype=np.uint64).astype(np.uint32)
    ids = np.int64(10_000_000_000) + np.arange(n_docs, dtype=np.int64) * 7
    rows[:, ID:ID + 2] = ids.view(np.uint32).reshape(n_docs, 2)
    rows[:, CONST] = 42
    if const_second:
        rows[:, TS] = 1_700_000_000
    return rows


def part_specs(m):
    return sorts(m)  # name -> (bit_offset, bit_count, kind): ts, bits5, bool, cat, float


def check(orc, oi, rows, n_docs, queries, got, what=""):
    for i, (q, g) in enumerate(zip(queries, got)):
        assert g.status == 0, (what, i, q.order, q.sort, "no query of this test may be declined")
        if q.order is None:
            check_sort(orc, oi, rows, n_docs, [q], [g], what)
            assert g.order_key is None
            continue
        r, w, k, total = expected(orc, oi, q, rows, n_docs)
        assert g.total_found == total, (what, i, g.total_found, total)
        assert len(g.rowid) == len(r), (what, i, len(g.rowid), len(r))
        assert np.array_equal(g.rowid, r), (what, i, q.order, q.ranker, q.max_matches, g.rowid[:8], r[:8])
        assert np.array_equal(g.weight, w), (what, i, q.order, g.weight[:8], w[:8])
        assert g.sort_key is None and g.order_key is not None and g.order_key.dtype == np.uint64
        assert np.array_equal(g.order_key, k), (what, i, q.order, g.order_key[:8], k[:8])


def random_order(m, rng):
    P = part_specs(m)
    tie = int(rng.integers(0, 3))
    if rng.random() < 0.4:
        name = list(BIGS)[int(rng.integers(0, len(BIGS)))]
        return m.Order([m.OrderPart(BIGS[name] * 32, 64, desc=bool(rng.integers(0, 2)), kind=m.SORTKEY_INT64)], then_weight=tie)
    a, b = rng.choice(len(P), 2, replace=False)
    parts = [m.OrderPart(P[n][0], P[n][1], desc=bool(rng.integers(0, 2)), kind=P[n][2]) for n in (list(P)[int(a)], list(P)[int(b)])]
    return m.Order(parts, then_weight=tie)


def random_queries(m, rng, nt, n):
    """test_gpu_sort's query shapes, rankers, filters and K, each under a random order"""
    qs = random_sort_queries(m, rng, nt, n)
    return [dataclasses.replace(q, sort=None, order=random_order(m, rng)) for q in qs]


def all_orders(m):
    """every bigint column in both directions and every ordered pair of the five <= 32-bit columns"""
    P = part_specs(m)
    out = [m.Order([m.OrderPart(it * 32, 64, desc=d, kind=m.SORTKEY_INT64)], then_weight=1) for it in BIGS.values() for d in (True, False)]
    for i, a in enumerate(P):
        for j, b in enumerate(P):
            if a != b:
                out.append(m.Order([m.OrderPart(P[a][0], P[a][1], desc=(i + j) % 2 == 0, kind=P[a][2]), m.OrderPart(P[b][0], P[b][1], desc=j % 2 == 0, kind=P[b][2])],
                                   then_weight=(i + j) % 3))
    return out


@pytest.mark.parametrize("n_fields", [4, 17])
def test_ordered_queries_vs_oracle(orc, dev, n_fields):
    m, ctx, batch = dev
    rng = np.random.default_rng(int(os.environ.get("MRK_FUZZ_SEED", 20261016)) + n_fields)
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
            if trial == 0:  # every column and every pair at least once, under a plain AND
                root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
                qs += [m.Query(root, ranker=[m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25][i % 2], max_matches=[10, 1000][i % 2], order=o) for i, o in enumerate(all_orders(m))]
            got = []
            for at in range(0, len(qs), 64):
                got += batch.search(seg, qs[at:at + 64])
                assert batch.stats()["packed"] == 1 and batch.stats()["n_rerun"] == 0
            check(orc, oi, rows, n_docs, qs, got, f"fields {n_fields} trial {trial}")
            if trial % 2 == 1:  # the same with a dead-row map
                dead = np.zeros((n_docs + 31) // 32, np.uint32)
                killed = rng.choice(n_docs, n_docs // 7, replace=False).astype(np.uint32)
                np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
                seg.set_dead_rows(dead)
                oi.dead_rows = dead
                check(orc, oi, rows, n_docs, qs[:48], batch.search(seg, qs[:48]), f"fields {n_fields} trial {trial} dead rows")
        finally:
            seg.close()


def same(a, b):
    return a.status == b.status == 0 and a.total_found == b.total_found and np.array_equal(a.rowid, b.rowid) and np.array_equal(a.weight, b.weight)


def test_one_part_through_order_equals_sort_and_mixed_batches(orc, dev):
    """One part of <= 32 bits through Query.order answers bit for bit as the same Sort; relevance and Sort queries next to Order
    queries answer exactly as in a batch without them, and the Order queries as alone."""
    m, ctx, batch = dev
    rng = np.random.default_rng(78)
    n_docs, nt = 20000, 6
    W, R, H = synth_postings(rng, n_docs, [0.7, 0.5, 0.4, 0.3, 0.2, 0.1], n_fields=3, max_pos=10)
    hi = m.index_from_hits(W, R, H, n_terms=nt, total_docs=n_docs, n_fields=3)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    oi.attrs = rows
    try:
        seg.set_attrs(rows)
        S = random_sort_queries(m, rng, nt, 24)
        via_order = [dataclasses.replace(q, sort=None, order=m.Order([m.OrderPart(q.sort.bit_offset, q.sort.bit_count, desc=q.sort.desc, kind=q.sort.kind)],
                                                                     then_weight=q.sort.then_weight)) for q in S]
        a, b = batch.search(seg, S), batch.search(seg, via_order)
        for q, x, y in zip(S, a, b):
            assert same(x, y), q.sort
            assert y.sort_key is None and np.array_equal(y.order_key, x.sort_key.astype(np.uint64) << np.uint64(32))
        check(orc, oi, rows, n_docs, via_order, b, "one part")
        # mixed: relevance | sort | order
        O = random_queries(m, rng, nt, 18)
        rel = [dataclasses.replace(q, sort=None) for q in random_sort_queries(m, rng, nt, 12)]
        others = rel + S[:12]
        mixed = [q for trio in zip(O, others, others[6:] + others[:6]) for q in trio]
        only_others = batch.search(seg, others)
        first = batch.search(seg, mixed)
        second = batch.search(seg, mixed)  # the same batch again: state carried between submits
        assert batch.stats()["n_rerun"] == 0
        check(orc, oi, rows, n_docs, mixed, first, "mixed")
        for x, y in zip(first, second):
            assert same(x, y) and (x.order_key is None) == (y.order_key is None) and (x.order_key is None or np.array_equal(x.order_key, y.order_key))
        solo = {id(q): g for q, g in zip(others, only_others)}
        for q, g in zip(mixed, first):
            if q.order is None:  # as in the batch without the order queries
                w = solo[id(q)]
                assert same(g, w) and (g.sort_key is None) == (w.sort_key is None) and (g.sort_key is None or np.array_equal(g.sort_key, w.sort_key))
            else:
                w = batch.search(seg, [q])[0]
                assert same(g, w) and np.array_equal(g.order_key, w.order_key)
        again = batch.search(seg, others)  # and once more without them
        for x, y in zip(only_others, again):
            assert same(x, y)
        # the batching front takes such a query like any other (no order_key, as it hands out no sort_key)
        bt = m.Batcher(ctx, max_batch=8)
        try:
            for q in O[:6]:
                g, w = bt.search(seg, q), batch.search(seg, [q])[0]
                assert same(g, w) and g.order_key is None
        finally:
            bt.close()
    finally:
        seg.close()


def test_three_million_docs_prune_past_a_constant_first_key(orc, dev):
    """A first column that is CONSTANT, a timestamp second: bins over the first part alone would put every match into the threshold
    bin (n_cands == total_found); the compressed bin must prune on the second part.  Exact, no rerun, n_cands < total_found."""
    m, ctx, batch = dev
    n_docs = 3_000_000
    hi = m.synth_index(n_docs, [0.3, 0.2], seed=3, skiplist_block_size=128, max_pos=16)
    rng = np.random.default_rng(9)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    measured = {}
    try:
        seg.set_attrs(rows)
        for ranker, name in ((m.SPH_RANK_BM25, "bm25"), (m.SPH_RANK_PROXIMITY_BM25, "proximity_bm25")):
            q = m.Query(m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2)), ranker=ranker, max_matches=1000,
                        order=m.Order([m.OrderPart(CONST * 32, 32, desc=True), m.OrderPart(TS * 32, 32, desc=True)], then_weight=1))
            got = batch.search(seg, [q])
            st = batch.stats()
            measured[name] = {"total_found": int(got[0].total_found), "n_cands": int(st["n_cands"]), "n_rerun": int(st["n_rerun"])}
            print(f"3M docs ORDER BY const DESC, ts DESC ({name}): {json.dumps(measured[name])}")
            check(orc, oi, rows, n_docs, [q], got, f"3M {name}")
            assert st["n_rerun"] == 0
            assert got[0].total_found >= 65536 and st["n_cands"] < got[0].total_found  # pruning past the first key is alive
        out = os.environ.get("MRK_ORDER_PRUNE_JSON")
        if out:
            with open(out, "w") as f:
                json.dump({"n_docs": n_docs, "order": "const DESC, ts DESC, weight() DESC", "k": 1000, "query": "2-way AND, keyword probabilities 0.3 / 0.2", **measured}, f, indent=1)
    finally:
        seg.close()


def test_overflowing_candidate_list_is_rerun_exactly(orc, dev):
    """Exact or loud: ~80 % of 3 M docs ordered by (bool, a constant second column): half of the > 2^20 matches share the best 64-bit
    key, more than the candidate list's 2^20 slots hold: the query is rerun alone and must come back exact."""
    m, ctx, batch = dev
    n_docs = 3_000_000
    hi = m.synth_index(n_docs, [0.8, 0.3], seed=5, skiplist_block_size=128, max_pos=16)
    rng = np.random.default_rng(21)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    try:
        seg.set_attrs(rows)
        off, cnt, kind = part_specs(m)["bool"]
        for ranker in (m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25):
            root = kw(m, 0, 1) if ranker == m.SPH_RANK_BM25 else m.XQNode(m.SPH_QUERY_OR, [kw(m, 0, 1), kw(m, 1, 2)])
            q = m.Query(root, ranker=ranker, max_matches=1000, order=m.Order([m.OrderPart(off, cnt, desc=True, kind=kind), m.OrderPart(CONST * 32, 32, desc=False)], then_weight=1))
            got = batch.search(seg, [q])
            st = batch.stats()
            print(f"overflow case ranker {ranker}: total_found {got[0].total_found}, n_cands {st['n_cands']}, n_rerun {st['n_rerun']}")
            assert got[0].total_found > 2 * 2 ** 20  # half of them share the best key: the list of 2^20 cannot hold them
            assert st["n_rerun"] == 1 and got[0].status == 0
            check(orc, oi, rows, n_docs, [q], got, f"overflow ranker {ranker}")
    finally:
        seg.close()


class Hip:
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.bufs = []

    def malloc(self, n):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(n, 8))) == 0
        self.bufs.append(p)
        return p

    def to_host(self, p, shape):
        a = np.zeros(shape, np.uint64)
        assert self.hip.hipMemcpy(C.c_void_p(a.ctypes.data), p, C.c_size_t(a.nbytes), 2) == 0
        return a

    def fill(self, p, byte, n):
        assert self.hip.hipMemset(p, byte, C.c_size_t(n)) == 0

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(p)
        self.bufs = []


def test_exchange_rows_decline_a_64_bit_key(dev):
    """A key of more than 32 bits fits no exchange row: an Order query leaves in narrow and in wide rows, exported and through a
    standing wide destination, with MRK_ROW_DECLINED, zero count and zero keys; the relevance and Sort queries' rows equal those of
    the batch without the Order queries, word for word."""
    m, ctx, batch = dev
    from manticoresearch_amd import _lib
    from manticoresearch_amd import dist as mdist

    lib, chk = _lib.lib(), _lib.check
    K1 = _lib.MRK_MAX_K
    rng = np.random.default_rng(31)
    n_docs, nt = 20000, 6
    W, R, H = synth_postings(rng, n_docs, [0.7, 0.5, 0.4, 0.3, 0.2, 0.1], n_fields=3, max_pos=10)
    hi = m.index_from_hits(W, R, H, n_terms=nt, total_docs=n_docs, n_fields=3)
    rows = make_rows(rng, n_docs)
    seg = m.Segment(ctx, hi)
    hip = Hip()
    b2 = m.Batch(ctx, 64)
    try:
        seg.set_attrs(rows)
        S = random_sort_queries(m, rng, nt, 8)
        rel = [dataclasses.replace(q, sort=None) for q in random_sort_queries(m, rng, nt, 8)]
        O = random_queries(m, rng, nt, 8)
        O[0] = dataclasses.replace(O[0], order=m.Order([m.OrderPart(BIG * 32, 64, kind=m.SORTKEY_INT64)]))
        O[1] = dataclasses.replace(O[1], order=m.Order([m.OrderPart(BITS * 32 + 31, 1), m.OrderPart(TS * 32, 32, desc=False)], then_weight=0))
        O[2] = dataclasses.replace(O[2], order=m.Order([m.OrderPart(TS * 32, 32)]))  # one part of <= 32 bits travels as the same Sort does
        others = [q for pair in zip(rel, S) for q in pair]
        mixed, is_wide = [], []
        for i, q in enumerate(others):
            mixed.append(q), is_wide.append(False)
            if i % 2 == 0:
                mixed.append(O[i // 2]), is_wide.append(i // 2 != 2)
        n_o, n_m = len(others), len(mixed)
        narrow, wide, standing = hip.malloc(n_m * m.ROW_WORDS * 8), hip.malloc(n_m * m.SROW_WORDS * 8), hip.malloc(n_m * m.SROW_WORDS * 8)

        def rows_of(qs, wide_dst=None):
            n = len(qs)
            if wide_dst is not None:
                hip.fill(wide_dst, 0xEE, n * m.SROW_WORDS * 8)
                chk(lib.mrk_batch_set_srows_dst(b2._h, wide_dst))
            b2.submit(seg, qs)
            b2.wait()
            st = [g.status for g in b2.results()]
            assert st == [0] * n and b2.stats()["n_rerun"] == 0
            if wide_dst is not None:
                chk(lib.mrk_batch_set_srows_dst(b2._h, None))
                return None, hip.to_host(wide_dst, (n, m.SROW_WORDS))
            chk(lib.mrk_batch_export_rows(b2._h, narrow))
            b2.export_srows(wide.value)
            return hip.to_host(narrow, (n, m.ROW_WORDS)), hip.to_host(wide, (n, m.SROW_WORDS))

        base_n, base_w = rows_of(others)
        got_n, got_w = rows_of(mixed)
        _, got_s = rows_of(mixed, standing)
        _, base_s = rows_of(others, standing)
        assert np.array_equal(base_s, base_w)  # (a standing wide destination writes what the export writes)
        keep = [i for i, w in enumerate(is_wide) if not w and mixed[i].order is None]
        assert len(keep) == n_o
        for got, base, what in ((got_n, base_n, "narrow"), (got_w, base_w, "wide"), (got_s, base_s, "standing wide")):
            assert np.array_equal(got[keep], base), what
            for i, w in enumerate(is_wide):
                if w:
                    assert int(got[i, K1 + 1]) == mdist.ROW_DECLINED and int(got[i, K1]) == 0 and not got[i, :K1].any(), (what, i)
                    assert not got[i, K1 + 2:].any(), (what, i)  # (wide rows: no mapped keys, spec word 0)
        # the one-part order's wide row is the row of the same Sort
        i2 = [i for i, q in enumerate(mixed) if q.order is not None and not is_wide[i]]
        assert len(i2) == 1
        _, as_sort = rows_of([dataclasses.replace(mixed[i2[0]], order=None, sort=m.Sort(TS * 32, 32))])
        assert np.array_equal(got_w[i2[0]], as_sort[0]) and np.array_equal(got_s[i2[0]], as_sort[0])
        assert not int(got_w[i2[0], K1 + 1]) & mdist.ROW_DECLINED
    finally:
        hip.free()
        b2.close()
        seg.close()


def test_declines_are_per_query_and_loud(dev):
    m, ctx, batch = dev
    from manticoresearch_amd import _lib

    rng = np.random.default_rng(3)
    n_docs = 4000
    W, R, H = synth_postings(rng, n_docs, [0.6, 0.4], n_fields=3, max_pos=8)
    hi = m.index_from_hits(W, R, H, n_terms=2, total_docs=n_docs, n_fields=3)
    rows = make_rows(rng, n_docs)
    nan_rows = rows.copy()
    nan_rows[17, FLT] = 0x7FC00000
    seg = m.Segment(ctx, hi)
    root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
    big = m.Order([m.OrderPart(BIG * 32, 64, kind=m.SORTKEY_INT64)])
    two = m.Order([m.OrderPart(BITS * 32 + 31, 1), m.OrderPart(TS * 32, 32)])
    plain = m.Query(root, ranker=m.SPH_RANK_BM25)
    Q = lambda o, **kwa: m.Query(root, ranker=m.SPH_RANK_BM25, order=o, **kwa)
    try:
        got = batch.search(seg, [plain, Q(big), Q(two)])  # no attribute rows yet
        assert [g.status for g in got] == [0, -2, -2] and got[1].order_key is None
        seg.set_attrs(nan_rows)
        fl = m.Order([m.OrderPart(TS * 32, 32), m.OrderPart(FLT * 32, 32, kind=m.SORTKEY_FLOAT)])
        blob = m.Order([m.OrderPart(-1, 0), m.OrderPart(TS * 32, 32)])
        got = batch.search(seg, [plain, Q(big, cutoff=50), Q(big), Q(fl), Q(two), Q(blob)])
        assert [g.status for g in got] == [0, -2, 0, -2, 0, -2]
        assert "blob" in _lib.lib().mrk_last_error().decode()
        # hostile specs fail the submit: MRK_E_INVAL
        for bad in (m.Order([m.OrderPart(BIG * 32 + 16, 64, kind=m.SORTKEY_INT64)]), m.Order([m.OrderPart(STRIDE * 32 - 32, 64, kind=m.SORTKEY_INT64)]),
                    m.Order([m.OrderPart(BIG * 32, 64, kind=m.SORTKEY_INT64), m.OrderPart(TS * 32, 32)]), m.Order([m.OrderPart(30, 5), m.OrderPart(TS * 32, 32)]),
                    m.Order([m.OrderPart(TS * 32, 32)] * 3), m.Order([]), m.Order([m.OrderPart(TS * 32, 32), m.OrderPart(0, 32, kind=5)]),
                    m.Order([m.OrderPart(TS * 32, 32), m.OrderPart(FLT * 32, 32)], then_weight=3)):
            with pytest.raises(Exception):
                batch.search(seg, [plain, Q(bad)])
        with pytest.raises(Exception):
            batch.search(seg, [m.Query(root, sort=m.Sort(TS * 32, 32), order=two)])
        assert batch.search(seg, [plain])[0].status == 0
    finally:
        seg.close()
