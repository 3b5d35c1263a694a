"""GPU: one submit that holds a query of every class -- relevance, Query.sort, a one-part Query.order, a 64-bit order, a two-part
order, the weight in front of a part, the weight ascending alone, a query the planner declines, a query that matches nothing -- and
what leaves the batch for each of them in each of the three exchange-row formats (narrow, wide, order), exported and through a
standing destination, with mrk_batch_orows_weight_first off and on.  The rule a row follows:
  narrow rows answer relevance queries only; wide rows also a sort and a one-part order (a 32-bit mapped key); order rows also a
  64-bit key and, only with the switch on, a weight-first order; a query the planner declined leaves declined in every format.
A declined row has count 0, no keys, MRK_ROW_DECLINED alone in its total_found word, a zero plane and spec word 0.  An answered row
equals mrk_batch_result: the keys in order, total_found, the plane unmapped through dist.unmap_keys / unmap_order_keys, the spec
word dist.sort_spec_word / order_spec_word build.  Then: a resubmit of relevance queries alone flags no row; and a 64-bit order whose
candidate list overflows leaves MRK_ROW_RERUN in a standing order row until mrk_batch_wait reran it and an export repaired the row.
Every comparison is exact."""
import numpy as np
import pytest

import sort_merge_common as smc
from helpers import synth_postings
from test_gpu_order import CONST
from test_gpu_order import make_rows as order_rows
from test_gpu_order import part_specs
from test_gpu_order_merge import Hip
from test_gpu_parity import kw

pytestmark = pytest.mark.gpu

K1 = 1024
N_DOCS = 4000
U32C, I64C, CATC, STRIDE = 0, 1, 3, 4  # dwords of a row: a 32-bit column, a 64-bit one (low dword first), one of five distinct values
KINDS = ("rows", "srows", "orows")
CLASSES = ("relevance", "sort", "one-part order", "64-bit order", "two-part order", "weight first + part", "weight asc alone", "planner-declined", "matches nothing")
# the row formats that answer a class (weight-first orders: order rows, under the switch only -- WF)
WF = "orows under the switch"
ANSWERED = {"relevance": KINDS, "matches nothing": KINDS, "sort": ("srows", "orows"), "one-part order": ("srows", "orows"), "64-bit order": ("orows",),
            "two-part order": ("orows",), "weight first + part": WF, "weight asc alone": WF, "planner-declined": ()}


def answered(cls, kind, switch):
    return (kind == "orows" and switch) if ANSWERED[cls] == WF else kind in ANSWERED[cls]


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    hip = Hip()
    rng = np.random.default_rng(71)
    W, R, H = synth_postings(rng, N_DOCS, [0.7, 0.5, 0.3], n_fields=3, max_pos=8)
    hi = m.index_from_hits(W, R, H, n_terms=3, total_docs=N_DOCS, n_fields=3)
    rows = np.zeros((N_DOCS, STRIDE), np.uint32)
    rows[:, U32C] = rng.integers(0, 1 << 32, N_DOCS, dtype=np.uint64).astype(np.uint32)
    big = (rng.integers(-2, 3, N_DOCS).astype(np.int64) << 32) + rng.integers(0, 1 << 32, N_DOCS, dtype=np.uint64).astype(np.int64)
    rows[:, I64C:I64C + 2] = big.view(np.uint32).reshape(N_DOCS, 2)
    rows[:, CATC] = np.arange(N_DOCS) % 5
    seg = m.Segment(ctx, hi)
    seg.set_attrs(rows)
    yield m, ctx, hip, seg
    hip.free()
    seg.close()
    ctx.close()


def every_class(m, K):
    P, O = m.OrderPart, m.Order
    root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
    Q = lambda **kwa: m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=K, **kwa)
    qs = [Q(), Q(sort=m.Sort(U32C * 32, 32, desc=True, then_weight=1)), Q(order=O([P(CATC * 32, 32, desc=False)], then_weight=2)),
          Q(order=O([P(I64C * 32, 64, desc=True, kind=m.SORTKEY_INT64)])), Q(order=O([P(CATC * 32, 32), P(U32C * 32, 32, desc=False)], then_weight=0)),
          Q(order=O([P(CATC * 32, 32, desc=True)], weight_first=1)), Q(order=O([], weight_first=2)),
          Q(order=O([P(-1, 0), P(U32C * 32, 32)])),  # a blob-stored sort key: MRK_E_UNSUPPORTED
          Q(filters=[m.Filter(CATC * 32, 32, values=[99])])]
    assert len(qs) == len(CLASSES)
    return qs


def relevance_only(m, n):
    roots = [kw(m, 0, 1), m.XQNode.AND(kw(m, 0, 1), kw(m, 2, 2)), m.XQNode.AND(kw(m, 1, 1), kw(m, 2, 2))]
    return [m.Query(roots[i % 3], ranker=m.SPH_RANK_BM25, max_matches=(7, 1024)[i % 2]) for i in range(n)]


def words(m, kind):
    return {"rows": m.ROW_WORDS, "srows": m.SROW_WORDS, "orows": m.OROW_WORDS}[kind]


def lib_of():
    from manticoresearch_amd import _lib

    return _lib.lib(), _lib.check


def export(m, hip, batch, kind, n):
    lib, chk = lib_of()
    buf = hip.malloc(n * words(m, kind) * 8)
    hip.fill(buf, 0xEE, n * words(m, kind) * 8)
    chk(getattr(lib, f"mrk_batch_export_{kind}")(batch._h, buf))
    return hip.to_host(buf, (n, words(m, kind)))


def spec_word(mdist, kind, q):
    """the spec word an ANSWERED row of q carries"""
    if kind == "rows" or (q.sort is None and q.order is None):
        return 0
    if kind == "srows":  # a sort, or the one-part order that is planned as the same sort
        p, tw = (q.sort, q.sort.then_weight) if q.sort is not None else (q.order.parts[0], q.order.then_weight)
        return mdist.sort_spec_word(p.kind, p.desc, tw, p.bit_count)
    if q.sort is not None:
        return mdist.order_spec_word([q.sort], q.sort.then_weight)
    return mdist.order_spec_word(q.order.parts, q.order.then_weight, weight_first=q.order.weight_first)


def check_row(mdist, kind, cls, q, g, row, is_answered, what):
    if not is_answered:
        assert int(row[K1 + 1]) == mdist.ROW_DECLINED and int(row[K1]) == 0 and not row[:K1].any() and not row[K1 + 2:].any(), (what, "a declined row")
        return
    assert g.status == 0 and not int(row[K1 + 1]) & (mdist.ROW_RERUN | mdist.ROW_DECLINED), (what, "flagged")
    n = len(g.rowid)
    assert n == min(g.total_found, q.max_matches) and (n > 0) == (cls != "matches nothing"), (what, n, g.total_found)
    assert int(row[K1]) == n and int(row[K1 + 1]) == g.total_found, (what, int(row[K1]), n)
    assert np.array_equal(row[:n], smc.make_keys(g.weight, g.rowid)) and not row[n:K1].any(), (what, "keys")
    if kind == "rows":
        return
    spec = spec_word(mdist, kind, q)
    assert int(row[-1]) == spec, (what, hex(int(row[-1])), hex(spec))
    raw = g.sort_key if q.sort is not None else g.order_key  # (None: a relevance query, or the weight alone -- no part of the row is in the order)
    assert (raw is not None) == (spec != 0 and not (q.order is not None and not q.order.parts)), what
    if kind == "srows":
        plane = mdist.srow_mkeys(row)
        assert not plane[n:].any(), (what, "plane past the count")
        if raw is None:
            assert not plane.any(), what
        else:
            assert np.array_equal(mdist.unmap_keys(spec, plane[:n]), raw if q.sort is not None else (raw >> np.uint64(32)).astype(np.uint32)), (what, "plane")
    else:
        plane = mdist.orow_mkeys(row)
        assert not plane[n:].any(), (what, "plane past the count")
        if raw is None:
            assert not plane.any(), what
        else:
            assert np.array_equal(mdist.unmap_order_keys(spec, plane[:n]), raw.astype(np.uint64) << np.uint64(32) if q.sort is not None else raw), (what, "plane")


def submit_all(m, seg, batch, qs, switch):
    batch.orows_weight_first(switch)
    batch.submit(seg, qs)
    batch.wait()
    got = batch.results()
    assert batch.stats()["n_rerun"] == 0 and batch.stats()["packed"] == 1
    assert [g.status for g in got] == [-2 if c == "planner-declined" else 0 for c in CLASSES]
    return got


@pytest.mark.parametrize("K", [7, 1024])
def test_every_class_in_every_format_with_the_switch_off_and_on(dev, K):
    m, ctx, hip, seg = dev
    from manticoresearch_amd import dist as mdist

    qs = every_class(m, K)
    batch = m.Batch(ctx, 16)
    try:
        rows_by = {}
        for switch in (False, True):
            got = submit_all(m, seg, batch, qs, switch)
            for kind in KINDS:
                rows = rows_by[switch, kind] = export(m, hip, batch, kind, len(qs))
                for i, cls in enumerate(CLASSES):
                    check_row(mdist, kind, cls, qs[i], got[i], rows[i], answered(cls, kind, switch), (K, switch, kind, cls))
        # the switch changes the two weight-first rows of the order export, from declined to answered, and nothing else
        wf = [i for i, c in enumerate(CLASSES) if ANSWERED[c] == WF]
        rest = [i for i in range(len(qs)) if i not in wf]
        assert len(wf) == 2
        for kind in KINDS:
            off, on = rows_by[False, kind], rows_by[True, kind]
            assert np.array_equal(off[rest], on[rest]), kind
            if kind != "orows":
                assert np.array_equal(off[wf], on[wf]), kind
        assert all(int(rows_by[False, "orows"][i, K1 + 1]) == mdist.ROW_DECLINED and not int(rows_by[True, "orows"][i, K1 + 1]) & mdist.ROW_DECLINED for i in wf)
    finally:
        batch.close()
        hip.free()


@pytest.mark.parametrize("kind", KINDS)
def test_standing_destination_equals_the_export_and_a_relevance_resubmit_flags_nothing(dev, kind):
    m, ctx, hip, seg = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = lib_of()
    setter = getattr(lib, f"mrk_batch_set_{kind}_dst")
    n, wd = len(CLASSES), words(m, kind)
    batch = m.Batch(ctx, 16)
    dst = hip.malloc(n * wd * 8)
    try:
        chk(setter(batch._h, dst))
        for K in (7, 1024):
            qs = every_class(m, K)
            for switch in ((False, True) if kind == "orows" else (False,)):
                hip.fill(dst, 0xEE, n * wd * 8)
                got = submit_all(m, seg, batch, qs, switch)
                standing = hip.to_host(dst, (n, wd))
                assert np.array_equal(standing, export(m, hip, batch, kind, n)), (K, switch, "standing != exported")
                for i, cls in enumerate(CLASSES):
                    check_row(mdist, kind, cls, qs[i], got[i], standing[i], answered(cls, kind, switch), (K, switch, kind, cls, "standing"))
            # the same batch again, relevance queries alone in every slot: the declines of the submit before leave no trace
            rel = relevance_only(m, n)
            hip.fill(dst, 0xEE, n * wd * 8)
            batch.submit(seg, rel)
            batch.wait()
            got = batch.results()
            assert [g.status for g in got] == [0] * n and batch.stats()["n_rerun"] == 0
            standing = hip.to_host(dst, (n, wd))
            assert np.array_equal(standing, export(m, hip, batch, kind, n)), (K, "resubmit: standing != exported")
            for i in range(n):
                check_row(mdist, kind, "relevance", rel[i], got[i], standing[i], True, (K, kind, i, "resubmit"))
        chk(setter(batch._h, None))
    finally:
        batch.close()
        hip.free()


def test_overflowing_64_bit_order_leaves_rerun_then_the_repaired_row(dev):
    """test_gpu_order_merge.py's overflow -- its big shard of 3 M docs, its order by (bool, a constant second column) at K = 1000: half
    of ~2.4 M matches share the best 64-bit key -- under a standing order-row destination."""
    m, ctx, hip, _ = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = lib_of()
    n_docs = 3_000_000
    hi = m.synth_index(n_docs, [0.8, 0.3], seed=5, max_pos=16)
    rows = order_rows(np.random.default_rng(21), n_docs)
    o, cnt, kind = part_specs(m)["bool"]
    qs = [m.Query(kw(m, 0, 1), ranker=m.SPH_RANK_BM25, max_matches=1000, order=m.Order([m.OrderPart(o, cnt, desc=True, kind=kind), m.OrderPart(CONST * 32, 32, desc=False)], then_weight=1)),
          m.Query(m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2)), ranker=m.SPH_RANK_BM25, max_matches=1000)]
    nq, RW = len(qs), m.OROW_WORDS
    seg = m.Segment(ctx, hi)
    batch = m.Batch(ctx, nq)
    dst = hip.malloc(nq * RW * 8)
    try:
        seg.set_attrs(rows)
        hip.fill(dst, 0xEE, nq * RW * 8)
        chk(lib.mrk_batch_set_orows_dst(batch._h, dst))
        batch.submit(seg, qs)
        hip.sync()  # the submit's kernels are through; mrk_batch_wait has not run
        row = hip.to_host(dst, (nq, RW))
        assert int(row[0, K1 + 1]) == mdist.ROW_RERUN and int(row[0, K1]) == 0 and not row[0, :K1].any() and not row[0, K1 + 2:mdist.OROW_SPEC].any()
        batch.wait()
        assert batch.stats()["n_rerun"] >= 1  # the overflow must happen, else this test shows nothing
        got = batch.results()
        assert got[0].status == 0 and got[0].total_found > 2 * 2 ** 20 and len(got[0].rowid) == 1000
        repaired = export(m, hip, batch, "orows", nq)
        for i, cls in enumerate(("two-part order", "relevance")):
            check_row(mdist, "orows", cls, qs[i], got[i], repaired[i], True, ("rerun", cls))
        assert np.array_equal(hip.to_host(dst, (nq, RW))[1], repaired[1])  # (the standing row of the query next to it was good all along)
        chk(lib.mrk_batch_set_orows_dst(batch._h, None))
    finally:
        batch.close()
        seg.close()
        hip.free()
