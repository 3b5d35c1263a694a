"""GPU: the nodes of the generic per-doc evaluator (gen_eval, csrc/mrk_keval.h) and their specialised twins (mrk_khits.h, the quorum
order code of mrk_scan_pk.hip) on the corpora of gen_edges_common.py -- distance ladders, field boundaries, the end flag inside
chains, shared positions, the three-stream merge, quorum order, list memory and the tf escape, the ring NEAR with its probe launch,
BEFORE spans, units.  test_gen_edges_cpu.py checks that every cell stands where its name says and that route() is the planner's.

Every query is compared bit for bit with the oracle's full answer: status 0, rowids in order, weights, total_found.  Every case is
asked under all eight rankers where its table row does not fix them, with max_matches 1000 and 3, with field weights None and a set
that holds a 0 and a negative.  Batches are pure: mrk_batch_stats.mq_chunks is (0, 0, > 0) for a generic batch and (., ., 0) for a
specialised one.  Every batch is searched twice and gives the same bytes; a generic batch a third time with gen_lane_hits = 16
(the lane arena's minimum: almost every list goes to the shared spill area), the same bytes again.  No query comes back declined, no
case is skipped, and the number of compared queries is the tables' length."""
import numpy as np
import pytest

import gen_edges_common as ge
from runtime_declines_common import Settings
from test_gpu_batch_state import oracle_all
from test_gpu_parity import orc_index_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, ge.MAX_BATCH)
    yield m, ctx, batch
    batch.close()
    ctx.close()


def same_bytes(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.status == y.status and x.total_found == y.total_found and x.rowid.tobytes() == y.rowid.tobytes() and x.weight.tobytes() == y.weight.tobytes(), (what, i)


def run_pure_batches(orc, dev, hi, batches, what, rowid_base=0, lane_hits=(16,), stats=None):
    """-> the number of queries compared.  hi stays referenced while its oracle index is in use (the oracle borrows its memory)."""
    m, ctx, batch = dev
    seg = m.Segment(ctx, hi, rowid_base=rowid_base)
    oi = orc_index_of(orc, hi)
    n = 0
    try:
        for route, items in batches:
            qs = [q for _, q in items]
            assert 0 < len(qs) <= ge.MAX_BATCH
            want = oracle_all(orc, hi, qs, oi)
            got = batch.search(seg, qs)
            st = batch.stats()
            mq = st["mq_chunks"]
            if stats is not None:
                stats.append(st)
            assert st["packed"] == 1, (what, st)
            if route == "G":
                assert mq[0] == 0 and mq[1] == 0 and mq[2] > 0, (what, route, mq)
            else:
                assert mq[2] == 0, (what, route, mq)
            for (case, q), g, w in zip(items, got, want):
                name = (what, route, getattr(case, "name", case), "ranker", q.ranker, "max_matches", q.max_matches, "fw", q.field_weights)
                assert g.status == 0, (name, "status", g.status)
                assert g.total_found == w.total_found, (name, "total_found", g.total_found, w.total_found, g.rowid[:8], w.rowid[:8])
                assert np.array_equal(g.rowid, w.rowid), (name, "rowids", g.rowid[:8], w.rowid[:8], g.weight[:8], w.weight[:8])
                assert np.array_equal(g.weight, w.weight), (name, "weights", g.rowid[:8], g.weight[:8], w.weight[:8])
                n += 1
            same_bytes(batch.search(seg, qs), got, (what, route, "the second search"))
            if route == "G":
                for lh in lane_hits:
                    with Settings(ctx, gen_lane_hits=lh):  # (the default back in its __exit__, whatever happens)
                        again = batch.search(seg, qs)
                    same_bytes(again, got, (what, route, "gen_lane_hits", lh))
    finally:
        seg.close()
        del oi
    return n


# ------------------------------------------------------------------ parts 1-5, 9, 10: the table cases
@pytest.mark.parametrize("block,fmt", ge.FORMS)
@pytest.mark.parametrize("key,layout", ge.corpus_ids())
def test_table_cases(orc, dev, key, layout, block, fmt):
    m = dev[0]
    c = ge.corpus(key, layout)
    cases = ge.cases(m, key)
    assert cases
    batches, n_queries = ge.batches_of(m, cases, c)
    routes = {r for r, _ in batches}
    assert "G" in routes and ("S" in routes or key == "units")  # the generic evaluator and its specialised twins see the same docs (units: no twin)
    hi = c.index(m, block, fmt)
    n = run_pure_batches(orc, dev, hi, batches, (key, layout, block, fmt))
    assert n == n_queries == sum(len(ge.queries_of(m, case, c)) for case in cases)


# ------------------------------------------------------------------ part 6: quorum order
@pytest.mark.parametrize("block,fmt", ge.FORMS)
def test_quorum_order(orc, dev, block, fmt):
    """Quorums of 3, 5 and 8 keywords whose doclists end at different rows, docs at last - 1, last and last + 1 of every
    keyword, thresholds 1, 2, k - 1 and k, one keyword absent from the dictionary; at the root (specialised) and below AND / OR /
    MAYBE / BEFORE, under BM25 and PROXIMITY_BM25."""
    m = dev[0]
    H = ge.quorum_corpus()
    hi = H.index(m, ge.Q_TERMS, ge.Q_DOCS, 2, block, fmt)
    by_route = {"S": [], "G": []}
    qs = ge.quorum_queries(m)
    for name, q in qs:
        by_route[ge.route(m, q.root, q.ranker)].append((name, q))
    assert by_route["S"] and by_route["G"]
    batches = [(r, v[i:i + ge.MAX_BATCH]) for r, v in by_route.items() for i in range(0, len(v), ge.MAX_BATCH)]
    assert run_pure_batches(orc, dev, hi, batches, (ge.QUORUM_EDGE, block, fmt)) == len(qs)


# ------------------------------------------------------------------ part 7: list memory and the tf escape
@pytest.mark.parametrize("block,fmt", ge.FORMS)
def test_list_memory_and_tf_escape(orc, dev, block, fmt):
    """gen_lane_hits = 256 (the default), 16 (the minimum) and 64: the takes of the docs with tf = 1..20 land on the lane slice's last
    slot and one past it, the docs with tf = 254, 255, 256 and 300 go through exc_tf, with and without a field limit on the keyword."""
    m = dev[0]
    c = ge.corpus("memory")
    cases = ge.cases(m, "memory")
    batches, n_queries = ge.batches_of(m, cases, c)
    assert {r for r, _ in batches} == {"G"}
    hi = c.index(m, block, fmt)
    assert run_pure_batches(orc, dev, hi, batches, ("memory", block, fmt), lane_hits=(16, 64)) == n_queries


# ------------------------------------------------------------------ part 8: the ring NEAR and its probe launch
RING_CONFIGS = [(128 << 10, 0), (4096, 0), (4096, (1 << 32) - ge.RING_TOTAL - 3)]


@pytest.mark.parametrize("block,fmt", ge.FORMS)
def test_ring_near(orc, dev, block, fmt):
    """A root NEAR over 3, 4 and 8 operands: rowid 0 inserts, inserting docs at r - 1 and r, more than 64 and more than 2048 rowids apart,
    several such queries in one batch (each has a near_tab of its own), a rowid_base near 2^32.  With item_bytes = 4096 the doclists
    of the filler docs are cut into more work items than with the default (mrk_batch_stats.n_items is the witness), so the inserting
    doc at row 0 and the dependent doc behind the fillers are evaluated by different items."""
    m, ctx, _ = dev
    c = ge.corpus("ring")
    cases = ge.cases(m, "ring")
    batches, n_queries = ge.batches_of(m, cases, c)
    assert {r for r, _ in batches} == {"G"} and n_queries >= 2
    hi = c.index(m, block, fmt)
    n_items = {}
    for item_bytes, rowid_base in RING_CONFIGS:
        ctx.set("item_bytes", item_bytes)
        try:
            stats = []
            assert run_pure_batches(orc, dev, hi, batches, ("ring", block, fmt, item_bytes, rowid_base), rowid_base=rowid_base, stats=stats) == n_queries
            n_items[(item_bytes, rowid_base)] = [st["n_items"] for st in stats]
        finally:
            ctx.set("item_bytes", 128 << 10)
    print("ring n_items", block, fmt, n_items)
    for cfg in RING_CONFIGS[1:]:
        assert all(small > dflt for small, dflt in zip(n_items[cfg], n_items[RING_CONFIGS[0]])), n_items
