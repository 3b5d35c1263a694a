"""GPU: the state rankers (RankStateT::update / finalize and hit_rank_prox<2/3/4>, csrc/mrk_khits.h) and the weight bounds in front of them
(prox_bounds, csrc/mrk_kprune.h, in scan_bt_kernel<true>) on the corpora of rank_edges_common.py: one doc per named edge.  test_rank_edges_cpu.py holds the
oracle against an independent model on the same corpora, so device == oracle here is device == model.

Every query is compared bit for bit with the oracle -- rowids, weights, total_found -- under every ranker its shape may run under, with max_matches >= the
docs, 3 and 1, field weights None / primes / a set with a 0 and a negative / a set shorter than the field count / a set that sums below 0, index_weight 1 and 3,
and every batch is searched twice.  A batch holds the queries of ONE rank pass, and mrk_batch_stats.mq_chunks says which one ran:

    P  AND / OR of 2-4 distinct keywords, PROXIMITY_BM25 / PROXIMITY           queue 0, hit_rank_prox<2/3/4>   (> 0, 0, 0)
    L  the same under SPH04 / WORDCOUNT / MATCHANY / FIELDMASK, a lone keyword
       under those four, repeated keywords under all six                        queue 0, hit_rank_plain         (> 0, 0, 0)
    F  "a b" c, "a b c"~2, a NEAR/2 b under the six hit rankers                 queue 1, hit_pass               (., > 0, 0)
    G  AND of 5..8 keywords under the six hit rankers                           queue 2, the generic evaluator  (., ., > 0)
    B  everything flat under BM25 / NONE, a lone keyword under the proximity
       pair: no hit pass at all                                                 (0, 0, 0)

P and L share a queue: rank_kernel picks hit_rank_prox for the proximity pair over distinct keywords (fast_prox, mrk_rank.hip), which is what sorts the
shapes into the two.  A query the planner sends to another queue turns its batch red.  VLB-direct reads no hits and declines every state ranker, loudly: its
third opinion covers route B's pure ANDs only.

The bounds part runs AND / OR / MAYBE of two keywords that stand in every one of 6000 docs (n_items_bt > 0: the tree kernel with the pruning instance)
with the attaining docs of rank_edges_common.bounds_corpus on the class's lowest and highest rowids, max_matches chosen so that an attaining doc is rank 1,
rank K and rank K + 1 -- under the default bound on the corpus flagged by keyword, and under prox_bound_keywords on its twin flagged by position.  Three
weight sets: "pos" (the plain ends on the cut), "neg" (one negative field among positive ones: its docs far below the cut) and "neglead" (every weight
negative, the corpus's field the least so: its docs lead and the SWAPPED ends `w < 0 ? w x h : w x one` lie on the cut); the query a@1 b@11 swaps which
class runs to 2, so that each class attains each end under some query."""
import numpy as np
import pytest

import rank_edges_common as C
from rank_edges_common import A, B
from test_gpu_parity import orc_index_of, to_orc

pytestmark = pytest.mark.gpu

ROUTES = ["P", "L", "F", "G", "B"]


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    segs = {}
    yield m, ctx, batch, segs
    for seg in segs.values():
        seg.close()
    batch.close()
    ctx.close()


_wanted = {}


def wanted(orc, m, name):
    """the oracle's answers for every route of one segment: computed once, shared, never changed"""
    if name not in _wanted:
        hi, _, _ = C.segment(name)
        oi = orc_index_of(orc, hi)
        _wanted[name] = {route: [to_orc(orc, q).run(oi) for _, _, q in qs] for route, qs in C.queries(m, name, index_weights=(1, 3)).items()}
    return _wanted[name]


def segment_on(dev, name):
    m, ctx, _, segs = dev
    if name not in segs:
        segs[name] = m.Segment(ctx, C.segment(name)[0])
    return segs[name]


def same(tag, q, g, w, names=None):
    assert g.status == 0, (tag, g.status)
    assert g.total_found == w.total_found, (tag, g.total_found, w.total_found)
    assert np.array_equal(g.rowid, w.rowid), (tag, g.rowid[:10], w.rowid[:10])
    if not np.array_equal(g.weight, w.weight):
        bad = np.flatnonzero(g.weight != w.weight)
        row = int(g.rowid[bad[0]])
        cell = next((c for c, r in (names or {}).items() if r == row), None)
        raise AssertionError((tag, q.ranker, q.max_matches, q.field_weights, q.index_weight, bad.size, row, cell, int(g.weight[bad[0]]), int(w.weight[bad[0]])))


def check_route(route, mq):
    if route in ("P", "L"):
        assert mq[0] > 0 and mq[1] == 0 and mq[2] == 0, (route, mq)
    elif route == "F":
        assert mq[1] > 0 and mq[2] == 0, (route, mq)
    elif route == "G":
        assert mq[2] > 0, (route, mq)
    else:
        assert mq == [0, 0, 0], (route, mq)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", C.SEGMENT_IDS)
def test_route_on_segment(orc, dev, name, route):
    m, ctx, batch, _ = dev
    hi, docs, names = C.segment(name)
    qs = C.queries(m, name, index_weights=(1, 3))[route]
    want = wanted(orc, m, name)[route]
    seg = segment_on(dev, name)
    n_rows = 0
    for i in range(0, len(qs), batch.max_queries):
        part = qs[i:i + batch.max_queries]
        for rep in range(2):
            got = batch.search(seg, [q for _, _, q in part])
            st = batch.stats()
            assert st["packed"] == 1 and st["n_rerun"] == 0, st
            check_route(route, list(st["mq_chunks"]))
            for j, ((shape, wname, q), g) in enumerate(zip(part, got)):
                same((name, route, shape, wname, rep), q, g, want[i + j], names)
                n_rows += g.rowid.size
    assert n_rows > 0


def test_the_batches_rank_every_cell(orc, dev):
    """what the batches above compared: every cell is a match of some query of the route it is made for, with max_matches above the docs"""
    m = dev[0]
    for name in C.SEGMENT_IDS:
        hi, docs, names = C.segment(name)
        qs = C.queries(m, name, index_weights=(1, 3))
        w = wanted(orc, m, name)
        shapes = C.shapes(m, name)
        for cell in C.CELLS:
            for (shape, family) in cell.expect:
                hit = False
                for route in ROUTES:
                    for (s, _, q), r in zip(qs.get(route, []), w.get(route, [])):
                        if s == shape and q.max_matches == 1000 and C.ranker_family(m).get(q.ranker) == family:
                            assert names[cell.name] in r.rowid.tolist(), (name, cell.name, shape)
                            hit = True
                assert hit, (name, cell.name, shape, family)
        assert all(r.total_found <= len(docs) for rs in w.values() for r in rs)


@pytest.mark.parametrize("name", ["N-inline-128", "N-plain-128"])
def test_vlb_direct_answers_what_it_can_and_declines_the_rest(orc, dev, name):
    """VLB-direct reads no hits: the state rankers run on the packed path only.  What it can give a third opinion on is route B's pure ANDs (the BM25 part and
    the matched fields every state ranker's weight is built on); every query of P and L must come back declined, MRK_E_UNSUPPORTED, never with an answer."""
    m, ctx, batch, _ = dev
    hi, docs, names = C.segment(name)
    seg = segment_on(dev, name)
    qs = C.queries(m, name, index_weights=(1, 3))
    want = wanted(orc, m, name)
    pure = [(x, w) for x, w in zip(qs["B"], want["B"]) if (x[2].root.word is not None or x[2].root.op == m.SPH_QUERY_AND) and x[2].ranker != m.SPH_RANK_PROXIMITY]
    assert len(pure) > 300
    try:
        ctx.set("path", 1)
        for i in range(0, len(pure), batch.max_queries):
            part = pure[i:i + batch.max_queries]
            got = batch.search(seg, [x[2] for x, _ in part])
            st = batch.stats()
            assert st["packed"] == 0 and list(st["mq_chunks"]) == [0, 0, 0], st
            for ((shape, wname, q), w), g in zip(part, got):
                same((name, "vlb", shape, wname), q, g, w, names)
        for route in ("P", "L"):
            part = [q for _, _, q in qs[route] if not (q.root.word is not None and q.ranker == m.SPH_RANK_PROXIMITY_BM25)][:batch.max_queries]
            got = batch.search(seg, part)
            assert all(g.status == -2 and g.rowid.size == 0 for g in got), [g.status for g in got][:8]
    finally:
        ctx.set("path", 0)


# --------------------------------------------------------------------------- the bounds part
BOUNDS_KS = (1, 8, 9, 10, 17, 18, 19, 20, 21, 100, 1000)
FIT = {"fit": [1, 1, 4208, 0, 0, 0, 0, 0], "no_fit": [1, 1, 4209, 0, 0, 0, 0, 0]}  # sum |w| = 4210: the bounds fit 32 bits and the scan prunes; 4211: it does not


def bounds_queries(m):
    kw = m.XQNode.keyword
    roots = {"and": m.XQNode.AND(kw(A, 1), kw(B, 2)), "or": m.XQNode(m.SPH_QUERY_OR, [kw(A, 1), kw(B, 2)]), "maybe": m.XQNode(m.SPH_QUERY_MAYBE, [kw(A, 1), kw(B, 2)]),
             "gap": m.XQNode.AND(kw(A, 1), kw(B, C.BOUNDS_GAP_QPOS))}  # (a@1 b@11: the fillers run to 2 and the adjacent pair to 1)
    out = []
    for rname, root in roots.items():
        for rk in (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_PROXIMITY):
            for fname, fw in list(C.BOUNDS_FW.items()) + [("none", None)]:
                for k in BOUNDS_KS:
                    out.append(((rname, rk, fname, k), m.Query(root, ranker=rk, max_matches=k, field_weights=fw)))
    for fname, fw in FIT.items():
        assert C.bounds_fit(fw, 1) == (fname == "fit")
        for k in (10, 1000):
            out.append((("and", m.SPH_RANK_PROXIMITY_BM25, fname, k), m.Query(roots["and"], ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=k, field_weights=fw)))
    out.append((("and", m.SPH_RANK_PROXIMITY_BM25, "pos x3", 10), m.Query(roots["and"], ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=10, field_weights=C.BOUNDS_FW["pos"], index_weight=3)))
    return out


@pytest.mark.parametrize("mode", ["default", "prox_bound_keywords"])
def test_bounds_corpus(orc, dev, mode):
    m, ctx, batch, _ = dev
    by_position = mode == "prox_bound_keywords"  # the tighter bound is the caller's statement about the index: it runs on the twin flagged by position
    hi, docs, kinds = C.bounds_segment(by_position)
    oi = orc_index_of(orc, hi)
    qs = bounds_queries(m)
    want = [to_orc(orc, q).run(oi) for _, q in qs]
    seg = m.Segment(ctx, hi)
    try:
        ctx.set("prox_bound_keywords", 1 if by_position else 0)
        for i in range(0, len(qs), batch.max_queries):
            for rep in range(2):
                got = batch.search(seg, [q for _, q in qs[i:i + batch.max_queries]])
                st = batch.stats()
                assert st["packed"] == 1 and st["n_rerun"] == 0 and st["n_items_bt"] > 0, st
                mq = list(st["mq_chunks"])
                assert mq[0] > 0 and mq[1] == 0 and mq[2] == 0, mq
                for (tag, q), g, w in zip(qs[i:], got, want[i:]):
                    same((mode, rep) + tag, q, g, w)
        # a field-limited keyword: the block scan's, without the bounds -- exact all the same
        lim = [m.Query(m.XQNode.AND(m.XQNode.keyword(A, 1), m.XQNode.keyword(B, 2, 1 << C.BOUNDS_FIELD)), ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=k,
                       field_weights=C.BOUNDS_FW["pos"]) for k in (10, 1000)]
        got = batch.search(seg, lim)
        assert batch.stats()["n_items_bt"] == 0, batch.stats()
        for q, g in zip(lim, got):
            same((mode, "field limit", q.max_matches), q, g, to_orc(orc, q).run(oi))
    finally:
        ctx.set("prox_bound_keywords", 0)
        seg.close()
    # what was compared: under BOUNDS_FW["pos"] the attaining docs lead the list, lowest and highest rowids of their class among them, and the
    # max_matches above cut at rank K and K + 1 of an attaining doc
    full = next(w for (tag, q), w in zip(qs, want) if tag == ("and", m.SPH_RANK_PROXIMITY_BM25, "pos", 1000))
    assert full.total_found == C.BOUNDS_DOCS
    lead = full.rowid[:18].tolist() if not by_position else full.rowid[:9].tolist()
    top_kinds = ("shared3", "adjacent") if not by_position else ("adjacent",)
    assert lead == [r for k in top_kinds for r in sorted(kinds[k])], lead
    assert lead[0] < C.BOUNDS_EDGE_ROWS and lead[8] >= C.BOUNDS_DOCS - C.BOUNDS_EDGE_ROWS
    assert {8, 9, 10} <= set(BOUNDS_KS) and {17, 18, 19} <= set(BOUNDS_KS)
    # under "neg" the low class leads and every doc of the negative field lies far below the cut: that set holds the mixed signs, not the swapped ends
    neg = next(w for (tag, q), w in zip(qs, want) if tag == ("and", m.SPH_RANK_PROXIMITY_BM25, "neg", 1000))
    assert set(neg.rowid.tolist()) <= set(kinds["low"])
    # under "neglead" (every weight negative, field 2 the least so) the docs of the negative field lead and the SWAPPED ends lie on the cut.
    # a@1 b@2: the fillers attain the swapped upper end w x one: rank 1 (the class's lowest rowid), rank K and K + 1 for every K
    lead = next(w for (tag, q), w in zip(qs, want) if tag == ("and", m.SPH_RANK_PROXIMITY_BM25, "neglead", 1000))
    fillers = sorted(kinds["filler"])
    assert lead.rowid.tolist() == fillers[:1000] and len(set(lead.weight.tolist())) == 1
    # a@1 b@11: the adjacent pair attains the swapped upper end on ranks 1..9, at the lowest and the highest rowids; shared3 and the tf docs follow; from
    # rank 20 on the fillers, which attain the swapped lower end w x h: max_matches 19, 20 and 21 put one on rank K + 1, K and K - 1
    gap = next(w for (tag, q), w in zip(qs, want) if tag == ("gap", m.SPH_RANK_PROXIMITY_BM25, "neglead", 1000))
    rows = gap.rowid.tolist()
    assert rows[:9] == sorted(kinds["adjacent"]) and rows[0] < C.BOUNDS_EDGE_ROWS and rows[8] >= C.BOUNDS_DOCS - C.BOUNDS_EDGE_ROWS
    assert set(rows[9:19]) == set(kinds["shared3"]) | set(kinds["tf255"]) and rows[19:] == fillers[:981]
    assert gap.weight[19] == gap.weight[-1] < gap.weight[18] and {19, 20, 21} <= set(BOUNDS_KS)
    # ... and under "pos" with that query the fillers attain the plain upper end as one tied class of thousands
    gpos = next(w for (tag, q), w in zip(qs, want) if tag == ("gap", m.SPH_RANK_PROXIMITY_BM25, "pos", 1000))
    assert gpos.rowid.tolist() == fillers[:1000]
