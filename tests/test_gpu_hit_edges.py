"""GPU: the three hit-stream decoders of mrk_khits.h (read_vlb32 / hit_advance, hs_fill / hs_advance, hit_rank_prox's `next`) on the
corpora of hit_edges_common.py, which reach every (varint length, window offset) pair, the terminator at every offset, every start
alignment and a list on the last byte of .spp (test_hit_edges_cpu.py asserts that from the bytes).  Every route runs as a batch of its
own on every segment, bit-exact against the oracle, with max_matches = 1000 >= the docs of a segment, so every doc's weight is compared;
mrk_batch_stats.mq_chunks says which rank pass the batch took:

    P  AND of 2-4 distinct keywords, PROXIMITY_BM25 / PROXIMITY      queue 0, hit_rank_prox<2/3/4>   (> 0, 0, 0)
    L  the same and A | B under SPH04 / WORDCOUNT / MATCHANY /
       FIELDMASK, a repeated keyword, the MergeHits3 field test       queue 0, hit_rank_plain         (> 0, 0, 0)
    F  PHRASE, "a b"~3, BEFORE, NEAR, NOTNEAR, ^a, a$, @f[N] a        queue 1, hit_pass               (., > 0, 0)
    S  ("A B") | E: the phrase leaf is decided inside the block scan by hit_pass.  Under BM25 nothing is queued: (0, 0, 0).  Under
       PROXIMITY_BM25 the matches go to queue 1 for their weight (TF_PHRASE_LEAF is part of TF_FAT): (0, > 0, 0)
    G  AND of five keywords, a five-word phrase                       queue 2, gen_open / gen_term    (., ., > 0)

'^C A' of the plan matches nothing here (C never stands at position 1), so '^A C' runs next to it: A's lists begin at position 1."""
import numpy as np
import pytest

import hit_edges_common as C
from test_gpu_parity import orc_index_of, to_orc

pytestmark = pytest.mark.gpu

ROUTES = ["P", "L", "F", "S_bm25", "S_prox", "G"]


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
    """the oracle's answers for every route of one segment, computed once"""
    if name not in _wanted:
        hi, _ = C.segment(name)
        oi = orc_index_of(orc, hi)
        _wanted[name] = {route: [to_orc(orc, q).run(oi) for q in qs] for route, qs in C.routes(m, hi.n_fields).items()}
    return _wanted[name]


def segment_on(dev, name):
    m, ctx, _, segs = dev
    if name not in segs:
        segs[name] = m.Segment(ctx, C.segment(name)[0])
    return segs[name]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", C.SEGMENT_IDS)
def test_route_on_segment(orc, dev, name, route):
    m, ctx, batch, _ = dev
    hi, docs = C.segment(name)
    qs = C.routes(m, hi.n_fields)[route]
    want = wanted(orc, m, name)[route]
    got = batch.search(segment_on(dev, name), qs)
    st = batch.stats()
    assert st["packed"] == 1 and st["n_rerun"] == 0, st
    mq = st["mq_chunks"]
    if route in ("P", "L"):
        assert mq[0] > 0 and mq[1] == 0 and mq[2] == 0, mq
    elif route == "F":
        assert mq[1] > 0 and mq[2] == 0, mq
    elif route == "S_bm25":
        assert mq == [0, 0, 0], mq
    elif route == "S_prox":
        assert mq[0] == 0 and mq[1] > 0 and mq[2] == 0, mq
    else:
        assert mq[2] > 0, mq
    n_rows = 0
    for i, (q, g, w) in enumerate(zip(qs, got, want)):
        assert g.status == 0, (i, g.status)
        assert g.total_found == w.total_found <= q.max_matches, (i, g.total_found, w.total_found)
        assert np.array_equal(g.rowid, w.rowid), (i, g.rowid[:10], w.rowid[:10])
        if not np.array_equal(g.weight, w.weight):
            bad = np.flatnonzero(g.weight != w.weight)
            d = docs[int(g.rowid[bad[0]])]
            raise AssertionError((i, bad.size, int(g.rowid[bad[0]]), int(g.weight[bad[0]]), int(w.weight[bad[0]]), d.kind, d.slot, getattr(d, "cell", None)))
        n_rows += g.rowid.size
    assert n_rows > 0


def test_every_route_ranks_the_crafted_docs(orc, dev):
    """what the batches above compared: all docs under P, L and G's ANDs, the phrase docs under F and G's phrase"""
    m = dev[0]
    for name in C.SEGMENT_IDS:
        hi, docs = C.segment(name)
        w = wanted(orc, m, name)
        assert all(r.total_found == len(docs) for r in w["P"][:6] + w["L"][:16] + w["G"][:2] + w["S_bm25"] + w["S_prox"])
        n_phrase = len(C.phrase_docs(docs))
        assert w["F"][0].total_found == n_phrase == w["G"][2].total_found + sum(1 for d in docs if d.kind in ("max_pos_lone", "max_pos_last", "max_pos_last_end") and d.slot == C.T_B)
        assert all(r.total_found > 0 for i, r in enumerate(w["F"]) if i // 2 != 6)  # ('^C A' alone is empty)


def test_vlb_direct_path_sizes_no_match_queue(orc, dev):
    m, ctx, batch, _ = dev
    hi, docs = C.segment("N-plain-128")
    qs = [m.Query(m.XQNode.AND(C.kw(m, C.T_A), C.kw(m, C.T_B)), ranker=rk, max_matches=1000, field_weights=C.PRIMES[:8])
          for rk in (m.SPH_RANK_BM25, m.SPH_RANK_NONE)]
    oi = orc_index_of(orc, hi)
    try:
        ctx.set("path", 1)
        got = batch.search(segment_on(dev, "N-plain-128"), qs)
        st = batch.stats()
    finally:
        ctx.set("path", 0)
    assert st["packed"] == 0 and st["mq_chunks"] == [0, 0, 0] and st["n_rerun"] == 0, st
    for q, g in zip(qs, got):
        w = to_orc(orc, q).run(oi)
        assert g.status == 0 and g.total_found == w.total_found == len(docs)
        assert np.array_equal(g.rowid, w.rowid) and np.array_equal(g.weight, w.weight)
