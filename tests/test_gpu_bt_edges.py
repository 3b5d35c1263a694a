"""GPU: the tree kernel over bitmap words (scan_bt_kernel, csrc/mrk_scan_bt.hip) at its step, block and window edges.

Every batch is answered three ways -- default settings (stats()["n_items_bt"] says the kernel ran: three work items per query it
takes, 134 windows = 64 + 64 + 6), bt_cover_inv = 0 (n_items_bt == 0: the block scan) and the oracle -- and the three must be equal
bit for bit: status 0, total_found, rowids, weights.  The corpora and what they sit on are described in bt_edges_common.py;
test_bt_edges_cpu.py pins the oracle on them against a numpy model."""
import numpy as np
import pytest

import bt_edges_common as C
from test_gpu_parity import orc_index_of, to_orc

pytestmark = pytest.mark.gpu

DEFAULTS = {"bt_cover_inv": 1024, "bt_phrase": 1, "prox_prune": 1, "prox_bound_keywords": 0}
KS = (1, 20, 1000, 1024)
FIELD_WEIGHTS = (None, [3, 1, 2], [-2, 5, 0], [5000, 1, 1])  # the last: the weight bounds do not fit 32 bits, the pruning is off
INDEX_WEIGHTS = (1, 3)


def rankers(m):
    return (m.SPH_RANK_NONE, m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_PROXIMITY, m.SPH_RANK_SPH04, m.SPH_RANK_WORDCOUNT,
            m.SPH_RANK_MATCHANY, m.SPH_RANK_FIELDMASK)


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 128)
    yield m, ctx, batch
    batch.close()
    ctx.close()


@pytest.fixture(scope="module")
def corpus(dev):
    return C.corpus_a(dev[0])


@pytest.fixture(scope="module")
def corpus_plain(dev):
    """the same hits with 32-doc skiplist blocks and hits kept out of the doclists"""
    return C.corpus_a(dev[0], block=32, fmt=0)


@pytest.fixture(scope="module")
def oindex(orc, corpus):
    return orc_index_of(orc, corpus[0])


def combo(i):
    """the i-th of the 32 (K, field weights, index weight) combinations"""
    return KS[i % 4], FIELD_WEIGHTS[(i // 4) % 4], INDEX_WEIGHTS[(i // 16) % 2]


def ranked_queries(m):
    """Every named tree under every ranker, twice, so that every ranker meets all 32 (K, field weights, index weight) combinations;
    then 100 seeded random trees."""
    qs = []
    for ti, (_, root) in enumerate(C.named_trees(m)):
        for ri, rk in enumerate(rankers(m)):
            for j in range(2):
                k, fw, iw = combo(ti * 2 + j + ri * 5)
                qs.append(m.Query(root, ranker=rk, max_matches=k, field_weights=fw, index_weight=iw))
    for i, root in enumerate(C.random_trees(m, 100)):
        k, fw, iw = combo(i * 7 + 3)
        qs.append(m.Query(root, ranker=rankers(m)[i % 8], max_matches=k, field_weights=fw, index_weight=iw))
    return qs


@pytest.fixture(scope="module")
def ranked(orc, dev, oindex):
    """the queries of the trees-and-rankers test with the oracle's answers: computed once, shared, never changed"""
    qs = ranked_queries(dev[0])
    return qs, [to_orc(orc, q).run(oindex) for q in qs]


def same(a, b, what):
    assert a.status == getattr(b, "status", 0) == 0, (what, a.status, getattr(b, "status", 0))  # (the oracle's results carry none)
    assert a.total_found == b.total_found, (what, a.total_found, b.total_found)
    assert np.array_equal(a.rowid, b.rowid), (what, a.rowid[:8], b.rowid[:8])
    assert np.array_equal(a.weight, b.weight), (what, a.weight[:8], b.weight[:8])


def docs_of(hi):
    return [int(x) for x in hi.dict["docs"]]


def on_and_off(dev, seg, qs, per_pass=3, cover_inv=1024, off=None, on=None):
    """The batch on the tree kernel (default settings, or `on`) and off it (bt_cover_inv = 0, plus `off`); the stat must say so."""
    m, ctx, batch = dev
    hi = seg.host
    n_bt = sum(C.on_tree_kernel(m, q, docs_of(hi), hi.total_docs, cover_inv) for q in qs)
    assert n_bt > 0, "a batch of this suite without a query for the tree kernel"
    try:
        for key, v in (on or {}).items():
            ctx.set(key, v)
        got_on = batch.search(seg, qs)
        st = batch.stats()
        assert st["packed"] == 1 and st["n_items_bt"] == per_pass * n_bt and st["n_items_bm"] >= st["n_items_bt"], (st, n_bt)
        for key, v in {"bt_cover_inv": 0, **(off or {})}.items():
            ctx.set(key, v)
        got_off = batch.search(seg, qs)
        assert batch.stats()["n_items_bt"] == 0, batch.stats()
    finally:
        for key, v in DEFAULTS.items():
            ctx.set(key, v)
    return got_on, got_off, st


def check(orc, dev, hi, qs, want=None, oi=None, rowid_base=0, dead=None, **kw):
    """device on the kernel == device off it == oracle, for every query"""
    m, ctx, batch = dev
    seg = m.Segment(ctx, hi, rowid_base=rowid_base)
    if dead is not None:
        seg.set_dead_rows(dead)
    if want is None:
        oi = oi if oi is not None else orc_index_of(orc, hi)
        oi.dead_rows = dead
        try:
            want = [to_orc(orc, q).run(oi) for q in qs]
        finally:
            oi.dead_rows = None
    out = []
    try:
        for i in range(0, len(qs), batch.max_queries):
            chunk = qs[i:i + batch.max_queries]
            got_on, got_off, _ = on_and_off(dev, seg, chunk, **kw)
            for j in range(len(chunk)):
                same(got_on[j], want[i + j], ("tree kernel vs oracle", i + j))
                same(got_off[j], want[i + j], ("bt_cover_inv=0 vs oracle", i + j))
            out += got_on
    finally:
        seg.close()
    return out


def test_trees_and_rankers(orc, dev, corpus, ranked):
    qs, want = ranked
    check(orc, dev, corpus[0], qs, want=want)


def test_sparse_covers_on_the_kernel(orc, dev, corpus, oindex):
    """'(a|b) f' and 'f MAYBE b' have the 256-doc keyword for their cover, just below 1/1024 of the docs: the default planner leaves them
    to the block scan.  bt_cover_inv = 2^20 sends them to the kernel: a sparse keyword of two blocks that meet on a step's edge drives."""
    m = dev[0]
    hi = corpus[0]
    roots = [r for _, r in C.named_trees(m)]
    moved = [r for r in roots if not C.on_tree_kernel(m, m.Query(r), docs_of(hi), C.N_DOCS) and C.on_tree_kernel(m, m.Query(r), docs_of(hi), C.N_DOCS, 1 << 20)]
    assert len(moved) >= 2
    qs = [m.Query(r, ranker=rk, max_matches=k) for r in moved + roots[:6] for rk in rankers(m)[:4] for k in (1, 1000)]
    got = check(orc, dev, hi, qs, oi=oindex, cover_inv=1 << 20, on={"bt_cover_inv": 1 << 20})
    assert got[1].total_found > 0


def test_the_full_step(orc, dev, corpus, oindex):
    """Keywords 1 and 2 hold all 8192 rowids of step 3: both popcounts of the shared prefix sum at their maximum, every lane with 128
    matches (the note ring wraps), or, under ANDNOT, 8192 bits that cancel."""
    m, ctx, batch = dev
    hi, rows, _ = corpus
    qs = [m.Query(root, ranker=rk, max_matches=k, index_weight=iw) for _, root in C.full_step_trees(m) for rk in rankers(m)
          for k, iw in ((1, 1), (1024, 3))]
    check(orc, dev, hi, qs, oi=oindex)
    # with every row below the step dead its rowids are the lowest: the answer under SPH_RANK_NONE is the step's first K rowids
    lo = C.FULL_STEP * C.STEP
    dead = C.dead_words(C.N_DOCS, np.arange(lo))
    none = [m.Query(root, ranker=m.SPH_RANK_NONE, max_matches=1024, index_weight=3) for _, root in C.full_step_trees(m)]
    for base in (0, 2 ** 32 - C.N_DOCS):
        got = check(orc, dev, hi, none, oi=oindex, dead=dead, rowid_base=base)
        for q, g in zip(none, got):
            total, rowid, weight = C.model(m, q, rows, C.N_DOCS, dead)
            assert g.total_found == total and np.array_equal(g.rowid, rowid) and np.array_equal(g.weight, weight)
        assert got[0].rowid.tolist() == list(range(lo, lo + 1024)) and got[3].rowid[0] >= lo + C.STEP  # 'b c' / 'b -c'


def test_dead_rows(orc, dev, corpus, oindex, ranked):
    """A fifth of the docs dead, the sparse keyword's edge rowids and the last row among them; then the whole full step dead."""
    m = dev[0]
    rng = np.random.default_rng(3)
    killed = np.union1d(rng.choice(C.N_DOCS, C.N_DOCS // 5, replace=False), C.EDGE_ROWIDS)
    qs = ranked[0][::4]
    check(orc, dev, corpus[0], qs, oi=oindex, dead=C.dead_words(C.N_DOCS, killed))
    full = np.arange(C.FULL_STEP * C.STEP, (C.FULL_STEP + 1) * C.STEP)
    step = [m.Query(root, ranker=rk, max_matches=1000) for _, root in C.full_step_trees(m) for rk in rankers(m)[:4]]
    check(orc, dev, corpus[0], step + ranked[0][1::16], oi=oindex, dead=C.dead_words(C.N_DOCS, full))


def test_rowid_bases(orc, dev, corpus, ranked):
    """rowid_base off the window grid, and the exact fit: the segment's last row is rowid 2^32 - 1."""
    qs, want = ranked
    for base in (3 * 65536 + 17, 2 ** 32 - C.N_DOCS):
        check(orc, dev, corpus[0], qs[::2], want=want[::2], rowid_base=base)


def test_block_sizes_and_hit_formats(orc, dev, corpus_plain, ranked):
    """The (32, plain hits) build holds the same hits as the (128, inline hits) one: the same answers."""
    qs, want = ranked
    check(orc, dev, corpus_plain[0], qs[1::2], want=want[1::2])


@pytest.mark.parametrize("fmt", ["inline", "plain"])
def test_phrases_on_bitmap_words(orc, dev, corpus, corpus_plain, fmt):
    """A root phrase of two common words takes its candidates -- the 6000 docs that hold both -- from the bitmap words.  With inline hits
    the lone-hit shortcut accepts 3000 of them, rejects 1500, and hands the 1500 with longer hit lists to the hit pass."""
    m = dev[0]
    hi, rows, classes = corpus if fmt == "inline" else corpus_plain
    k8, k9, a = C.kw(m, 8, 1), C.kw(m, 9, 2), C.kw(m, 0, 3)
    r8, r9 = C.kw(m, 8, 2), C.kw(m, 9, 1)
    roots = [C.PHRASE(m, k8, k9), C.PHRASE(m, r9, r8), C.PROXIMITY(m, 3, k8, k9), C.AND(m, C.PHRASE(m, k8, k9), a)]
    qs = [m.Query(r, ranker=rk, max_matches=k) for r in roots for rk in (m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_SPH04) for k in (20, 1000)]
    got = check(orc, dev, hi, qs, off={"bt_phrase": 0})
    assert np.intersect1d(rows[8], rows[9]).size == C.PH_COMMON
    assert got[0].total_found == C.PH_ACCEPT + C.PH_MULTI_WITH and got[6].total_found == C.PH_REVERSED  # accepted + decided by the hit pass; '"9 8"'
    assert got[12].total_found > got[0].total_found  # '"8 9"~3' takes the gapped and the reversed ones too


def test_pruning_under_ties(orc, dev):
    """Corpus B: thousands of matches share the K-th weight and their weight bounds are exact, so the threshold of the pruning in front
    of the hit pass climbs to the K-th weight and its second level cuts inside the tied population.  Pruned == unpruned == bound by hits
    == bound by keywords == oracle."""
    m, ctx, batch = dev
    hi, _ = C.corpus_b(m)
    a, b, c = (C.kw(m, t, t + 1) for t in range(3))
    roots = [C.AND(m, C.OR(m, a, b), c), C.OR(m, a, b, c)]
    # (the field weights set the bins' width, and with it how coarse the rowid slices of the second level are)
    qs = [m.Query(r, ranker=rk, max_matches=k, field_weights=fw) for r in roots for rk in (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_PROXIMITY) for k in (10, 1000)
          for fw in (None, [3, 1], [-2, 5], [40, 40], [100, 60], [300, 200])]
    oi = orc_index_of(orc, hi)
    want = [to_orc(orc, q).run(oi) for q in qs]
    assert all(w.total_found > 20000 for w in want)
    for on in ({}, {"prox_prune": 0}, {"prox_bound_keywords": 1}, {"prox_bound_keywords": 1, "prox_prune": 0}):
        check(orc, dev, hi, qs, want=want, per_pass=1, on=on, off=on)


def test_reused_batch(orc, dev, corpus, oindex):
    """One batch: tree batches alternate with batches the kernel does not take -- field-limited keywords, a two-keyword BM25 AND (the
    two-bitmap AND kernel's), a five-keyword AND -- forwards and backwards; n_items_bt per submit."""
    m, ctx, batch = dev
    hi = corpus[0]
    named = [r for _, r in C.named_trees(m)]
    limited = C.OR(m, m.XQNode.keyword(0, 1, 1), m.XQNode.keyword(1, 2, 6))
    five = C.AND(m, *[C.kw(m, t, i + 1) for i, t in enumerate((0, 1, 2, 8, 9))])
    pair = C.AND(m, C.kw(m, 0, 1), C.kw(m, 1, 2))

    def Q(roots, rk, k=100):
        return [m.Query(r, ranker=rk, max_matches=k) for r in roots]

    sets = [Q(named, m.SPH_RANK_PROXIMITY_BM25), Q([limited, pair, five], m.SPH_RANK_BM25), Q(named[:3], m.SPH_RANK_NONE, 1), Q([pair], m.SPH_RANK_BM25),
            Q(named + [limited], m.SPH_RANK_BM25, 1000), Q([five, limited], m.SPH_RANK_PROXIMITY_BM25), Q(named[::-1], m.SPH_RANK_SPH04, 20)]
    n_bt = [sum(C.on_tree_kernel(m, q, docs_of(hi), C.N_DOCS) for q in qs) for qs in sets]
    assert [n > 0 for n in n_bt] == [True, False, True, False, True, False, True]
    seg = m.Segment(ctx, hi)
    try:
        want = [[to_orc(orc, q).run(oindex) for q in qs] for qs in sets]
        for order in (range(len(sets)), reversed(range(len(sets)))):
            for s in order:
                got = batch.search(seg, sets[s])
                assert batch.stats()["n_items_bt"] == 3 * n_bt[s], (s, batch.stats())
                for i, g in enumerate(got):
                    same(g, want[s][i], ("set", s, i))
    finally:
        seg.close()


def test_candidate_overflow_is_rerun(orc, dev):
    """Corpus C: every doc holds three keywords with one weight.  Under BM25 nothing prunes, the candidate list overflows and the query
    is rerun alone, on the tree kernel again; under SPH_RANK_NONE the bins are the rowid's and the query prunes."""
    m, ctx, batch = dev
    hi, rows = C.corpus_c(m)
    a, b, c = (C.kw(m, t, t + 1) for t in range(3))
    roots = [C.OR(m, a, b, c), C.AND(m, C.OR(m, a, b), c)]
    qs = [m.Query(r, ranker=m.SPH_RANK_BM25, max_matches=100) for r in roots] + [m.Query(r, ranker=m.SPH_RANK_NONE, max_matches=50) for r in roots]
    oi = orc_index_of(orc, hi)
    seg = m.Segment(ctx, hi)
    try:
        per_pass = (C.C_DOCS + C.WINDOW - 1) // C.WINDOW // C.ITEM_WINDOWS + 1  # 635 windows in items of 64
        got_on, got_off, st = on_and_off(dev, seg, qs, per_pass=per_pass)
        assert st["n_rerun"] >= 1 and batch.stats()["n_rerun"] >= 1, st
        for i, q in enumerate(qs):
            total, rowid, weight = C.model(m, q, rows, C.C_DOCS)
            assert got_on[i].total_found == total == C.C_DOCS and got_on[i].rowid.tolist() == list(range(q.max_matches)) == rowid.tolist(), i
            same(got_on[i], got_off[i], ("tree kernel vs bt_cover_inv=0", i))
            if i < 2:
                same(got_on[i], to_orc(orc, q).run(oi), ("tree kernel vs oracle", i))
            else:
                assert np.array_equal(got_on[i].weight, weight)
    finally:
        seg.close()
