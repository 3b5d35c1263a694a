"""CPU: the corpora of the tree kernel's suite (bt_edges_common.py) hold what they claim, and the oracle agrees with the numpy model
on them -- total_found for every tree of test_gpu_bt_edges.py, the rows under SPH_RANK_NONE -- before any device is asked."""
import numpy as np
import pytest

import bt_edges_common as C
from test_gpu_parity import orc_index_of, to_orc


@pytest.fixture(scope="module")
def m():
    import manticoresearch_amd

    return manticoresearch_amd


@pytest.fixture(scope="module")
def corpus(m):
    return C.corpus_a(m)


def test_corpus_a_structure(m, corpus):
    hi, rows, classes = corpus
    docs = [int(x) for x in hi.dict["docs"]]
    assert C.N_DOCS == 272385 and C.N_WINDOWS == 134
    # dense and sparse classes (corpus_a asserts them too)
    assert all(docs[t] >= C.DENSE_MIN for t in (0, 1, 2, 8, 9)), docs
    assert all(0 < docs[t] < C.N_DOCS // 64 for t in (3, 4, 5, 6)) and docs[7] == 0, docs
    # edges
    assert np.isin(C.EDGE_ROWIDS, rows[3]).all()
    full = np.arange(C.FULL_STEP * C.STEP, (C.FULL_STEP + 1) * C.STEP)
    assert np.isin(full, rows[1]).all() and np.isin(full, rows[2]).all()
    assert rows[1][-1] == rows[2][-1] == rows[3][-1] == rows[6][0] == C.N_DOCS - 1 and rows[6].size == 1
    # keyword 5: its first 128-doc block ends on a step's last rowid, the next one begins on the following step's first
    assert rows[5].size == 256 and rows[5][127] == 17 * C.STEP - 1 and rows[5][128] == 17 * C.STEP
    # keyword 4: 31 whole blocks inside one step
    assert rows[4].size == 4000 and rows[4][0] // C.STEP == rows[4][31 * 128 - 1] // C.STEP == 5 and rows[4].size // 128 >= 31
    # tf >= 255 on a dense and on a sparse keyword
    hits = [int(x) for x in hi.dict["hits"]]
    assert rows[1][::C.FAT_EVERY].size >= 30 and rows[3][::C.FAT_EVERY].size == 2
    assert hits[1] > 300 * rows[1][::C.FAT_EVERY].size and hits[3] > 300 * 2
    # the phrase pair's common docs
    both = np.intersect1d(rows[8], rows[9])
    assert both.size == C.PH_COMMON == sum(classes[k].size for k in ("accept", "reject_field", "reject_gap", "reversed", "multi_with", "multi_without"))


def test_item_geometry():
    """134 = 64 + 64 + 6: two items of 16 windows = 4 whole steps per wave, one of 2 windows per wave for waves 0-2 and none for wave 3."""
    ranges = C.item_ranges()
    assert [r for r, _ in ranges] == [(0, 64), (64, 128), (128, 134)]
    assert ranges[0][1] == [(0, 16), (16, 32), (32, 48), (48, 64)]
    assert ranges[2][1] == [(128, 130), (130, 132), (132, 134), (134, 134)]
    assert ranges[2][1][1][0] % 4 == 2 and (6 // 4) * 4 != 6 and (C.N_DOCS - 1) // C.WINDOW == 133 and (C.N_DOCS - 1) % C.WINDOW == 0


def all_tree_queries(m):
    """Every boolean tree test_gpu_bt_edges.py asks of corpus A, under SPH_RANK_NONE, K = 1000."""
    roots = [r for _, r in C.named_trees(m)] + [r for _, r in C.full_step_trees(m)] + C.random_trees(m, 100)
    return [m.Query(r, ranker=m.SPH_RANK_NONE, max_matches=1000, index_weight=1 + 2 * (i % 2)) for i, r in enumerate(roots)]


def same_as_model(m, orc, oi, qs, rows, n_docs, dead=None):
    oi.dead_rows = dead
    try:
        for i, q in enumerate(qs):
            want = to_orc(orc, q).run(oi)
            total, rowid, weight = C.model(m, q, rows, n_docs, dead)
            assert want.total_found == total, (i, want.total_found, total)
            assert np.array_equal(want.rowid, rowid) and np.array_equal(want.weight, weight), (i, want.rowid[:8], rowid[:8])
    finally:
        oi.dead_rows = None


def test_oracle_equals_model_on_corpus_a(m, orc, corpus):
    hi, rows, _ = corpus
    oi = orc_index_of(orc, hi)
    qs = all_tree_queries(m)
    same_as_model(m, orc, oi, qs, rows, C.N_DOCS)
    rng = np.random.default_rng(3)
    killed = np.union1d(rng.choice(C.N_DOCS, C.N_DOCS // 5, replace=False), C.EDGE_ROWIDS)
    same_as_model(m, orc, oi, qs, rows, C.N_DOCS, C.dead_words(C.N_DOCS, killed))
    full = np.arange(C.FULL_STEP * C.STEP, (C.FULL_STEP + 1) * C.STEP)
    same_as_model(m, orc, oi, qs[:30], rows, C.N_DOCS, C.dead_words(C.N_DOCS, full))
    # totals under a weighing ranker
    for q in qs[:24]:
        q2 = m.Query(q.root, ranker=m.SPH_RANK_BM25, max_matches=20)
        assert to_orc(orc, q2).run(oi).total_found == C.model(m, q2, rows, C.N_DOCS)[0]


def test_phrase_candidates_of_every_kind(m, orc, corpus):
    """'"8 9"' matches the accepted lone-hit docs and the multi-hit docs with an occurrence; '"9 8"' the reversed ones."""
    hi, rows, classes = corpus
    oi = orc_index_of(orc, hi)
    a, b = C.kw(m, 8, 1), C.kw(m, 9, 2)
    r89 = to_orc(orc, m.Query(C.PHRASE(m, a, b), ranker=m.SPH_RANK_BM25, max_matches=10)).run(oi)
    assert r89.total_found == C.PH_ACCEPT + C.PH_MULTI_WITH
    r98 = to_orc(orc, m.Query(C.PHRASE(m, C.kw(m, 9, 1), C.kw(m, 8, 2)), ranker=m.SPH_RANK_BM25, max_matches=10)).run(oi)
    assert r98.total_found == C.PH_REVERSED
    assert 0 < r98.total_found < r89.total_found < C.PH_COMMON


@pytest.mark.parametrize("k", [10, 1000])
def test_corpus_b_ties_at_the_kth_weight(m, orc, k):
    hi, rows = C.corpus_b(m)
    oi = orc_index_of(orc, hi)
    a, b, c = (C.kw(m, t, t + 1) for t in range(3))
    for ranker in (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_PROXIMITY):
        for root in (C.AND(m, C.OR(m, a, b), c), C.OR(m, a, b, c)):
            r = to_orc(orc, m.Query(root, ranker=ranker, max_matches=C.B_DOCS)).run(oi)
            assert r.total_found > 20000 and r.rowid.size == r.total_found
            assert int((r.weight == r.weight[k - 1]).sum()) >= 4 * k, (ranker, k, int((r.weight == r.weight[k - 1]).sum()))


def test_oracle_equals_model_on_corpora_b_and_c(m, orc):
    a, b, c = (C.kw(m, t, t + 1) for t in range(3))
    roots = (C.OR(m, a, b, c), C.AND(m, C.OR(m, a, b), c))
    hi, rows = C.corpus_b(m)
    same_as_model(m, orc, orc_index_of(orc, hi), [m.Query(r, ranker=m.SPH_RANK_NONE, max_matches=k) for r in roots for k in (10, 1000)], rows, C.B_DOCS)
    hi, rows = C.corpus_c(m)
    qs = [m.Query(r, ranker=m.SPH_RANK_NONE, max_matches=50) for r in roots]
    same_as_model(m, orc, orc_index_of(orc, hi), qs, rows, C.C_DOCS)
    for q in qs:
        total, rowid, weight = C.model(m, q, rows, C.C_DOCS)
        assert total == C.C_DOCS and rowid.tolist() == list(range(50)) and weight.tolist() == [1] * 50
