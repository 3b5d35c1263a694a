"""GPU: the two-bitmap AND kernel's burst pipeline against the oracle and a bm_wmax=0 segment.

scan_bm_kernel keeps the next burst of four windows in flight while it works the current one: bitmap, dead-row and tf-class words
and the threshold poll are requested a burst ahead and taken over at the loop top.  Results must not move: every check is bit-exact
on status, total_found, rowids and weights, bm_wmax=1 against bm_wmax=0 against the oracle.

Segments of 33, 37, 41, 45 and 47 windows (the last one not full) at bm_min_windows=16 leave a last work item of 1, 5, 9, 13 and 15
windows, i.e. wave shares of 0 to 4 windows and bursts that start off a multiple of four (their classes reach into the next group of
four windows): the pipeline's prologue and epilogue alone.  A segment of 150 windows at bm_min_windows=64 gives every wave several
bursts; with a small k the threshold moves while the waves run -- it now reaches a wave one burst later -- and words are dropped."""
import numpy as np
import pytest

from helpers import synth_postings
from test_gpu_parity import orc_index_of
from test_gpu_bm_wmax import PROBS, AND, Pair, grouped, oracle, run

pytestmark = pytest.mark.gpu

SHORT = [33, 37, 41, 45, 47]
LONG = 150


def docs_of(windows):
    return (windows - 1) * 2048 + 777  # the last window is not full


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 64)
    yield m, ctx, batch
    batch.close()
    ctx.close()


@pytest.fixture(scope="module")
def corpora(orc, dev):
    """windows -> (host index, oracle index), built once.  One synthetic corpus of 47 windows serves them all (synth_postings takes
    seconds per 100 K docs): a short segment is its first rows, the long one four copies of it 47 windows apart, cut at 150."""
    m, ctx, batch = dev
    top = max(SHORT)
    W0, R0, H0 = synth_postings(np.random.default_rng(4747), docs_of(top), PROBS, n_fields=3, max_pos=40)
    out = {}
    for w in SHORT + [LONG]:
        n = docs_of(w)
        copies = -(-w // top)
        W, H = np.tile(W0, copies), np.tile(H0, copies)
        R = np.concatenate([R0 + np.uint32(c * top * 2048) for c in range(copies)])
        keep = R < n
        W, R, H = W[keep], R[keep], H[keep]
        o = np.lexsort((H, R, W))
        hi = m.index_from_hits(W[o], R[o], H[o], n_terms=len(PROBS), total_docs=n, n_fields=3)
        out[w] = (hi, orc_index_of(orc, hi))
    return out


def queries(m, ks):
    """groups of 4, 3, 2 and 1 per k; then SPH_RANK_NONE and a field-limited query, which stay off the bound's path"""
    qs = []
    for k in ks:
        qs += grouped(m, k)
    return qs + [AND(m, 0, 2, k=10, ranker=m.SPH_RANK_NONE), AND(m, 2, 3, k=10, mask=(0xFFFFFFFF, 6))]


def dead_rows(n_docs, seed):
    rng = np.random.default_rng(seed)
    dead = np.zeros((n_docs + 31) // 32, np.uint32)
    killed = rng.choice(n_docs, size=n_docs // 5, replace=False)
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    return dead


@pytest.mark.parametrize("windows", SHORT)
def test_prologue_and_epilogue(orc, dev, corpora, windows):
    m, ctx, batch = dev
    hi, oi = corpora[windows]
    ctx.set("bm_min_windows", 16)
    pair = Pair(dev, hi)
    try:
        qs = queries(m, (10, 1000))
        st = run(dev, pair, qs, oracle(orc, oi, qs))
        assert st["bm_words_queued"] > 0, st
    finally:
        pair.close()
        ctx.set("bm_min_windows", 256)


@pytest.fixture(scope="module")
def long_pair(dev, corpora):
    m, ctx, batch = dev
    ctx.set("bm_min_windows", 64)
    pair = Pair(dev, corpora[LONG][0])
    yield pair
    pair.close()
    ctx.set("bm_min_windows", 256)


@pytest.mark.parametrize("k", [10, 50, 1000])
def test_many_bursts(orc, dev, corpora, long_pair, k):
    m, ctx, batch = dev
    ctx.set("bm_min_windows", 64)
    qs = queries(m, (k,))
    batch.search(long_pair.on, qs[:10])
    assert batch.stats()["n_bm_groups"] == [1, 1, 1, 1]
    st = run(dev, long_pair, qs, oracle(orc, corpora[LONG][1], qs))
    assert st["bm_words_queued"] > 0, st
    if k == 10:
        assert st["bm_words_pruned"] > 0, st


def test_off_the_bounds_path(orc, dev, corpora, long_pair):
    """SPH_RANK_NONE and field limits do not take the bound's path: the pipeline serves them, the counters stay 0"""
    m, ctx, batch = dev
    ctx.set("bm_min_windows", 64)
    qs = [AND(m, 0, 2, k=10, ranker=m.SPH_RANK_NONE), AND(m, 2, 3, k=50, ranker=m.SPH_RANK_NONE), AND(m, 2, 3, k=10, mask=(0xFFFFFFFF, 6)), AND(m, 0, 1, k=10, mask=(1, 3))]
    st = run(dev, long_pair, qs, oracle(orc, corpora[LONG][1], qs))
    assert st["bm_words_pruned"] == 0 and st["bm_words_queued"] == 0, st


def test_dead_rows(orc, dev, corpora):
    m, ctx, batch = dev
    hi = corpora[LONG][0]
    dead = dead_rows(docs_of(LONG), 3)
    ctx.set("bm_min_windows", 64)
    pair = Pair(dev, hi, dead=dead)
    oi = orc_index_of(orc, hi)
    oi.dead_rows = dead
    try:
        qs = queries(m, (10, 1000))
        st = run(dev, pair, qs, oracle(orc, oi, qs))
        assert st["bm_words_pruned"] > 0, st
    finally:
        pair.close()
        ctx.set("bm_min_windows", 256)


def test_dead_rows_short(orc, dev, corpora):
    m, ctx, batch = dev
    hi = corpora[45][0]
    dead = dead_rows(docs_of(45), 4)
    ctx.set("bm_min_windows", 16)
    pair = Pair(dev, hi, dead=dead)
    oi = orc_index_of(orc, hi)
    oi.dead_rows = dead
    try:
        qs = queries(m, (10,))
        run(dev, pair, qs, oracle(orc, oi, qs))
    finally:
        pair.close()
        ctx.set("bm_min_windows", 256)


def test_rowid_base(orc, dev, corpora):
    m, ctx, batch = dev
    hi, oi = corpora[LONG]
    ctx.set("bm_min_windows", 64)
    pair = Pair(dev, hi, rowid_base=5 * 65536 + 33)
    try:
        qs = queries(m, (10, 50))
        st = run(dev, pair, qs, oracle(orc, oi, qs))
        assert st["bm_words_pruned"] > 0, st
    finally:
        pair.close()
        ctx.set("bm_min_windows", 256)


@pytest.mark.parametrize("windows,minw", [(41, 16), (LONG, 64)])
def test_without_the_slot_ordered_plane(orc, dev, corpora, windows, minw):
    """attr_seq=0: the kernel's non-SEQ instances"""
    m, ctx, batch = dev
    hi, oi = corpora[windows]
    ctx.set("bm_min_windows", minw)
    ctx.set("attr_seq", 0)
    try:
        pair = Pair(dev, hi)
    finally:
        ctx.set("attr_seq", 1)
    try:
        qs = queries(m, (10, 1000))
        st = run(dev, pair, qs, oracle(orc, oi, qs))
        assert st["bm_words_queued"] > 0, st
    finally:
        pair.close()
        ctx.set("bm_min_windows", 256)
