"""GPU: the two-bitmap AND kernel's per-word weight bound (ctx key bm_wmax) against the kernel without it and the oracle.

With bm_wmax=1 a segment carries one nibble per 32-rowid bitmap word and keyword, the largest tf among the keyword's postings
in the word (capped at 15), and scan_bm_kernel drops a match word -- counted, never unpacked, no tf / field bytes fetched --
when the best weight its two nibbles allow lies behind the query's pruning threshold.  Results must not move: every check is
bit-exact on status, total_found, rowids and weights, bm_wmax=1 against bm_wmax=0 against the oracle.  The counters
bm_words_queued / bm_words_pruned (Batch.stats()) show that the bound fired where it must, and nowhere it must not."""
import numpy as np
import pytest

from helpers import synth_postings
from test_gpu_parity import kw, orc_index_of, to_orc

pytestmark = pytest.mark.gpu

# keywords 0 and 1 sit in more than half of the docs: their idf is negative
PROBS = [0.6, 0.55, 0.45, 0.3, 0.25, 0.2, 0.12, 0.08, 0.05, 0.03]
N_DOCS = 150001  # no multiple of the 2048-rowid window
FAT = 3          # the keyword with 300-hit docs (the 255-tf escape)
# planted rows (keywords 6 and 7, all three fields): the best row of the pair sits in a bitmap word that also holds tf-1
# postings of both keywords; ROW_15 / ROW_255 carry a tf in class 15 / beyond the packed byte
ROW_BEST, ROW_15, ROW_255 = 70003, 100_010, 131_080


def plant(W, R, H, term, row, tf, n_fields=3):
    keep = ~((W == term + 1) & (R == row))
    W, R, H = W[keep], R[keep], H[keep]
    pos = np.arange(1, tf + 1, dtype=np.uint32)
    hp = ((pos % n_fields).astype(np.uint32) << 24) | pos
    return np.concatenate([W, np.full(tf, term + 1, np.uint64)]), np.concatenate([R, np.full(tf, row, np.uint32)]), np.concatenate([H, hp])


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 64)
    yield m, ctx, batch
    batch.close()
    ctx.close()


@pytest.fixture(scope="module")
def corpus(dev):
    m, ctx, batch = dev
    rng = np.random.default_rng(8192)
    W, R, H = synth_postings(rng, N_DOCS, PROBS, n_fields=3, max_pos=40)
    fat = rng.choice(N_DOCS, 30, replace=False).astype(np.uint32)
    for r in fat:
        W, R, H = plant(W, R, H, FAT, int(r), 300)
    for t in (6, 7):
        W, R, H = plant(W, R, H, t, ROW_BEST, 12)
        for d in (-2, -1, 1, 2):  # (70003 & 31 == 19: the neighbours share its word)
            W, R, H = plant(W, R, H, t, ROW_BEST + d, 1)
        W, R, H = plant(W, R, H, t, ROW_15, 40)
        W, R, H = plant(W, R, H, t, ROW_255, 300)
    o = np.lexsort((H, R, W))
    return m.index_from_hits(W[o], R[o], H[o], n_terms=len(PROBS), total_docs=N_DOCS, n_fields=3)


def AND(m, a, b, ranker=None, mask=(0xFFFFFFFF, 0xFFFFFFFF), k=1000, fw=None, iw=1):
    return m.Query(m.XQNode.AND(kw(m, a, 1, mask[0]), kw(m, b, 2, mask[1])), ranker=ranker if ranker is not None else m.SPH_RANK_BM25,
                   max_matches=k, field_weights=fw, index_weight=iw)


def grouped(m, k, fw=None, iw=1):
    """Groups of 4, 3, 2 and 1 (test_gpu_bm_group.sized_groups): keyword 0 -- negative idf -- in seven queries; (1, 0): both negative;
    the pair (2, 3) as given and swapped; (4, 5) alone."""
    pairs = [(0, 1), (0, 2), (0, 3), (0, 5), (0, 6), (0, 7), (0, 8), (2, 3), (3, 2), (4, 5)]
    return [AND(m, a, b, k=k, fw=fw, iw=iw) for a, b in pairs]


def same(a, b, what):
    assert a.status == getattr(b, "status", 0) == 0, (what, a.status, getattr(b, "status", 0))  # (the oracle's results carry none)
    assert a.total_found == b.total_found, (what, a.total_found, b.total_found)
    assert np.array_equal(a.rowid, b.rowid), (what, a.rowid[:8], b.rowid[:8])
    assert np.array_equal(a.weight, b.weight), (what, a.weight[:8], b.weight[:8])


class Pair:
    """The same index as a segment with the plane and as one without."""

    def __init__(self, dev, hi, rowid_base=0, dead=None):
        m, ctx, batch = dev
        self.on = m.Segment(ctx, hi, rowid_base=rowid_base)
        ctx.set("bm_wmax", 0)
        try:
            self.off = m.Segment(ctx, hi, rowid_base=rowid_base)
        finally:
            ctx.set("bm_wmax", 1)
        if dead is not None:
            self.on.set_dead_rows(dead)
            self.off.set_dead_rows(dead)
        assert self.on.device_bytes > self.off.device_bytes

    def close(self):
        self.on.close()
        self.off.close()


def run(dev, pair, qs, want):
    """qs on both segments against `want`; returns the stats with the plane.  Without it both counters stay 0."""
    m, ctx, batch = dev
    got = batch.search(pair.on, qs)
    st = batch.stats()
    assert st["n_items_bm"] > 0
    ref = batch.search(pair.off, qs)
    st0 = batch.stats()
    assert st0["bm_words_queued"] == 0 and st0["bm_words_pruned"] == 0, st0
    for i in range(len(qs)):
        same(ref[i], want[i], ("bm_wmax=0 vs oracle", i))
        same(got[i], want[i], ("bm_wmax=1 vs oracle", i))
    return st


def oracle(orc, oi, qs):
    return [to_orc(orc, q).run(oi) for q in qs]


@pytest.fixture(scope="module")
def plain(orc, dev, corpus):
    pair = Pair(dev, corpus)
    yield pair, orc_index_of(orc, corpus)
    pair.close()


@pytest.mark.parametrize("k", [3, 100, 1000])
def test_groups_of_one_to_four(orc, dev, plain, k):
    m, ctx, batch = dev
    pair, oi = plain
    qs = grouped(m, k)
    batch.search(pair.on, qs)
    assert batch.stats()["n_bm_groups"] == [1, 1, 1, 1]
    st = run(dev, pair, qs, oracle(orc, oi, qs))
    assert st["bm_words_queued"] > 0
    if k < 1000:
        assert st["bm_words_pruned"] > 0, st


@pytest.mark.parametrize("fw,iw", [([3, 1, 2], 1), ([1, 5, 1], 1), (None, 2), ([1, 5, 1], 2)])
def test_field_weights_and_index_weight(orc, dev, plain, fw, iw):
    m, ctx, batch = dev
    pair, oi = plain
    qs = grouped(m, 3, fw, iw) + grouped(m, 100, fw, iw)
    st = run(dev, pair, qs, oracle(orc, oi, qs))
    assert st["bm_words_pruned"] > 0, st


def test_more_room_than_matches_prunes_nothing(orc, dev, plain):
    """About 225 docs hold keywords 8 and 9, and K is 1000: no threshold ever forms, no word may be dropped."""
    m, ctx, batch = dev
    pair, oi = plain
    qs = [AND(m, 8, 9), AND(m, 9, 8), AND(m, 7, 9, fw=[1, 5, 1])]
    want = oracle(orc, oi, qs)
    assert all(w.total_found < 1000 for w in want)
    st = run(dev, pair, qs, want)
    assert st["bm_words_pruned"] == 0 and st["bm_words_queued"] > 0, st


def test_planted_rows_lead(orc, dev, plain):
    """The best rows of (6, 7) are the planted ones: tf 300 (the escape), tf 40 (class 15), and tf 12 in a word whose other
    postings have tf 1 -- the word's class is its largest tf, not its first or last posting's."""
    m, ctx, batch = dev
    pair, oi = plain
    qs = [AND(m, 6, 7, k=3), AND(m, 7, 6, k=3, fw=[3, 1, 2]), AND(m, 6, 7, k=100), AND(m, FAT, 6, k=3), AND(m, FAT, 0, k=3), AND(m, 1, FAT, k=100)]
    want = oracle(orc, oi, qs)
    assert list(want[0].rowid) == [ROW_255, ROW_15, ROW_BEST]
    st = run(dev, pair, qs, want)
    assert st["bm_words_pruned"] > 0, st


def test_field_limits_and_rank_none_keep_the_old_path(orc, dev, plain):
    m, ctx, batch = dev
    pair, oi = plain
    qs = [AND(m, 0, 2, k=3, mask=(1, 0xFFFFFFFF)), AND(m, 2, 3, k=3, mask=(0xFFFFFFFF, 6)), AND(m, 4, 5, k=100, mask=(3, 5)),
          AND(m, 0, 2, k=3, ranker=m.SPH_RANK_NONE), AND(m, 2, 3, k=100, ranker=m.SPH_RANK_NONE)]
    st = run(dev, pair, qs, oracle(orc, oi, qs))
    assert st["bm_words_pruned"] == 0 and st["bm_words_queued"] == 0, st


@pytest.mark.parametrize("iw", [-1, -2])
def test_negative_index_weight_keeps_the_old_path(orc, dev, plain, iw):
    """Multiplying by a negative index_weight turns the order round: an upper bound of the tfidf sum bounds nothing, so such a
    query is not eligible.  The best rows are the ones with the LOWEST sums -- exactly the words a bound would drop."""
    m, ctx, batch = dev
    pair, oi = plain
    qs = grouped(m, 3, iw=iw) + grouped(m, 100, fw=[3, 1, 2], iw=iw) + [AND(m, 6, 7, k=3, iw=iw)]
    want = oracle(orc, oi, qs)
    assert all(w.weight[0] < 0 for w in want)
    st = run(dev, pair, qs, want)
    assert st["bm_words_pruned"] == 0 and st["bm_words_queued"] == 0, st


def test_dead_rows(orc, dev, corpus):
    m, ctx, batch = dev
    rng = np.random.default_rng(2)
    dead = np.zeros((N_DOCS + 31) // 32, np.uint32)
    killed = np.concatenate([rng.choice(N_DOCS, size=N_DOCS // 5, replace=False), [ROW_255]])
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    pair = Pair(dev, corpus, dead=dead)
    oi = orc_index_of(orc, corpus)
    oi.dead_rows = dead
    try:
        qs = grouped(m, 3) + grouped(m, 100, fw=[3, 1, 2]) + [AND(m, 6, 7, k=3)]
        st = run(dev, pair, qs, oracle(orc, oi, qs))
        assert st["bm_words_pruned"] > 0, st
    finally:
        pair.close()


def test_rowid_base(orc, dev, corpus):
    m, ctx, batch = dev
    pair = Pair(dev, corpus, rowid_base=3 * 65536 + 17)
    try:
        qs = grouped(m, 3) + grouped(m, 1000) + [AND(m, 6, 7, k=3)]
        st = run(dev, pair, qs, oracle(orc, orc_index_of(orc, corpus), qs))
        assert st["bm_words_pruned"] > 0, st
    finally:
        pair.close()


def test_nibble_plane_instance(orc, dev, corpus):
    """attr_nibbles: the segment gathers from the one-byte plane, the kernel's non-SEQ instance."""
    m, ctx, batch = dev
    ctx.set("attr_nibbles", 1)
    try:
        pair = Pair(dev, corpus)
    finally:
        ctx.set("attr_nibbles", 0)
    try:
        qs = grouped(m, 3) + grouped(m, 100, fw=[1, 5, 1], iw=2) + [AND(m, 6, 7, k=3), AND(m, FAT, 6, k=3)]
        st = run(dev, pair, qs, oracle(orc, orc_index_of(orc, corpus), qs))
        assert st["bm_words_pruned"] > 0, st
    finally:
        pair.close()


def test_ungrouped_layout(orc, dev, plain):
    """bm_group=0: the kernel's other two instances, a workgroup per query."""
    m, ctx, batch = dev
    pair, oi = plain
    qs = grouped(m, 3) + grouped(m, 100)
    ctx.set("bm_group", 0)
    try:
        st = run(dev, pair, qs, oracle(orc, oi, qs))
    finally:
        ctx.set("bm_group", 1)
    assert st["n_bm_groups"] == [0, 0, 0, 0] and st["bm_words_pruned"] > 0, st


def test_one_batch_across_submits(orc, dev, plain):
    m, ctx, batch = dev
    pair, oi = plain
    sets = [grouped(m, 3), [AND(m, 8, 9)], grouped(m, 100, fw=[3, 1, 2]), [AND(m, 0, 2, k=3, ranker=m.SPH_RANK_NONE), AND(m, 6, 7, k=3)]]
    want = [oracle(orc, oi, qs) for qs in sets]
    pruned = []
    for order in (range(len(sets)), reversed(range(len(sets)))):
        for s in order:
            pruned.append((s, run(dev, pair, sets[s], want[s])["bm_words_pruned"]))
    assert all(p == 0 for s, p in pruned if s == 1) and all(p > 0 for s, p in pruned if s != 1), pruned


def test_candidate_overflow_is_rerun(orc, dev):
    """1.2 M docs tie at the best weight (tf 2 of both keywords), more than a candidate list holds: the queries overflow and are
    rerun alone; the 100 000 docs with tf 1 lie behind the threshold, in words of their own.  (The keywords sit in a quarter of
    the docs: their idf is positive, and large enough for tf 1 and tf 2 to fall in different bins.)"""
    m, ctx, batch = dev
    n_docs, n_held, n_top = 5_200_000, 1_300_000, 1_200_000
    rows = np.arange(n_held, dtype=np.uint32)
    W, R, H = [], [], []
    for t in range(2):
        for pos in (1, 2):
            r = rows if pos == 1 else rows[:n_top]
            W.append(np.full(r.size, t + 1, np.uint64)), R.append(r), H.append(np.full(r.size, (t << 24) | (2 * t + pos), np.uint32))  # (keyword t in field t: a match holds both fields, the bound's field-weight sum)
    W, R, H = np.concatenate(W), np.concatenate(R), np.concatenate(H)
    o = np.lexsort((H, R, W))
    hi = m.index_from_hits(W[o], R[o], H[o], n_terms=2, total_docs=n_docs, n_fields=2)
    qs = [AND(m, 0, 1), AND(m, 1, 0, k=10)]
    pair = Pair(dev, hi)
    try:
        want = oracle(orc, orc_index_of(orc, hi), qs)
        assert want[0].total_found == n_held and list(want[0].rowid) == list(range(1000))
        st = run(dev, pair, qs, want)
        assert st["n_rerun"] == 2 and st["bm_words_pruned"] > 0, st
    finally:
        pair.close()
