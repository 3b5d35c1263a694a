"""GPU: the lean block-scan instance (ctx key pair_scan, scan_p2_kernel) against the generic one (pair_scan=0) and the oracle.

With pair_scan=1 a batch of plain one- and two-keyword queries (NONE / BM25 / single-keyword PROXIMITY, no trees, filters or
sort, a segment of <= 8 fields packed with bitmaps on) runs its block-scan work items on the lean kernel; stats()["pk_lean"]
says which instance ran.  Every check is bit-exact on status, total_found, rowids and weights.  The corpus holds the keyword
densities at which the kernel takes another path: dense keywords probed through their bitmap (0.3, 0.05, one just above
1/64), the densest block-probed keyword (just below 1/64), keywords of several blocks with a partial last one, one partial
block, one doc, and a keyword whose tf saturates the packed byte."""
import numpy as np
import pytest

from test_gpu_parity import kw, orc_index_of, to_orc

pytestmark = pytest.mark.gpu

N_DOCS = 300001  # no multiple of the 2048-rowid window or of the 128-doc block
DENSE_MIN = (N_DOCS + 63) // 64  # docs * 64 >= total docs: the keyword gets a bitmap
# keyword -> docs: 0.3, 0.05, just above / below 1/64, 2e-3 (4 blocks + 88), 1e-3 (2 blocks + 44), 1e-4 (one partial block), one doc
COUNTS = [90000, 15000, DENSE_MIN, DENSE_MIN - 1, 600, 300, 30, 1]
K_FAT = len(COUNTS)  # keyword 8: 30 docs of 300 hits each
DEFAULT_ITEM_BYTES = 128 << 10


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 128)
    yield m, ctx, batch
    batch.close()
    ctx.close()


def make_corpus(m):
    rng = np.random.default_rng(2048)
    rows = [np.sort(rng.choice(N_DOCS, c, replace=False)).astype(np.uint32) for c in COUNTS[:5]]

    def part(src, n, total):
        """n rows of src and total - n others: the sparse keywords meet each other often enough to match"""
        a = rng.choice(src, n, replace=False)
        rest = np.setdiff1d(np.arange(N_DOCS, dtype=np.uint32), a)
        return np.sort(np.concatenate([a, rng.choice(rest, total - n, replace=False)])).astype(np.uint32)

    rows[3] = part(rows[4], 150, COUNTS[3])
    rows.append(part(rows[4], 150, COUNTS[5]))
    rows.append(part(np.intersect1d(rows[4], rows[5]), 12, COUNTS[6]))
    rows.append(rows[4][17:18].copy())
    rows.append(part(rows[4], 12, 30))
    W, R, H = [], [], []
    for t, rw in enumerate(rows):
        if t == K_FAT:  # 300 hits in field 1: the tf saturates the packed byte (the 255-tf escape)
            W.append(np.full(rw.size * 300, t + 1, np.uint64))
            R.append(np.repeat(rw, 300))
            H.append(np.tile((np.uint32(1) << 24) | np.arange(1, 301, dtype=np.uint32), rw.size))
            continue
        tf = 1 + np.minimum(254, rng.geometric(0.5, rw.size) - 1)
        n = int(tf.sum())
        W.append(np.full(n, t + 1, np.uint64))
        R.append(np.repeat(rw, tf))
        H.append(((rng.integers(0, 3, n).astype(np.uint32)) << 24) | rng.integers(1, 41, n).astype(np.uint32))
    W, R, H = np.concatenate(W), np.concatenate(R), np.concatenate(H)
    o = np.lexsort((H, R, W))
    W, R, H = W[o], R[o], H[o]
    keep = np.ones(W.size, bool)
    keep[1:] = (W[1:] != W[:-1]) | (R[1:] != R[:-1]) | (H[1:] != H[:-1])
    hi = m.index_from_hits(W[keep], R[keep], H[keep], n_terms=len(rows), total_docs=N_DOCS, n_fields=3)
    assert [int(x) for x in hi.dict["docs"]] == COUNTS + [30]
    return hi


@pytest.fixture(scope="module")
def corpus(dev):
    return make_corpus(dev[0])


@pytest.fixture(scope="module")
def oindex(orc, corpus):
    return orc_index_of(orc, corpus)


def AND(m, a, b, ranker=None, mask=(0xFFFFFFFF, 0xFFFFFFFF), k=1000, fw=None, iw=1):
    return m.Query(m.XQNode.AND(kw(m, a, 1, mask[0]), kw(m, b, 2, mask[1])), ranker=ranker if ranker is not None else m.SPH_RANK_BM25,
                   max_matches=k, field_weights=fw, index_weight=iw)


def ONE(m, a, ranker=None, mask=0xFFFFFFFF, k=1000, fw=None, iw=1):
    return m.Query(kw(m, a, 1, mask), ranker=ranker if ranker is not None else m.SPH_RANK_BM25, max_matches=k, field_weights=fw, index_weight=iw)


SPARSE = [4, 5, 6, 7, 8]


def fixed(m):
    """sparse x dense (bitmap probe), sparse x sparse (block probe), the below-1/64 keyword as second term, every pair also
    swapped, single keywords of every density the block scan serves, both rankers, single-keyword PROXIMITY."""
    qs = []
    for s in SPARSE:
        for d in (0, 1, 2, 3):
            qs += [AND(m, s, d), AND(m, d, s, ranker=m.SPH_RANK_NONE)]
    for a in SPARSE:
        for b in SPARSE:
            if a < b:
                qs += [AND(m, a, b), AND(m, b, a)]
    qs += [AND(m, 3, 2), AND(m, 3, 1), AND(m, 0, 3, k=100)]
    for t in (3, 4, 5, 6, 7, 8):
        qs += [ONE(m, t), ONE(m, t, ranker=m.SPH_RANK_NONE, k=3), ONE(m, t, ranker=m.SPH_RANK_PROXIMITY, fw=[3, 1, 2]),
               ONE(m, t, ranker=m.SPH_RANK_PROXIMITY_BM25, mask=5)]
    return qs


def mixed(m, rng, n):
    """Random pairs with a sparse driver: field limits on either keyword, field weights, index weights, K in {3, 100, 1000}."""
    qs = []
    fws = [None, [3, 1, 2], [1, 5, 1]]
    for _ in range(n):
        a = int(rng.choice([3, 4, 5, 6, 8]))
        b = int(rng.choice([x for x in range(9) if x != a]))
        if rng.random() < 0.5:
            a, b = b, a
        mask = tuple(0xFFFFFFFF if rng.random() < 0.6 else int(rng.integers(1, 8)) for _ in range(2))
        qs.append(AND(m, a, b, ranker=m.SPH_RANK_NONE if rng.random() < 0.3 else m.SPH_RANK_BM25, mask=mask,
                      k=int(rng.choice([3, 100, 1000])), fw=fws[int(rng.integers(0, 3))], iw=int(rng.choice([1, 2]))))
    return qs


def same(a, b, what):
    assert a.status == getattr(b, "status", 0) == 0, (what, a.status, getattr(b, "status", 0))  # (the oracle's results carry none)
    assert a.total_found == b.total_found, (what, a.total_found, b.total_found)
    assert np.array_equal(a.rowid, b.rowid), (what, a.rowid[:8], b.rowid[:8])
    assert np.array_equal(a.weight, b.weight), (what, a.weight[:8], b.weight[:8])


def run_both(dev, seg, qs):
    """The batch's answers with pair_scan=1 and with pair_scan=0; the stats say which instance the block items ran on."""
    m, ctx, batch = dev
    out = []
    try:
        for p in (1, 0):
            ctx.set("pair_scan", p)
            got = batch.search(seg, qs)
            st = batch.stats()
            assert st["packed"] == 1 and st["n_items"] > st["n_items_bm"]  # block-scan work items were launched ...
            assert st["pk_lean"] == p, st  # ... on the instance asked for
            out.append((got, st))
    finally:
        ctx.set("pair_scan", 1)
    return out


def check(orc, dev, hi, oi, qs, rowid_base=0, dead=None, want=None):
    m, ctx, batch = dev
    seg = m.Segment(ctx, hi, rowid_base=rowid_base)
    if dead is not None:
        seg.set_dead_rows(dead)
    oi.dead_rows = dead
    try:
        for i in range(0, len(qs), batch.max_queries):
            chunk = qs[i:i + batch.max_queries]
            (lean, _), (generic, _) = run_both(dev, seg, chunk)
            for j, q in enumerate(chunk):
                w = want[i + j] if want is not None else to_orc(orc, q).run(oi)
                same(lean[j], w, ("pair_scan=1 vs oracle", i + j))
                same(generic[j], w, ("pair_scan=0 vs oracle", i + j))
    finally:
        oi.dead_rows = None
        seg.close()


def test_densities_pairs_and_rankers(orc, dev, corpus, oindex):
    m = dev[0]
    check(orc, dev, corpus, oindex, fixed(m) + mixed(m, np.random.default_rng(1), 60))


def test_batch_of_one_and_of_128(orc, dev, corpus, oindex):
    m = dev[0]
    check(orc, dev, corpus, oindex, [AND(m, 5, 0)])
    check(orc, dev, corpus, oindex, [ONE(m, 7)])
    qs = mixed(m, np.random.default_rng(2), 128)
    assert len(qs) == dev[2].max_queries
    check(orc, dev, corpus, oindex, qs)


def test_item_sizes_one_block_and_many(orc, dev, corpus, oindex):
    """item_bytes=4096 cuts the items down to a block per wave.  A large item_bytes with pk_min_items=1 (no finer cut of a small
    batch) leaves one item per query: a wave walks a quarter of the driver's block list -- 176 blocks of the 0.3 keyword,
    past the 63 entries of one block-index chunk -- and the block-probed keyword's blocks one after the other."""
    m, ctx, batch = dev
    qs = fixed(m)[:40] + [ONE(m, 0, mask=3), ONE(m, 1, mask=3), ONE(m, 3), AND(m, 3, 1), AND(m, 3, 0, mask=(6, 5))] + mixed(m, np.random.default_rng(3), 40)
    want = [to_orc(orc, q).run(oindex) for q in qs]
    n_items = []
    try:
        for ib, cut in ((4096, 2048), (64 << 20, 1)):
            ctx.set("item_bytes", ib)
            ctx.set("pk_min_items", cut)
            check(orc, dev, corpus, oindex, qs, want=want)
            n_items.append(batch.stats()["n_items"])
    finally:
        ctx.set("item_bytes", DEFAULT_ITEM_BYTES)
        ctx.set("pk_min_items", 2048)
    assert n_items[0] > 4 * n_items[1]


def test_dead_rows_and_rowid_base(orc, dev, corpus, oindex):
    m = dev[0]
    rng = np.random.default_rng(4)
    dead = np.zeros((N_DOCS + 31) // 32, np.uint32)
    killed = rng.choice(N_DOCS, size=N_DOCS // 5, replace=False)
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    qs = fixed(m)[:50] + mixed(m, rng, 40)
    check(orc, dev, corpus, oindex, qs, dead=dead)
    check(orc, dev, corpus, oindex, qs, rowid_base=3 * 65536 + 17)


def test_reused_batch_alternating_instances(orc, dev, corpus, oindex):
    """One batch, submits that alternate between sets the lean instance takes and sets it must leave to the generic one (a
    third keyword, a hit ranker over two keywords, a tree), forwards and back."""
    m, ctx, batch = dev
    rng = np.random.default_rng(5)
    three = m.Query(m.XQNode.AND(kw(m, 4, 1), kw(m, 5, 2), kw(m, 0, 3)), ranker=m.SPH_RANK_BM25)
    tree = m.Query(m.XQNode(m.SPH_QUERY_OR, [kw(m, 4, 1), kw(m, 6, 2)]), ranker=m.SPH_RANK_BM25)
    sets = [(mixed(m, rng, 30), 1), ([AND(m, 4, 0), three], 0), ([ONE(m, 6)], 1), ([AND(m, 4, 5, ranker=m.SPH_RANK_PROXIMITY_BM25), AND(m, 5, 4)], 0),
            (fixed(m)[:60], 1), ([tree, AND(m, 5, 1)], 0), (mixed(m, rng, 90), 1)]
    seg = m.Segment(ctx, corpus)
    try:
        want = [[to_orc(orc, q).run(oindex) for q in qs] for qs, _ in sets]
        for order in (range(len(sets)), reversed(range(len(sets)))):
            for s in order:
                got = batch.search(seg, sets[s][0])
                assert batch.stats()["pk_lean"] == sets[s][1], (s, batch.stats())
                for i, g in enumerate(got):
                    same(g, want[s][i], ("set", s, i))
    finally:
        seg.close()


def test_candidate_overflow_is_rerun(orc, dev):
    """Every doc holds the keyword in field 1 with one weight: under BM25 nothing prunes, the candidate list (2^20 slots)
    overflows, and the query is rerun alone with a list that holds every doc -- on the lean instance again, 64 driver blocks
    per wave.  The field limit keeps the query on the block scan."""
    m, ctx, batch = dev
    n_docs = 1_300_000
    rows = np.arange(n_docs, dtype=np.uint32)
    W = np.concatenate([np.full(n_docs, 1, np.uint64), np.full(n_docs // 100, 2, np.uint64)])
    R = np.concatenate([rows, rows[::100][: n_docs // 100]])
    H = np.concatenate([np.full(n_docs, (1 << 24) | 1, np.uint32), np.full(n_docs // 100, (1 << 24) | 2, np.uint32)])
    o = np.lexsort((H, R, W))
    hi = m.index_from_hits(W[o], R[o], H[o], n_terms=2, total_docs=n_docs, n_fields=2)
    qs = [ONE(m, 0, mask=2), ONE(m, 0, mask=2, ranker=m.SPH_RANK_NONE, k=50), AND(m, 1, 0, k=100)]
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    try:
        (lean, st1), (generic, st0) = run_both(dev, seg, qs)
        # (the BM25 query overflows; the bins of SPH_RANK_NONE are the rowid's, so that query prunes and needs no rerun)
        assert st1["n_rerun"] >= 1 and st0["n_rerun"] >= 1, (st1, st0)
        for i, q in enumerate(qs):
            g = lean[i]
            if i < 2:
                assert g.total_found == n_docs and list(g.rowid) == list(range(q.max_matches)), i
            same(g, generic[i], ("pair_scan=1 vs pair_scan=0", i))
            if i != 1:
                same(g, to_orc(orc, q).run(oi), ("pair_scan=1 vs oracle", i))
    finally:
        seg.close()
