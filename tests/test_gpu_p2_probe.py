"""GPU: the lean block scan's probe of a SPARSE second keyword (scan_p2_kernel: every driver doc finds its own block in the
block-index chunk and its slot by a lower bound over the packed words) against the generic instance (pair_scan=0) and the oracle.

The context runs with bitmap_inv=1: no keyword of the corpus gets a bitmap, so every second keyword is block-probed whatever its
density -- the only way to narrow widths and long block spans at 300 001 docs.  Every check is bit-exact on status, total_found,
rowids and weights; stats()["pk_lean"] says which instance ran.  The keywords are built for the edges of the probe:
  LONG    90 000 docs: a 128-doc driver block of DRV300 spans more than 200 of its blocks (several chunk passes, the 64-ary search)
  RUN     1 000 consecutive rowids: blocks of width 7; eight driver blocks inside one block of GAP
  W16     a block whose last offset is 65 535 (width 16), one whose last offset is 65 536 (32-bit planes), a last block of one
          doc at offset 0 (width 0)
  L127 / L128   last blocks of 127 and of 128 docs
  GAP     2 000 docs with a hole around RUN
  EDGE    driver docs below LONG's first and above its last doc, on the first and last doc of blocks of LONG / W16 / RUN / L127 /
          L128, on a block's base rowid and one below the next block's base
  FAT     30 docs of 300 hits (the tf byte saturates: the exception list), TINY 12 docs that drive it
Every pair runs in both orders, under BM25 and NONE, with K = 3 (the threshold prunes), with a field limit on either keyword,
with dead rows, and with a rowid_base just below 2^32."""
import numpy as np
import pytest

from test_gpu_parity import kw, orc_index_of, to_orc

pytestmark = pytest.mark.gpu

N_DOCS = 300001
LONG, DRV300, RUN, W16, L127, L128, GAP, EDGE, FAT, TINY = range(10)


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    ctx.set("bitmap_inv", 1)  # (before the segments are packed)
    batch = m.Batch(ctx, 128)
    yield m, ctx, batch
    batch.close()
    ctx.close()


def pick(rng, lo, hi, n):
    return np.sort(rng.choice(np.arange(lo, hi, dtype=np.uint32), n, replace=False)).astype(np.uint32)


def block_edges(rows, blocks):
    """first and last doc, base rowid, one before the first doc and one past the last doc of the given 128-doc blocks"""
    out = []
    for b in blocks:
        first, last = int(rows[128 * b]), int(rows[min(128 * b + 127, rows.size - 1)])
        base = int(rows[128 * b - 1]) + 1 if b else 0
        out += [first, last, base, max(first - 1, 0), min(last + 1, N_DOCS - 1)]
    return out


def make_corpus(m):
    rng = np.random.default_rng(950)
    rows = [None] * 10
    rows[LONG] = pick(rng, 10, N_DOCS - 10, 90000)
    rows[DRV300] = pick(rng, 0, N_DOCS, 300)
    rows[RUN] = np.arange(5000, 6000, dtype=np.uint32)
    rows[W16] = np.concatenate([pick(rng, 0, 65535, 127), [65535], pick(rng, 65536, 131072, 127), [131072, 131073]]).astype(np.uint32)
    rows[L127] = pick(rng, 0, N_DOCS, 255)
    rows[L128] = pick(rng, 0, N_DOCS, 256)
    gap = np.concatenate([pick(rng, 0, 4000, 40), pick(rng, 8000, N_DOCS, 1955), [5000, 5127, 5128, 5500, 5999]])
    rows[GAP] = np.sort(gap).astype(np.uint32)
    n_long = (rows[LONG].size + 127) // 128
    edge = [0, 1, 2, N_DOCS - 2, N_DOCS - 1, 4999, 5000, 5127, 5128, 5999, 6000, 65534, 65535, 65536, 65537, 131071, 131072, 131073, 131074]
    edge += block_edges(rows[LONG], [0, 1, 2, 62, 63, 64, 126, 127, 300, n_long - 2, n_long - 1])
    edge += block_edges(rows[W16], [0, 1, 2]) + block_edges(rows[L127], [0, 1]) + block_edges(rows[L128], [0, 1]) + block_edges(rows[GAP], [0, 1, 15])
    rows[EDGE] = np.unique(np.array(edge, np.uint32))
    assert rows[EDGE].size < 128
    both = np.intersect1d(rows[DRV300], rows[LONG])
    rows[FAT] = np.unique(np.concatenate([both[:10], rows[EDGE][::7][:10], pick(rng, 0, N_DOCS, 10)])).astype(np.uint32)
    rows[TINY] = np.unique(np.concatenate([rows[FAT][::3], pick(rng, 0, N_DOCS, 3)])).astype(np.uint32)
    W, R, H = [], [], []
    for t, rw in enumerate(rows):
        if t == FAT:  # 300 hits in field 1: the tf saturates the packed byte
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
    assert [int(x) for x in hi.dict["docs"]] == [r.size for r in rows]
    assert rows[W16].size == 257 and rows[L127].size % 128 == 127 and rows[L128].size % 128 == 0 and rows[TINY].size < rows[FAT].size
    return hi


@pytest.fixture(scope="module")
def corpus(dev):
    return make_corpus(dev[0])


@pytest.fixture(scope="module")
def oindex(orc, corpus):
    return orc_index_of(orc, corpus)


def AND(m, a, b, ranker=None, mask=(0xFFFFFFFF, 0xFFFFFFFF), k=1000, fw=None):
    return m.Query(m.XQNode.AND(kw(m, a, 1, mask[0]), kw(m, b, 2, mask[1])), ranker=ranker if ranker is not None else m.SPH_RANK_BM25,
                   max_matches=k, field_weights=fw)


PAIRS = [(DRV300, LONG), (EDGE, LONG), (EDGE, W16), (EDGE, RUN), (EDGE, L127), (EDGE, L128), (EDGE, GAP), (RUN, LONG), (RUN, GAP),
         (L127, L128), (L127, LONG), (L128, LONG), (W16, LONG), (W16, RUN), (L128, W16), (TINY, FAT), (FAT, DRV300), (FAT, EDGE), (FAT, LONG),
         (DRV300, GAP), (TINY, EDGE), (DRV300, L127)]


def queries(m):
    """every pair and its swap: BM25, NONE, K = 3 under both, a field limit on the first / the second keyword, field weights"""
    qs = []
    for a, b in PAIRS:
        for x, y in ((a, b), (b, a)):
            qs += [AND(m, x, y), AND(m, x, y, ranker=m.SPH_RANK_NONE), AND(m, x, y, k=3), AND(m, x, y, ranker=m.SPH_RANK_NONE, k=3),
                   AND(m, x, y, mask=(0xFFFFFFFF, 1)), AND(m, x, y, mask=(2, 0xFFFFFFFF), fw=[3, 1, 2]), AND(m, x, y, mask=(5, 6), k=100)]
    return qs


def same(a, b, what):
    assert a.status == getattr(b, "status", 0) == 0, (what, a.status, getattr(b, "status", 0))  # (the oracle's results carry none)
    assert a.total_found == b.total_found, (what, a.total_found, b.total_found)
    assert np.array_equal(a.rowid, b.rowid), (what, a.rowid[:8], b.rowid[:8])
    assert np.array_equal(a.weight, b.weight), (what, a.weight[:8], b.weight[:8])


def run_both(dev, seg, qs):
    """the batch's answers on the lean and on the generic instance, with each run's stats"""
    m, ctx, batch = dev
    out = []
    try:
        for p in (1, 0):
            ctx.set("pair_scan", p)
            got = batch.search(seg, qs)
            st = batch.stats()
            assert st["packed"] == 1 and st["n_items_bm"] == 0 and st["n_items"] > 0, st  # nothing but block-scan work items ...
            assert st["pk_lean"] == p, st  # ... on the instance asked for
            out.append((got, st))
    finally:
        ctx.set("pair_scan", 1)
    return out


@pytest.fixture(scope="module")
def wanted(orc, dev, oindex):
    """the oracle's answers, computed once (without dead rows, which only one test sets)"""
    qs = queries(dev[0])
    return qs, [to_orc(orc, q).run(oindex) for q in qs]


def check(dev, hi, qs, want, rowid_base=0, dead=None):
    m, ctx, batch = dev
    seg = m.Segment(ctx, hi, rowid_base=rowid_base)
    if dead is not None:
        seg.set_dead_rows(dead)
    n_items = 0
    try:
        for i in range(0, len(qs), batch.max_queries):
            chunk = qs[i:i + batch.max_queries]
            (lean, st), (generic, _) = run_both(dev, seg, chunk)
            n_items += st["n_items"]
            for j in range(len(chunk)):
                same(lean[j], want[i + j], ("pair_scan=1 vs oracle", i + j))
                same(generic[j], want[i + j], ("pair_scan=0 vs oracle", i + j))
    finally:
        seg.close()
    return n_items


def test_corpus_reaches_the_probes_edges(corpus, wanted):
    """what the cases rest on: some docs match at every edge, and the found-then-failed field limit exists"""
    qs, want = wanted
    per = 7
    found = {PAIRS[i // (2 * per)]: want[i].total_found for i in range(0, len(qs), 2 * per)}
    for p in ((DRV300, LONG), (EDGE, LONG), (EDGE, W16), (EDGE, RUN), (EDGE, L127), (EDGE, L128), (EDGE, GAP), (RUN, GAP), (TINY, FAT), (FAT, DRV300)):
        assert found[p] > 0, p
    i = PAIRS.index((DRV300, LONG)) * 2 * per
    assert 0 < want[i + 4].total_found < want[i].total_found  # docs the second keyword holds, but not in the field asked for


def test_every_edge_both_orders(dev, corpus, wanted):
    qs, want = wanted
    check(dev, corpus, qs, want)


def test_item_cap_keeps_results_and_adds_items(dev, corpus, wanted):
    """p2_max_blocks = 4: one driver block per wave.  (pk_min_items = 2: a batch this small is otherwise cut down to four blocks an
    item by that rule already.)"""
    m, ctx, batch = dev
    qs, want = wanted
    n_items = []
    try:
        ctx.set("pk_min_items", 2)
        for cap in (0, 4):
            ctx.set("p2_max_blocks", cap)
            n_items.append(check(dev, corpus, qs, want))
    finally:
        ctx.set("p2_max_blocks", 4)
        ctx.set("pk_min_items", 2048)
    assert n_items[1] > n_items[0], n_items


def test_dead_rows(orc, dev, corpus, oindex, wanted):
    qs = wanted[0][::3]
    rng = np.random.default_rng(5)
    dead = np.zeros((N_DOCS + 31) // 32, np.uint32)
    killed = rng.choice(N_DOCS, size=N_DOCS // 4, replace=False)
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    oindex.dead_rows = dead
    try:
        want = [to_orc(orc, q).run(oindex) for q in qs]
    finally:
        oindex.dead_rows = None
    assert sum(w.total_found for w in want) < sum(w.total_found for w in wanted[1][::3])
    check(dev, corpus, qs, want, dead=dead)


def test_rowid_base_just_below_2_to_32(dev, corpus, wanted):
    qs, want = wanted
    check(dev, corpus, qs[::2], want[::2], rowid_base=(1 << 32) - N_DOCS - 3)
