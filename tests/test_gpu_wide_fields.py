"""GPU: segments with 9-32 full-text fields on the packed path (the field-mask plane pk_fmask and the WIDE instances of the scan
and rank kernels), bit-exact against the oracle: keywords, N-way ANDs, OR / MAYBE / ANDNOT / QUORUM trees, PHRASE, "a b"~N,
BEFORE, NEAR, NOTNEAR, ^a / a$ / @field[N], a 5-word phrase (the generic evaluator), field limits that name high fields only or mix
low and high ones, every ranker, random weights for all 32 fields (negative ones included), index weights, attribute filters,
weight filters and cutoff.  Every query runs packed with status 0; pruning in front of the hit pass and the bound by keywords
change nothing; the same AND / BM25 / NONE batch on the VLB path gives the same answer; a query parsed with 20 named fields."""
import numpy as np
import pytest

from helpers import synth_postings
from test_gpu_parity import orc_index_of, to_orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    yield m, ctx, batch
    batch.close()
    ctx.close()


def kw(m, t, pos, mask=0xFFFFFFFF):
    return m.XQNode.keyword(t, pos, mask)


def wide_corpus(m, n_fields, block, fmt, end_markers, seed):
    """synth_postings spreads every keyword's hits over all fields; one more keyword holds docs whose tf >= 255 is spread
    over two or more fields above 8."""
    rng = np.random.default_rng(seed)
    n_docs = 6000
    probs = [0.4, 0.25, 0.1, 0.05, 0.02, 0.6]
    W, R, H = synth_postings(rng, n_docs, probs, n_fields=n_fields, max_pos=300, end_markers=end_markers)
    W2, R2, H2 = [W], [R], [H]
    hi_fields = list(range(8, n_fields))
    for r in rng.choice(n_docs, 40, replace=False):
        fs = rng.choice(hi_fields, size=min(len(hi_fields), int(rng.integers(2, 5))), replace=False)
        hp = np.unique(np.concatenate([(np.uint32(f) << 24) | np.arange(1, 1 + int(rng.integers(90, 200)), dtype=np.uint32) for f in fs]))
        W2.append(np.full(hp.size, len(probs) + 1, np.uint64))
        R2.append(np.full(hp.size, r, np.uint32))
        H2.append(hp)
    W, R, H = (np.concatenate(x) for x in (W2, R2, H2))
    order = np.lexsort((H, R, W))
    hi = m.index_from_hits(W[order], R[order], H[order], n_terms=len(probs) + 1, total_docs=n_docs, skiplist_block_size=block,
                           hit_format=fmt, n_fields=n_fields)
    return hi, len(probs) + 1


def high_masks(n_fields):
    top = n_fields - 1
    return [0xFFFFFFFF, 1 << 8, 1 << min(20, top), 1 << top, (1 << 2) | (1 << top), 0xFF, ((1 << n_fields) - 1) & ~0xFF]


ALL_RANKERS = ["SPH_RANK_NONE", "SPH_RANK_BM25", "SPH_RANK_PROXIMITY_BM25", "SPH_RANK_PROXIMITY", "SPH_RANK_SPH04", "SPH_RANK_WORDCOUNT",
               "SPH_RANK_MATCHANY", "SPH_RANK_FIELDMASK"]


def query_mix(m, rng, n_terms, n_fields, with_filters):
    masks = high_masks(n_fields)
    rankers = [getattr(m, r) for r in ALL_RANKERS]
    qs = []

    def k(pos):
        return kw(m, int(rng.integers(0, n_terms)), pos, int(rng.choice(masks)))

    def weights():
        return [int(x) for x in rng.integers(-20, 100, 32)] if rng.random() < 0.8 else None

    def add(root, ranker, **extra):
        qs.append(m.Query(root, ranker=ranker, max_matches=int(rng.choice([20, 1000])), field_weights=weights(),
                          index_weight=int(rng.choice([1, 1, 3])), **extra))

    for _ in range(12):  # single keywords: the weight-sum forms of the proximity rankers too
        add(k(1), int(rng.choice(rankers + [m.SPH_RANK_PROXIMITY, m.SPH_RANK_PROXIMITY_BM25])))
    for _ in range(16):
        a, b, c = (int(x) for x in rng.choice(n_terms, 3, replace=False))
        ma, mb, mc = (int(rng.choice(masks)) for _ in range(3))
        rk = int(rng.choice(rankers))
        add(m.XQNode.AND(kw(m, a, 1, ma), kw(m, b, 2, mb)), rk)
        add(m.XQNode.AND(kw(m, a, 1, ma), kw(m, b, 2, mb), kw(m, c, 3, mc)), rk)
        add(m.XQNode(m.SPH_QUERY_OR, [kw(m, a, 1, ma), kw(m, b, 2, mb)]), rk)
        add(m.XQNode(m.SPH_QUERY_MAYBE, [kw(m, a, 1, ma), kw(m, b, 2, mb)]), rk)
        add(m.XQNode(m.SPH_QUERY_ANDNOT, [kw(m, a, 1, ma), kw(m, b, 2, mb)]), rk)
        add(m.XQNode.AND(m.XQNode(m.SPH_QUERY_OR, [kw(m, a, 1, ma), kw(m, b, 2, mb)]), kw(m, c, 3, mc)), rk)
        add(m.XQNode(m.SPH_QUERY_QUORUM, [kw(m, a, 1), kw(m, b, 2), kw(m, c, 3)], None, m.ALL_FIELDS, 2), rk)
        # a field limit on the operator rather than on its keywords
        add(m.XQNode(m.SPH_QUERY_AND, [kw(m, a, 1), kw(m, b, 2)], None, int(rng.choice(masks[1:]))), rk)
        # the hit-reading shapes
        add(m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, a, 1), kw(m, b, 2)]), rk)
        add(m.XQNode(m.SPH_QUERY_PROXIMITY, [kw(m, a, 1), kw(m, b, 2), kw(m, c, 3)], None, m.ALL_FIELDS, int(rng.integers(2, 6))), rk)
        add(m.XQNode(m.SPH_QUERY_BEFORE, [kw(m, a, 1), kw(m, b, 2)]), rk)
        add(m.XQNode(m.SPH_QUERY_NEAR, [kw(m, a, 1), kw(m, b, 2)], None, m.ALL_FIELDS, int(rng.integers(1, 8))), rk)
        add(m.XQNode(m.SPH_QUERY_NOTNEAR, [kw(m, a, 1), kw(m, b, 2)], None, m.ALL_FIELDS, int(rng.integers(1, 8))), rk)
        add(m.XQNode.AND(m.XQNode.keyword(a, 1, ma, field_start=True), kw(m, b, 2, mb)), rk)
        add(m.XQNode.AND(m.XQNode.keyword(a, 1, field_end=True), kw(m, b, 2)), rk)
        add(m.XQNode.AND(m.XQNode.keyword(a, 1, ma, field_max_pos=int(rng.integers(5, 60))), kw(m, b, 2)), rk)
        add(m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, int(x), i + 1) for i, x in enumerate(rng.choice(n_terms, 5, replace=False))]), rk)
        add(m.XQNode(m.SPH_QUERY_OR, [m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, a, 1), kw(m, b, 2)]), kw(m, c, 3, mc)]), rk)
    if with_filters:
        for q in qs[::3]:
            q.filters = [m.Filter(0, 32, values=[1, 3, 4])]
        for q in qs[1::5]:
            if q.ranker != m.SPH_RANK_NONE:
                q.weight_filters = [m.Filter(0, 32, min=-50000, max=2000 * q.index_weight)]
        for q in qs[2::7]:
            if not q.weight_filters:
                q.cutoff = int(rng.choice([1, 7, 100]))
    return qs


def run_and_check(orc, dev, hi, queries, attrs=None):
    m, ctx, batch = dev
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    if attrs is not None:
        seg.set_attrs(attrs)
        oi.attrs = attrs
    try:
        out = []
        for i in range(0, len(queries), batch.max_queries):
            chunk = queries[i:i + batch.max_queries]
            got = batch.search(seg, chunk)
            assert batch.stats()["packed"] == 1
            for q, g in zip(chunk, got):
                want = to_orc(orc, q).run(oi)
                assert g.status == 0
                assert g.total_found == want.total_found, (g.total_found, want.total_found)
                assert np.array_equal(g.rowid, want.rowid), (g.rowid[:10], want.rowid[:10])
                assert np.array_equal(g.weight, want.weight), (g.weight[:10], want.weight[:10])
            out += got
        return out
    finally:
        seg.close()


@pytest.mark.parametrize("n_fields", [9, 16, 31, 32])
@pytest.mark.parametrize("block,fmt,end_markers", [(32, 0, False), (128, 1, True), (128, 0, True), (32, 1, False)])
def test_wide_segment_every_shape_and_ranker(orc, dev, n_fields, block, fmt, end_markers):
    m = dev[0]
    hi, nt = wide_corpus(m, n_fields, block, fmt, end_markers, seed=n_fields * 7 + block + fmt)
    rng = np.random.default_rng(n_fields + 100 * block + fmt)
    attrs = (np.arange(hi.total_docs, dtype=np.uint32) % 5).reshape(-1, 1)
    run_and_check(orc, dev, hi, query_mix(m, rng, nt, n_fields, with_filters=True), attrs)


def test_wide_segment_packed_equals_vlb(orc, dev):
    """AND / BM25 / NONE: the packed WIDE instance and the VLB kernel agree (and both agree with the oracle)."""
    m, ctx, batch = dev
    hi, nt = wide_corpus(m, 20, 128, 1, True, seed=5)
    rng = np.random.default_rng(5)
    qs = []
    for _ in range(40):
        a, b = (int(x) for x in rng.choice(nt, 2, replace=False))
        qs.append(m.Query(m.XQNode.AND(kw(m, a, 1, int(rng.choice(high_masks(20)))), kw(m, b, 2)), ranker=int(rng.choice([m.SPH_RANK_NONE, m.SPH_RANK_BM25])),
                          field_weights=[int(x) for x in rng.integers(-5, 60, 32)]))
    packed = run_and_check(orc, dev, hi, qs)
    seg = m.Segment(ctx, hi)
    try:
        ctx.set("path", 1)
        vlb = batch.search(seg, qs)
        assert batch.stats()["packed"] == 0
    finally:
        ctx.set("path", 0)
        seg.close()
    for p, v in zip(packed, vlb):
        assert v.status == 0 and p.total_found == v.total_found
        assert np.array_equal(p.rowid, v.rowid) and np.array_equal(p.weight, v.weight)


def test_wide_segment_dense_keywords_without_bitmap_kernels(orc, dev):
    """Dense keywords keep their bitmaps (the block scan probes them) but a wide segment never goes to the bitmap kernels."""
    m = dev[0]
    rng = np.random.default_rng(9)
    W, R, H = synth_postings(rng, 40000, [0.6, 0.5, 0.3, 0.01], n_fields=24, max_pos=50)
    hi = m.index_from_hits(W, R, H, n_terms=4, total_docs=40000, n_fields=24)
    qs = [m.Query(m.XQNode.AND(kw(m, a, 1, mk), kw(m, b, 2)), ranker=rk, field_weights=[int(x) for x in rng.integers(-3, 30, 32)])
          for a in range(4) for b in range(4) if a != b for mk in (0xFFFFFFFF, 1 << 23, 0xFF00) for rk in (m.SPH_RANK_NONE, m.SPH_RANK_BM25)]
    run_and_check(orc, dev, hi, qs)
    assert dev[2].stats()["n_items_bm"] == 0


def test_wide_segment_pruning_changes_nothing(orc, dev):
    """prox_prune 0 == 1, and prox_bound_keywords 0 == 1 on a corpus without field-end flags, under the hit rankers."""
    m, ctx, batch = dev
    hi, nt = wide_corpus(m, 24, 128, 1, False, seed=8)
    rng = np.random.default_rng(8)
    qs = []
    for _ in range(60):
        a, b, c = (int(x) for x in rng.choice(nt, 3, replace=False))
        root = m.XQNode.AND(kw(m, a, 1, int(rng.choice(high_masks(24)))), kw(m, b, 2), kw(m, c, 3)) if rng.random() < 0.5 else \
            m.XQNode.AND(kw(m, a, 1), kw(m, b, 2, int(rng.choice(high_masks(24)))))
        qs.append(m.Query(root, ranker=int(rng.choice([m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_PROXIMITY])), max_matches=int(rng.choice([10, 100])),
                          field_weights=[int(x) for x in rng.integers(-10, 100, 32)]))
    base = run_and_check(orc, dev, hi, qs)
    seg = m.Segment(ctx, hi)
    try:
        for key in ("prox_prune", "prox_bound_keywords"):
            for v in (0, 1):
                ctx.set(key, v)
                got = batch.search(seg, qs)
                assert batch.stats()["packed"] == 1
                for p, g in zip(base, got):
                    assert g.status == 0 and g.total_found == p.total_found
                    assert np.array_equal(g.rowid, p.rowid) and np.array_equal(g.weight, p.weight)
        ctx.set("prox_prune", 1)
        ctx.set("prox_bound_keywords", 0)
    finally:
        seg.close()


def test_wide_segment_parsed_query_with_20_named_fields(orc, dev):
    m = dev[0]
    hi, nt = wide_corpus(m, 20, 128, 1, True, seed=4)
    names = [f"f{i}" for i in range(20)]
    words = {f"w{i}": i for i in range(nt)}
    qs = []
    for text in ["@(f12,f19) \"w0 w1\"~3 | w2 << w3", "@f15 w0 w5", "@(f0,f9) w1 -w2", "\"w0 w1 w2\"/2", "@f8 ^w0 w1$", "w5 NEAR/4 w0"]:
        root = m.parse_query(text, names, lookup=lambda w: words.get(w, -1))
        for rk in ALL_RANKERS:
            qs.append(m.Query(root, ranker=getattr(m, rk), field_weights=list(range(1, 33))))
    run_and_check(orc, dev, hi, qs)


def test_wide_segment_larger_corpus_proximity_mix(orc, dev):
    """16 fields, 1 M docs from the synthetic generator, 3-keyword PROXIMITY_BM25 queries like bench.py's config 3."""
    m = dev[0]
    probs = [0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005]
    hi = m.synth_index(1_000_000, probs, seed=0x5EED0016, n_fields=16)
    rng = np.random.default_rng(16)
    qs = []
    for i in range(48):
        a, b, c = (int(x) for x in rng.choice(len(probs), 3, replace=False))
        k = [kw(m, a, 1), kw(m, b, 2), kw(m, c, 3)]
        shape = i % 4
        root = (m.XQNode.AND(*k) if shape == 0 else m.XQNode.AND(m.XQNode(m.SPH_QUERY_OR, k[:2]), k[2]) if shape == 1
                else m.XQNode.AND(k[0], m.XQNode(m.SPH_QUERY_OR, k[1:])) if shape == 2 else m.XQNode(m.SPH_QUERY_ANDNOT, [m.XQNode.AND(*k[:2]), k[2]]))
        qs.append(m.Query(root, ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=1000, field_weights=[int(x) for x in rng.integers(1, 20, 32)]))
    run_and_check(orc, dev, hi, qs)
