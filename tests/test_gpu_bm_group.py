"""GPU: the grouped two-bitmap AND kernel (ctx key bm_group) against the ungrouped layout (bm_group=0) and the oracle.

With bm_group=1 a batch's scan_bm queries that share a keyword run in one workgroup, a wave per member (mrk_batch_submit,
scan_bm_kernel<SEQ, true>).  Every check is bit-exact on status, total_found, rowids and weights: groups of 1 to 4 members
in one batch, the same keyword pair twice and swapped, a keyword held by more than four queries, field limits, SPH_RANK_NONE
(the none_fast path), dead rows, rowid_base != 0, the nibble plane (the non-SEQ instance), a candidate-list overflow and its
rerun, and one batch reused across submits whose groupings differ."""
import numpy as np
import pytest

from helpers import synth_postings
from test_gpu_parity import kw, orc_index_of, to_orc

pytestmark = pytest.mark.gpu

PROBS = [0.6, 0.45, 0.3, 0.25, 0.2, 0.12, 0.08, 0.05, 0.03]


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
    m, ctx, batch = dev
    rng = np.random.default_rng(4096)
    n_docs = 150001  # no multiple of the 2048-rowid window
    W, R, H = synth_postings(rng, n_docs, PROBS, n_fields=3, max_pos=40)
    # docs of keyword 2 with 300 hits: the tf saturates the packed byte (the 255-tf escape)
    fat = rng.choice(n_docs, 30, replace=False).astype(np.uint32)
    keep = ~((W == 3) & np.isin(R, fat))
    W, R, H = W[keep], R[keep], H[keep]
    W = np.concatenate([W, np.full(fat.size * 300, 3, np.uint64)])
    R = np.concatenate([R, np.repeat(fat, 300)])
    H = np.concatenate([H, np.tile((np.uint32(1) << 24) | np.arange(1, 301, dtype=np.uint32), fat.size)])
    o = np.lexsort((H, R, W))
    return m.index_from_hits(W[o], R[o], H[o], n_terms=len(PROBS), total_docs=n_docs, n_fields=3), n_docs


def AND(m, a, b, ranker=None, mask=(0xFFFFFFFF, 0xFFFFFFFF), k=1000, fw=None, iw=1):
    return m.Query(m.XQNode.AND(kw(m, a, 1, mask[0]), kw(m, b, 2, mask[1])), ranker=ranker if ranker is not None else m.SPH_RANK_BM25,
                   max_matches=k, field_weights=fw, index_weight=iw)


def sized_groups(m):
    """Groups of 4, 3, 2 and 1 by the planner's greedy: keyword 0 in seven queries (a group of four, then three), the pair
    (1, 2) as given and swapped, and (3, 4) whose keywords the others hold only in groups already formed."""
    return [AND(m, 0, 1), AND(m, 0, 2), AND(m, 0, 3), AND(m, 0, 5), AND(m, 0, 6), AND(m, 0, 7), AND(m, 0, 8),
            AND(m, 1, 2), AND(m, 2, 1, ranker=m.SPH_RANK_NONE), AND(m, 3, 4)]


def mixed(m, rng, n):
    """Random pairs over the dense keywords: shared keywords, repeated and swapped pairs, field limits, both rankers,
    field weights (members of a group must share them: several classes), index weights, small and large K."""
    qs = []
    fws = [None, [3, 1, 2], [1, 5, 1]]
    for _ in range(n):
        a, b = (int(x) for x in rng.choice(7, 2, replace=False))
        mask = tuple(0xFFFFFFFF if rng.random() < 0.7 else int(rng.integers(1, 8)) for _ in range(2))
        qs.append(AND(m, a, b, ranker=m.SPH_RANK_NONE if rng.random() < 0.3 else m.SPH_RANK_BM25, mask=mask,
                      k=int(rng.choice([3, 100, 1000])), fw=fws[int(rng.integers(0, 3))], iw=int(rng.choice([1, 2]))))
    return qs


def same(a, b, what):
    assert a.status == getattr(b, "status", 0) == 0, (what, a.status, getattr(b, "status", 0))  # (the oracle's results carry none)
    assert a.total_found == b.total_found, (what, a.total_found, b.total_found)
    assert np.array_equal(a.rowid, b.rowid), (what, a.rowid[:8], b.rowid[:8])
    assert np.array_equal(a.weight, b.weight), (what, a.weight[:8], b.weight[:8])


def run_both(dev, seg, qs):
    """The batch's answers with bm_group=1 and with bm_group=0; the bitmap kernel must have run, and with bm_group=1 in
    groups of more than one query (stats n_bm_groups: groups of 1, 2, 3, 4 queries)."""
    m, ctx, batch = dev
    out = []
    try:
        for g in (1, 0):
            ctx.set("bm_group", g)
            got = batch.search(seg, qs)
            st = batch.stats()
            assert st["n_items_bm"] > 0
            if g:
                assert sum(st["n_bm_groups"][1:]) > 0, st["n_bm_groups"]
            else:
                assert st["n_bm_groups"] == [0, 0, 0, 0]
            out.append(got)
    finally:
        ctx.set("bm_group", 1)
    return out


def check(orc, dev, hi, qs, rowid_base=0, dead=None):
    m, ctx, batch = dev
    seg = m.Segment(ctx, hi, rowid_base=rowid_base)
    oi = orc_index_of(orc, hi)
    if dead is not None:
        seg.set_dead_rows(dead)
        oi.dead_rows = dead
    try:
        grouped, plain = run_both(dev, seg, qs)
        for i, q in enumerate(qs):
            want = to_orc(orc, q).run(oi)
            same(grouped[i], want, ("grouped vs oracle", i))
            same(plain[i], want, ("bm_group=0 vs oracle", i))
    finally:
        seg.close()


def test_group_sizes_pairs_and_rankers(orc, dev, corpus):
    m, ctx, batch = dev
    hi, _ = corpus
    seg = m.Segment(ctx, hi)
    try:
        batch.search(seg, sized_groups(m))
        assert batch.stats()["n_bm_groups"] == [1, 1, 1, 1]  # the planner formed the groups sized_groups() is built for
    finally:
        seg.close()
    rng = np.random.default_rng(1)
    qs = sized_groups(m) + [AND(m, 1, 2), AND(m, 4, 3, ranker=m.SPH_RANK_NONE), AND(m, 5, 6, mask=(1, 6))] + mixed(m, rng, 60)
    check(orc, dev, hi, qs)


def test_dead_rows_and_rowid_base(orc, dev, corpus):
    m, ctx, batch = dev
    hi, n_docs = corpus
    rng = np.random.default_rng(2)
    dead = np.zeros((n_docs + 31) // 32, np.uint32)
    killed = rng.choice(n_docs, size=n_docs // 5, replace=False)
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    qs = sized_groups(m) + mixed(m, rng, 40)
    check(orc, dev, hi, qs, dead=dead)
    check(orc, dev, hi, qs, rowid_base=3 * 65536 + 17)


def test_nibble_plane_instance(orc, dev, corpus):
    """attr_nibbles: the segment gathers from the one-byte plane, the kernel's non-SEQ instance."""
    m, ctx, batch = dev
    hi, _ = corpus
    ctx.set("attr_nibbles", 1)
    try:
        check(orc, dev, hi, sized_groups(m) + mixed(m, np.random.default_rng(3), 40))
    finally:
        ctx.set("attr_nibbles", 0)


def test_reused_batch_with_changing_groupings(orc, dev, corpus):
    """One batch, submits whose groups differ (sizes, classes, a lone query, then grouped again), forwards and back."""
    m, ctx, batch = dev
    hi, _ = corpus
    rng = np.random.default_rng(4)
    sets = [sized_groups(m), [AND(m, 5, 6)], mixed(m, rng, 90), [AND(m, 0, 1), AND(m, 1, 0)], mixed(m, rng, 25)]
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    try:
        want = [[to_orc(orc, q).run(oi) for q in qs] for qs in sets]
        for order in (range(len(sets)), reversed(range(len(sets)))):
            for s in order:
                got = batch.search(seg, sets[s])
                for i, g in enumerate(got):
                    same(g, want[s][i], ("set", s, i))
    finally:
        seg.close()


def test_candidate_overflow_in_a_group_is_rerun(orc, dev):
    """Every doc holds all three keywords with one weight: nothing prunes, the grouped members' candidate lists overflow,
    and each query is rerun alone (ungrouped) with a full-size list."""
    m, ctx, batch = dev
    n_docs = 1_300_000
    rows = np.arange(n_docs, dtype=np.uint32)
    W = np.concatenate([np.full(n_docs, t + 1, np.uint64) for t in range(3)])
    R = np.concatenate([rows] * 3)
    H = np.concatenate([np.full(n_docs, (1 << 24) | (t + 1), np.uint32) for t in range(3)])
    hi = m.index_from_hits(W, R, H, n_terms=3, total_docs=n_docs, n_fields=2)
    qs = [AND(m, 0, 1), AND(m, 0, 2, k=100), AND(m, 1, 2, k=10), AND(m, 2, 0, ranker=m.SPH_RANK_NONE, k=50)]
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    try:
        grouped, plain = run_both(dev, seg, qs)
        for i, q in enumerate(qs):
            g = grouped[i]
            assert g.total_found == n_docs and list(g.rowid) == list(range(q.max_matches)), i
            same(g, plain[i], ("grouped vs bm_group=0", i))
            if i < 2:
                same(g, to_orc(orc, q).run(oi), ("grouped vs oracle", i))
    finally:
        seg.close()
