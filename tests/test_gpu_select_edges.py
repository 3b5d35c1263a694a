"""GPU: the relevance top-K selection (csrc/mrk_select.hip: sel_tau_kernel, sel_filter_kernel, sel_sort_kernel with its sub-bin pass) at
its edges -- ties across the rank-K class, winners at either end of the candidate list, lists of 2048 j +- 1 keys, rowid bins on large
rowid bases, the planner's fallback geometry, a list of two chunks of slices, a launch of two filter groups.  One small deterministic
corpus per edge (tests/select_edges_common.py); tests/test_select_edges_cpu.py asserts on the CPU that each has the structure its case
names and that the planner gives the geometry it relies on.

Every result is bit-exact against the DEFINITION of the sorter's order (weight descending, rowid ascending) applied to the oracle's
full match list: status, rowids in order, weights, total_found.  Routes: "bitmap" (packed, bitmap_inv = 64: the two-bitmap AND kernel
feeds the selection), "block" (packed, bitmap_inv = 0: the block scan does), "vlb" (path = 1: no mrk_select.hip at all -- a third
opinion).  Every batch is searched twice and must give the same bytes.

n_cands.  The scan kernels prune by pruning BIN alone (bin_of(..) >= tau_bin in scan_bm / scan_p2 / scan_pk; the second-level
histogram is the proximity rankers').  Under BM25 every member of the weight class that holds rank K shares the final threshold's bin, so
the candidate lists must hold them all: n_cands >= the sum of those classes' sizes over the batch.  Under SPH_RANK_NONE the bins are
over the ROWID: the one weight class spreads over them and the scan rightly drops its members below the threshold bin (scan_bm even
skips whole windows), so the bound the code gives is K per query -- except where the segment ends at 2^32 - 1 and every match shares
the clamped bin 0: there it is the whole class again.  A query whose list overflowed stops counting (its other work items return
early): all that holds is n_cands > the list's 2^20 slots."""
import contextlib

import numpy as np
import pytest

import manticoresearch_amd as m
import select_edges_common as se

pytestmark = pytest.mark.gpu

ROUTES = ("bitmap", "block", "vlb")


@pytest.fixture(scope="module")
def corpora(orc):
    return se.Corpora(m, orc)


@contextlib.contextmanager
def device(route, hi, max_queries, rowid_base=0):
    """one context, segment and batch on the route, closed whatever happens"""
    ctx = m.Context(0)
    seg = batch = None
    try:
        ctx.set("path", 1 if route == "vlb" else 0)
        ctx.set("bitmap_inv", 64 if route == "bitmap" else 0)
        seg = m.Segment(ctx, hi, rowid_base=rowid_base)
        batch = m.Batch(ctx, max_queries)
        yield ctx, seg, batch
    finally:
        if batch is not None:
            batch.close()
        if seg is not None:
            seg.close()
        ctx.close()


def class_size(full, K):
    """T: the size of the class that holds rank K"""
    cls = se.classes(full)
    return cls[se.rank_class(cls, K)[0]][1] if cls else 0


def run(route, seg, batch, queries, wants, floor, pairs=True, rerun=0):
    """search twice; every result against its expectation (rowids, weights, total); the route really taken; n_cands >= floor"""
    got = batch.search(seg, queries)
    st = batch.stats()
    again = batch.search(seg, queries)
    for i, (q, g, a, (rid, w, total)) in enumerate(zip(queries, got, again, wants)):
        assert g.status == 0, (route, i, g.status)
        assert g.total_found == total, (route, i, g.total_found, total)
        assert np.array_equal(g.rowid, rid), (route, i, q.max_matches, len(g.rowid), len(rid), g.rowid[:4], rid[:4], np.flatnonzero(g.rowid[:min(len(rid), len(g.rowid))] != rid[:min(len(rid), len(g.rowid))])[:4])
        assert np.array_equal(g.weight, w), (route, i, g.weight[:4], w[:4])
        assert a.status == 0 and a.total_found == g.total_found and a.rowid.tobytes() == g.rowid.tobytes() and a.weight.tobytes() == g.weight.tobytes(), (route, i, "second search differs")
    if route == "vlb":
        assert st["packed"] == 0
        return st
    assert st["packed"] == 1
    if route == "bitmap" and pairs:
        assert st["n_items_bm"] > 0  # the two-bitmap AND kernel took the dense pairs
    assert st["n_rerun"] == rerun, st["n_rerun"]
    print("%s: n_cands %d floor %d n_items %d n_items_bm %d scan %.3f ms" % (route, st["n_cands"], floor, st["n_items"], st["n_items_bm"], st["scan_ms"]))
    assert st["n_cands"] >= floor, (route, st["n_cands"], floor)
    return st


# ------------------------------------------------------------------ A: ladders
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("placement", se.PLACEMENTS)
@pytest.mark.parametrize("ladder", ["L1", "L2"])
def test_ladders(corpora, ladder, placement, route):
    """Rank K as the last of a class, the first of the next, inside a class smaller than the sort's buffer (no sub-bins) and inside one
    far larger with other classes above it (sub-bins, need = K - above); better classes at the front, at the end and all over the list."""
    name = ("shared", ladder, placement)
    hi, _ = corpora.get(*name)
    full = corpora.full(name, "bm25", se.q_and(m, 1000))
    qs = [se.q_and(m, K) for K in se.LADDER_KS[ladder]]
    wants = [se.cut(full, q.max_matches) for q in qs]
    with device(route, hi, len(qs)) as (ctx, seg, batch):
        run(route, seg, batch, qs, wants, sum(class_size(full, q.max_matches) for q in qs))
        one = se.q_and(m, 1000)
        run(route, seg, batch, [one], [se.cut(full, 1000)], class_size(full, 1000))


# ------------------------------------------------------------------ B: one class
@pytest.mark.parametrize("route", ROUTES)
def test_one_class(corpora, route):
    """60 000 matches of one weight: the list fits its slots (no rerun), the rowid alone decides."""
    name = ("shared", "ONE", "low")
    hi, _ = corpora.get(*name)
    full = corpora.full(name, "bm25", se.q_and(m, 1000))
    qs = [se.q_and(m, K) for K in se.LADDER_KS["ONE"]]
    wants = [se.cut(full, q.max_matches) for q in qs]
    assert wants[-1][0].tolist() == [4 * i for i in range(1024)]
    with device(route, hi, len(qs)) as (ctx, seg, batch):
        run(route, seg, batch, qs, wants, len(qs) * se.SHARED_MATCHES, rerun=0)
        run(route, seg, batch, qs[2:3], wants[2:3], se.SHARED_MATCHES, rerun=0)


# ------------------------------------------------------------------ C: slice edges
@pytest.mark.parametrize("route", ROUTES)
def test_slice_edges(corpora, route):
    """Lists of 2048 j - 1, 2048 j and 2048 j + 1 keys (and of one), back to back in one batch: slice counts, the last slice's length, the
    neighbours' slice counters; a ten-doc class on top that every scan finds last."""
    name = ("slices",)
    hi, _ = corpora.get(*name)
    qs = se.slice_batch(m)
    fulls = [corpora.full(name, ("one", t), q) for t, q in enumerate(qs[:9])] * 2 + [corpora.full(name, ("and", t), q) for t, q in enumerate(qs[18:])]
    wants = [se.cut(f, q.max_matches) for f, q in zip(fulls, qs)]
    with device(route, hi, len(qs)) as (ctx, seg, batch):
        run(route, seg, batch, qs, wants, sum(class_size(f, q.max_matches) for f, q in zip(fulls, qs)))


# ------------------------------------------------------------------ D: rowid bins and large bases
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("base", se.BASES, ids=["base0", "base2p24", "ends_at_2p32"])
def test_rowid_bins_and_bases(corpora, base, route):
    """SPH_RANK_NONE bins by global rowid: a small shift at base 0, shift 15 at 2^24 (sub-bins over rowids), shift 22 and the clamped bin 0
    for a range that ends at 2^32 - 1 (no sub-bins: one sort over 60 000 ties).  The ladder under BM25 at the same bases runs
    rowid_hi - rowid with a base.  A segment one rowid further is refused."""
    name = ("shared", "L2", "even")
    hi, _ = corpora.get(*name)
    none = corpora.full(name, "none", se.q_and(m, 1000, ranker=m.SPH_RANK_NONE))
    full = corpora.full(name, "bm25", se.q_and(m, 1000))
    ks = (1, 1000, 1024)
    qn = [se.q_and(m, K, ranker=m.SPH_RANK_NONE) for K in ks]
    qb = [se.q_and(m, K) for K in se.LADDER_KS["L2"]]
    all_in_bin0 = base + se.SHARED_DOCS == 2**32
    with device(route, hi, 8, rowid_base=base) as (ctx, seg, batch):
        run(route, seg, batch, qn, [se.cut(none, K) for K in ks], 3 * se.SHARED_MATCHES if all_in_bin0 else sum(ks))
        run(route, seg, batch, qn[1:2], [se.cut(none, 1000)], se.SHARED_MATCHES if all_in_bin0 else 1000)
        run(route, seg, batch, qb, [se.cut(full, q.max_matches) for q in qb], sum(class_size(full, q.max_matches) for q in qb))
        if all_in_bin0:
            with pytest.raises(m.MrkError) as e:
                m.Segment(ctx, hi, rowid_base=base + 1)
            assert e.value.code == -1  # MRK_E_INVAL


# ------------------------------------------------------------------ E: the planner's fallback geometry
@pytest.mark.parametrize("route", ROUTES)
def test_fallback_geometry(corpora, route):
    """Field weights whose planned range leaves int32 (bin_lo = INT32_MIN, bin_shift = 31; select_subkey.cpp asserts it): two bins, and
    every survivor in sub-bin 0."""
    name = ("shared", "L2", "even")
    hi, _ = corpora.get(*name)
    fw = list(se.FALLBACK_FIELD_WEIGHTS)
    full = corpora.full(name, "fallback", se.q_and(m, 1000, field_weights=fw))
    assert int(full.weight.max()) < 2**31 - 1 and int(full.weight.min()) > 0
    qs = [se.q_and(m, K, field_weights=fw) for K in (1000, 1024)]
    with device(route, hi, len(qs)) as (ctx, seg, batch):
        run(route, seg, batch, qs, [se.cut(full, q.max_matches) for q in qs], 2 * se.SHARED_MATCHES)  # (one bin holds every match)
        run(route, seg, batch, qs[:1], [se.cut(full, 1000)], se.SHARED_MATCHES)


# ------------------------------------------------------------------ F: two chunks of slices
def test_two_chunks(corpora):
    """2.2 M candidates of one bin: the 2^20-slot list overflows, the rerun's list is 1075 slices -- two chunks of the sort pass -- and
    the 700 best docs are the LAST keys of the second chunk.  Block route only.  (The one case here that takes more than a moment:
    DESIGN.md section 4 has its time.)"""
    name = ("chunks",)
    hi, _ = corpora.get(*name)
    q = se.q_one(m, 0, 1000)
    want = corpora.want(name, "one", q)
    assert want[0].tolist() == list(range(se.CHUNK_DOCS - se.CHUNK_TOP, se.CHUNK_DOCS)) + list(range(1000 - se.CHUNK_TOP))
    assert 1024 * 2048 < se.CHUNK_DOCS < 2 * 1024 * 2048  # SCH slices of SEL_SLICE keys per chunk: two chunks
    with device("block", hi, 1) as (ctx, seg, batch):
        run("block", seg, batch, [q], [want], (1 << 20) + 1, pairs=False, rerun=1)


# ------------------------------------------------------------------ G: the second filter group (keep this test the last of the file)
def test_second_filter_group(corpora):
    """4100 queries in one launch: sel_filter_kernel runs twice, the second time with q0 = 4096; the lists around the group edge are
    the 4097-, 6143- and 6145-key ones.  Single keywords: the block scan feeds the selection on either packed route, so one route."""
    name = ("slices",)
    hi, _ = corpora.get(*name)
    group = se.group_batch(m)
    assert len(group) == se.GROUP_QUERIES and [t for t, _ in group[4093:]] == [6, 7, 8, 6, 7, 8, 6]
    qs = [se.q_one(m, t, K) for t, K in group]
    want_of = {(t, K): corpora.want(name, ("one", t), se.q_one(m, t, K)) for t, K in set(group)}
    size_of = {(t, K): class_size(corpora.full(name, ("one", t), None), K) for t, K in set(group)}
    with device("block", hi, len(qs)) as (ctx, seg, batch):
        run("block", seg, batch, qs, [want_of[g] for g in group], sum(size_of[g] for g in group), pairs=False)
