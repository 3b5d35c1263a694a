"""GPU: the dispatch order of the two-bitmap AND kernel's work items (ctx key bm_place) against the oracle.

bm_place only reorders the finished work items of a launch (mrk::place_bm_items: 1 = owners that share keywords in one of
eight dispatch classes, every class in window order; 2 = window order alone; 0 = the layout's piece-major order), so every
answer must stay bit for bit what the oracle gives: status, total_found, rowids and weights.  The corpus has 74 windows and
bm_min_windows is 16: a group of four is cut into 19 pieces, a lone query into 5, so the orders really differ.  Checked: the
three modes on groups of all four sizes (more than eight owners), the ungrouped layout (bm_group=0), dead rows, rowid_base
!= 0, SPH_RANK_NONE and field-limited members, one batch reused across submits whose groupings and placements differ, a
candidate overflow and its rerun, a one-query launch, where no placement runs, and the least launch size (bm_place_min_items)."""
import numpy as np
import pytest

from helpers import synth_postings
from test_gpu_bm_group import AND, PROBS, mixed, same, sized_groups
from test_gpu_parity import orc_index_of, to_orc

pytestmark = pytest.mark.gpu

MODES = (1, 2, 0)


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    ctx.set("bm_min_windows", 16)
    ctx.set("bm_place_min_items", 0)  # (launches this small keep the layout's order by default)
    batch = m.Batch(ctx, 128)
    yield m, ctx, batch
    batch.close()
    ctx.close()


@pytest.fixture(scope="module")
def corpus(dev):
    m, ctx, batch = dev
    rng = np.random.default_rng(4096)
    n_docs = 150001  # 74 windows of 2048 rowids, the last one short
    W, R, H = synth_postings(rng, n_docs, PROBS, n_fields=3, max_pos=40)
    o = np.lexsort((H, R, W))
    return m.index_from_hits(W[o], R[o], H[o], n_terms=len(PROBS), total_docs=n_docs, n_fields=3), n_docs


def queries(m, seed=11, n=34):
    """Groups of 4, 3, 2 and 1 by construction, then random pairs (shared keywords, swapped pairs, field limits, both rankers,
    several field-weight classes): 44 queries, more than eight owners."""
    return sized_groups(m) + mixed(m, np.random.default_rng(seed), n)


def run_modes(dev, seg, qs, group=1):
    """The batch's answers under bm_place 1, 2 and 0, with each submit's stats."""
    m, ctx, batch = dev
    out = []
    try:
        ctx.set("bm_group", group)
        for mode in MODES:
            ctx.set("bm_place", mode)
            got = batch.search(seg, qs)
            out.append((mode, got, batch.stats()))
    finally:
        ctx.set("bm_group", 1)
        ctx.set("bm_place", 2)
    return out


def check(orc, dev, hi, qs, rowid_base=0, dead=None, group=1):
    m, ctx, batch = dev
    seg = m.Segment(ctx, hi, rowid_base=rowid_base)
    oi = orc_index_of(orc, hi)
    if dead is not None:
        seg.set_dead_rows(dead)
        oi.dead_rows = dead
    try:
        want = [to_orc(orc, q).run(oi) for q in qs]
        runs = run_modes(dev, seg, qs, group)
        for mode, got, st in runs:
            assert st["n_items_bm"] > 0
            for i in range(len(qs)):
                same(got[i], want[i], ("bm_place", mode, "bm_group", group, "query", i))
        return runs
    finally:
        seg.close()


def test_modes_on_groups_of_every_size(orc, dev, corpus):
    m, ctx, batch = dev
    hi, _ = corpus
    runs = check(orc, dev, hi, queries(m))
    for mode, _, st in runs:
        groups = st["n_bm_groups"]
        assert min(groups) >= 1 and sum(groups) > 8, groups  # owners of all four sizes, more than the eight classes
        if mode == 0:
            assert st["bm_owner_keys"] == 0 and st["bm_class_keys"] == 0, st
        else:
            # every group holds at least two keywords; the classes cannot hold more pairs than the owners
            assert st["bm_owner_keys"] >= 2 * sum(groups) and 1 <= st["bm_class_keys"] <= st["bm_owner_keys"], st
    by_mode = {mode: st for mode, _, st in runs}
    # one class holds each of the launch's keywords once: eight classes cannot hold fewer
    assert by_mode[1]["bm_class_keys"] >= by_mode[2]["bm_class_keys"] and by_mode[1]["bm_owner_keys"] == by_mode[2]["bm_owner_keys"], by_mode


def test_ungrouped_layout(orc, dev, corpus):
    m, ctx, batch = dev
    hi, _ = corpus
    runs = check(orc, dev, hi, queries(m, seed=12), group=0)
    for mode, _, st in runs:
        assert st["n_bm_groups"] == [0, 0, 0, 0]
        if mode:
            assert st["bm_owner_keys"] == 2 * 44, st  # an owner is a query: its two keywords


def test_dead_rows_and_rowid_base(orc, dev, corpus):
    m, ctx, batch = dev
    hi, n_docs = corpus
    rng = np.random.default_rng(2)
    dead = np.zeros((n_docs + 31) // 32, np.uint32)
    killed = rng.choice(n_docs, size=n_docs // 5, replace=False)
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    qs = queries(m, seed=13)
    check(orc, dev, hi, qs, dead=dead)
    check(orc, dev, hi, qs, rowid_base=3 * 65536 + 17)


def test_rank_none_and_field_limited_members(orc, dev, corpus):
    """Owners whose members differ in kind: SPH_RANK_NONE (counted off the match words), field limits on one or both keywords."""
    m, ctx, batch = dev
    hi, _ = corpus
    qs = []
    for a in range(6):
        for b in range(a + 1, 7):
            kind = (a + b) % 3
            qs.append(AND(m, a, b, ranker=m.SPH_RANK_NONE if kind == 0 else m.SPH_RANK_BM25, mask=(0xFFFFFFFF, 0xFFFFFFFF) if kind < 2 else (1 + a % 7, 6),
                          k=(3, 100, 1000)[b % 3]))
    qs += [AND(m, 1, 0, ranker=m.SPH_RANK_NONE, mask=(5, 0xFFFFFFFF)), AND(m, 8, 7, mask=(2, 2))]
    check(orc, dev, hi, qs)
    check(orc, dev, hi, qs, group=0)


def test_reused_batch_with_changing_groupings_and_placements(orc, dev, corpus):
    """One batch, submits whose groups and dispatch orders differ (sizes, classes, a lone query, the modes in turn), forwards and back."""
    m, ctx, batch = dev
    hi, _ = corpus
    rng = np.random.default_rng(4)
    sets = [sized_groups(m), [AND(m, 5, 6)], mixed(m, rng, 90), [AND(m, 0, 1), AND(m, 1, 0)], mixed(m, rng, 25)]
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    try:
        want = [[to_orc(orc, q).run(oi) for q in qs] for qs in sets]
        step = 0
        for order in (range(len(sets)), reversed(range(len(sets)))):
            for s in order:
                ctx.set("bm_place", MODES[step % 3])
                ctx.set("bm_group", 0 if step % 4 == 3 else 1)
                step += 1
                got = batch.search(seg, sets[s])
                for i, g in enumerate(got):
                    same(g, want[s][i], ("set", s, "step", step, i))
    finally:
        ctx.set("bm_place", 2)
        ctx.set("bm_group", 1)
        seg.close()


def test_candidate_overflow_is_rerun(orc, dev):
    """Every doc holds all three keywords with one weight: nothing prunes, the candidate lists overflow whatever the dispatch order,
    and each query is rerun alone (a one-query launch: no placement) with a full-size list."""
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
        want = [to_orc(orc, q).run(oi) for q in qs[:2]]
        runs = run_modes(dev, seg, qs)
        for mode, got, st in runs:
            assert st["n_rerun"] > 0, (mode, st)
            for i, q in enumerate(qs):
                g = got[i]
                assert g.total_found == n_docs and list(g.rowid) == list(range(q.max_matches)), (mode, i)
                same(g, runs[-1][1][i], ("bm_place", mode, "vs bm_place=0", i))
                if i < 2:
                    same(g, want[i], ("bm_place", mode, "vs oracle", i))
    finally:
        seg.close()


def test_one_query_launch_runs_no_placement(orc, dev, corpus):
    m, ctx, batch = dev
    hi, _ = corpus
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    try:
        q = AND(m, 0, 1)
        for mode in MODES:
            ctx.set("bm_place", mode)
            got = batch.search(seg, [q])
            st = batch.stats()
            assert st["n_items_bm"] == 5, st  # 74 windows in pieces of 16
            assert st["bm_owner_keys"] == 0 and st["bm_class_keys"] == 0, st
            same(got[0], to_orc(orc, q).run(oi), ("one query, bm_place", mode))
    finally:
        ctx.set("bm_place", 2)
        seg.close()


def test_short_launches_keep_the_layout_order(orc, dev, corpus):
    """bm_place_min_items: a launch of fewer work items is not placed (the default keeps launches of this corpus's size as laid out)."""
    m, ctx, batch = dev
    hi, _ = corpus
    qs = queries(m, seed=14)
    seg = m.Segment(ctx, hi)
    oi = orc_index_of(orc, hi)
    try:
        want = [to_orc(orc, q).run(oi) for q in qs]
        for least, placed in ((0, True), (1 << 20, False), (0, True)):
            ctx.set("bm_place_min_items", least)
            got = batch.search(seg, qs)
            st = batch.stats()
            assert (st["bm_owner_keys"] > 0) == placed and (st["bm_class_keys"] > 0) == placed, (least, st)
            for i in range(len(qs)):
                same(got[i], want[i], ("bm_place_min_items", least, i))
    finally:
        ctx.set("bm_place_min_items", 0)
        seg.close()
