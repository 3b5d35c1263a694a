"""GPU: grouped queries (Query.group) answered across segments and shards through the GROUP rows (MRK_GROW_WORDS).  The yardstick is
ONE grouping sorter fed with the matches of all segments: the merge of the shards' exported rows (mrk_topk_merge_grows) must equal,
word for word, the row the unsharded device run exports, group_expect's model over the whole match set, and the numpy mirror
(dist.merge_grows_np) -- zero padding included, into buffers pre-filled with 0xEE.  The limit (4 * max_matches distinct values) is
counted over ALL lists; what cannot be answered is MRK_ROW_DECLINED, never a truncated answer.  Every comparison is exact, and no
case is skipped because the model declines unless the test designates the decline."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import group_merge_common as gmc
from group_expect import GROUPSORT_COUNT, GROUPSORT_KEY, GROUPSORT_WEIGHT
from helpers import synth_postings
from test_gpu_group import AUX, BITS, C2, C16, C17, C64, C65, N_DOCS, ORDERS, PROBS, STRIDE, Q, Settings, make_rows, scr, shapes
from test_gpu_order_merge import Hip
from test_gpu_parity import orc_index_of
from test_gpu_sort_merge import L, off

pytestmark = pytest.mark.gpu

CUTS = {1: [0, N_DOCS], 2: [0, 4001, N_DOCS], 3: [0, 2000, 6001, N_DOCS], 8: [0, 1100, 2300, 3400, 4600, 5700, 6800, 7900, N_DOCS]}
RW, G = gmc.WORDS, gmc.G
# columns of the limit test's rows: per-shard disjoint values (values per shard of the 3-way cut; of the 8-way cut), and one column
# with the same 8 values, equally often, in every shard
D16, D17, D4, D5, D8, D9, D4096, D4097, SAME8 = range(9)
PER3 = {D16: (6, 5, 5), D17: (6, 6, 5), D4: (2, 1, 1), D5: (2, 2, 1), D8: (3, 3, 2), D9: (3, 3, 3)}


def disjoint_rows():
    rows = np.zeros((N_DOCS, STRIDE), np.uint32)
    r = np.arange(N_DOCS, dtype=np.uint64)
    for col, per in PER3.items():
        for s, (lo, hi) in enumerate(zip(CUTS[3][:-1], CUTS[3][1:])):
            rows[lo:hi, col] = scr(s * 100000 + r[lo:hi] % per[s])
    for col, extra in ((D4096, 0), (D4097, 1)):
        for s, (lo, hi) in enumerate(zip(CUTS[8][:-1], CUTS[8][1:])):
            rows[lo:hi, col] = scr(s * 100000 + r[lo:hi] % (512 + (extra if s == 5 else 0)))
    rows[:, SAME8] = scr(r % 8)
    return rows


class Corpus:
    """One corpus of N_DOCS docs, whole and cut into rowid-range shards (rowid_base), the attribute rows sliced at the same cuts"""

    def __init__(self, m, ctx, orc, n_fields, rows, layouts, seed=5):
        rng = np.random.default_rng(seed + n_fields)
        W, R, H = synth_postings(rng, N_DOCS, PROBS, n_fields=n_fields, max_pos=6)
        self.m, self.ctx, self.rows, self.n_docs, self.layouts = m, ctx, rows, N_DOCS, layouts
        idx = lambda sel, lo, n: m.index_from_hits(W[sel], R[sel] - np.uint32(lo), H[sel], n_terms=len(PROBS), total_docs=n, n_fields=n_fields)
        self.whole_hi = idx(slice(None), 0, N_DOCS)
        self.gdocs = {t: int(self.whole_hi.dict[t]["docs"]) for t in range(len(PROBS))}
        self.segs = {}
        for n in layouts:
            cuts = CUTS[n]
            self.segs[n] = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                seg = m.Segment(ctx, idx((R >= lo) & (R < hi), lo, hi - lo), rowid_base=lo)
                seg.set_attrs(np.ascontiguousarray(rows[lo:hi]))
                self.segs[n].append(seg)
        self.whole = self.segs[1][0]
        self.oi = orc_index_of(orc, self.whole_hi)
        self.oi.attrs = rows
        self.cache = {}

    def globalize(self, q):
        return dataclasses.replace(q, total_docs=self.n_docs, local_docs=dict(self.gdocs))

    def matches(self, orc, q):
        key = (repr(q.root), q.ranker, q.group.bit_offset, q.group.bit_count, q.index_weight)
        if key not in self.cache:
            self.cache[key] = gmc.whole_matches(orc, self.oi, q, self.rows, self.n_docs)
        return self.cache[key]

    def close(self):
        for segs in self.segs.values():
            for s in segs:
                s.close()


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    hip = Hip()
    yield m, ctx, batch, hip
    hip.free()
    batch.close()
    ctx.close()


@pytest.fixture(scope="module")
def corpora(orc, dev):
    m, ctx, _, _ = dev
    cs = {4: Corpus(m, ctx, orc, 4, make_rows(N_DOCS), (1, 2, 3, 8)), 17: Corpus(m, ctx, orc, 17, make_rows(N_DOCS), (1, 2, 3, 8))}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def limits(orc, dev):
    m, ctx, _, _ = dev
    c = Corpus(m, ctx, orc, 4, disjoint_rows(), (1, 3, 8), seed=11)
    yield c
    c.close()


def export(batch, hip, segs, qs, dst=None, want_status=None):
    """every segment's group rows of the batch, exported behind mrk_batch_wait -> device [S][nq][GROW_WORDS] pre-filled with 0xEE"""
    nq, S = len(qs), len(segs)
    dst = dst or hip.malloc(S * nq * RW * 8)
    hip.fill(dst, 0xEE, S * nq * RW * 8)
    for s, seg in enumerate(segs):
        batch.submit(seg, qs)
        batch.wait()
        assert batch.stats()["packed"] == 1
        if want_status is not None:
            assert [r.status for r in batch.results()] == want_status[s], ("shard", s)
        batch.export_grows(dst.value + s * nq * RW * 8)
    return dst


def merge(ctx, hip, rows_all, n_lists, nq, k=1024):
    lib, chk = L()
    out = hip.malloc(nq * RW * 8)
    hip.fill(out, 0xEE, nq * RW * 8)
    chk(lib.mrk_topk_merge_grows(ctx._h, rows_all, n_lists, nq, k, out))
    return hip.to_host(out, (nq, RW))


@pytest.mark.parametrize("n_fields", [4, 17])
def test_sharded_equals_unsharded_equals_model(orc, dev, corpora, n_fields):
    """1, 2, 3 and 8 lists; all seven shapes under all six orders; columns at, under and over their limit"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    c = corpora[n_fields]
    cols = [(C64, 32, 0, 16, True), (C16, 32, 0, 4, True), (C2, 32, 0, 1000, True), (BITS, 7, 9, 32, True), (C65, 32, 0, 16, False), (C17, 32, 0, 1024, True)]
    qs, must = [], []
    for si, sh in enumerate(shapes(m)):
        for oi_, (by, desc) in enumerate(ORDERS):
            col, bits, shift, K, ok = cols[(si + oi_) % len(cols)]
            qs.append(c.globalize(Q(m, sh, col, bits=bits, shift=shift, K=K, by=by, desc=desc, index_weight=1 + (si + oi_) % 2 * 2)))
            must.append(ok if sh in ("one", "none") or ok else None)  # (keyword 0 is in every doc: every value of the column matches)
    nq = len(qs)
    whole = hip.to_host(export(batch, hip, [c.whole], qs), (1, nq, RW))[0]
    n_decl = 0
    for qi, q in enumerate(qs):
        n_decl += gmc.check_merged(mdist, q, c.matches(orc, q), whole[qi], ("unsharded", n_fields, qi), must[qi])
    assert n_decl >= 2 and n_decl == sum(int(r[gmc.TOTAL]) == gmc.DECLINED for r in whole)
    for S in (1, 2, 3, 8):
        dev_rows = export(batch, hip, c.segs[S], qs)
        lists = hip.to_host(dev_rows, (S, nq, RW))
        got = merge(ctx, hip, dev_rows, S, nq)
        assert np.array_equal(got, mdist.merge_grows_np(lists, 1024)), ("kernel != numpy mirror", S)
        assert np.array_equal(got, whole), ("merged != the unsharded row", S, [qi for qi in range(nq) if not np.array_equal(got[qi], whole[qi])][:5])
        hip.free()


def limit_queries(m, c):
    cases = [(D16, 4, True), (D17, 4, False), (D4, 1, True), (D5, 1, False), (D8, 2, True), (D9, 2, False)]
    qs = [c.globalize(Q(m, sh, col, K=K, by=by)) for col, K, _ in cases for sh, by in (("one", GROUPSORT_COUNT), ("none", GROUPSORT_KEY))]
    return qs, [ok for _, _, ok in cases for _ in range(2)]


def test_limit_edges_with_shard_disjoint_values(orc, dev, limits):
    """the values of a column depend on the shard, so no single list decides: 6 + 5 + 5 = 16 answer at K = 4, 6 + 6 + 5 = 17 decline;
    K = 1 and K = 2 (tables of 16 and 32 slots) at 4 / 5 and 8 / 9; K = 1024: 8 lists x 512 = 4096, the full-size sort, and one more"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    c = limits
    qs, must = limit_queries(m, c)
    nq = len(qs)
    dev_rows = export(batch, hip, c.segs[3], qs, want_status=[[0] * nq] * 3)
    lists = hip.to_host(dev_rows, (3, nq, RW))
    assert not (lists[:, :, gmc.TOTAL] & np.uint64(gmc.RERUN | gmc.DECLINED)).any(), "every list alone is inside its limit"
    got = merge(ctx, hip, dev_rows, 3, nq)
    assert np.array_equal(got, mdist.merge_grows_np(lists, 1024))
    for qi, q in enumerate(qs):
        assert gmc.check_merged(mdist, q, c.matches(orc, q), got[qi], ("limit", qi), must[qi]) == (not must[qi])
    assert [int(x) for x in got[::2, gmc.TOTAL]] == [16, gmc.DECLINED, 4, gmc.DECLINED, 8, gmc.DECLINED]
    whole = hip.to_host(export(batch, hip, [c.whole], qs), (nq, RW))
    assert np.array_equal(got, whole), "the unsharded run answers and declines the same"
    hip.free()
    big = [c.globalize(Q(m, "one", D4096, K=1024, by=GROUPSORT_COUNT, desc=False)), c.globalize(Q(m, "one", D4097, K=1024)), c.globalize(Q(m, "none", D4096, K=1024, by=GROUPSORT_WEIGHT))]
    dev_rows = export(batch, hip, c.segs[8], big, want_status=[[0] * 3] * 8)
    lists = hip.to_host(dev_rows, (8, 3, RW))
    assert [int(x) for x in lists[:, 0, gmc.TOTAL]] == [512] * 8 and sorted(int(x) for x in lists[:, 1, gmc.TOTAL]) == [512] * 7 + [513]
    got = merge(ctx, hip, dev_rows, 8, 3)
    assert np.array_equal(got, mdist.merge_grows_np(lists, 1024))
    for qi, ok in enumerate((True, False, True)):
        assert gmc.check_merged(mdist, big[qi], c.matches(orc, big[qi]), got[qi], ("4096", qi), ok) == (not ok)
    assert int(got[0, gmc.CNT]) == 4096 and int(got[2, gmc.TOTAL]) == 4096
    hip.free()


def test_the_same_values_in_every_list(orc, dev, limits):
    """counts add up to the unsharded count; SPH_RANK_NONE: every weight is equal, so the head is the lowest GLOBAL rowid across
    shards, and under the head-weight and @count orders every part ties: the groups leave by head rowid"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    c = limits
    qs = [c.globalize(Q(m, "none", SAME8, K=K, by=by, desc=desc)) for by in (GROUPSORT_WEIGHT, GROUPSORT_COUNT, GROUPSORT_KEY) for desc in (True, False) for K in (2, 20)]
    nq = len(qs)
    for S in (3, 8):
        dev_rows = export(batch, hip, c.segs[S], qs, want_status=[[0] * nq] * S)
        lists = hip.to_host(dev_rows, (S, nq, RW))
        got = merge(ctx, hip, dev_rows, S, nq)
        assert np.array_equal(got, mdist.merge_grows_np(lists, 1024))
        for qi, q in enumerate(qs):
            assert not gmc.check_merged(mdist, q, c.matches(orc, q), got[qi], ("same", S, qi), True)
            rowid, weight, key, cnt, total = mdist.grow_groups(got[qi])
            per_list = sum((lists[s, qi, gmc.PLANE:gmc.PLANE + 8] & np.uint64(0xFFFFFFFF)).astype(np.int64).sum() for s in range(S))
            assert total == 8 and (cnt == N_DOCS // 8).all() and per_list == N_DOCS and (weight == 1).all()
            if q.group.sort_by != GROUPSORT_KEY:
                assert rowid.tolist() == list(range(min(8, q.max_matches))), ("ties leave by head rowid", qi, rowid)
        hip.free()


def test_associativity_of_staged_merges(dev, limits):
    """merge(merge(A, B), C) == merge(A, B, C) word for word; D17 and D5 are declined only at the last step"""
    m, ctx, batch, hip = dev
    c = limits
    qs, must = limit_queries(m, c)
    qs += [c.globalize(Q(m, "and2", SAME8, K=3, by=GROUPSORT_COUNT)), c.globalize(m.Query(shapes(m)["and2"][0], ranker=m.SPH_RANK_BM25, max_matches=50))]
    nq = len(qs)
    dev_rows = export(batch, hip, c.segs[3], qs)
    one_step = merge(ctx, hip, dev_rows, 3, nq)
    ab = merge(ctx, hip, dev_rows, 2, nq)
    assert not (ab[:, gmc.TOTAL] & np.uint64(gmc.RERUN | gmc.DECLINED)).any(), "the first step answers every query"
    assert int(ab[2, gmc.TOTAL]) == 12 and int(one_step[2, gmc.TOTAL]) == gmc.DECLINED, "17 values: declined at the last step only"
    stage = hip.malloc(2 * nq * RW * 8)
    hip.to_dev(stage, ab)
    hip.d2d(off(stage, nq * RW * 8), off(dev_rows, 2 * nq * RW * 8), nq * RW * 8)
    assert np.array_equal(merge(ctx, hip, stage, 2, nq), one_step)
    bc = merge(ctx, hip, off(dev_rows, nq * RW * 8), 2, nq)  # A + (B + C)
    hip.to_dev(off(stage, nq * RW * 8), bc)
    hip.d2d(stage, dev_rows, nq * RW * 8)
    assert np.array_equal(merge(ctx, hip, stage, 2, nq), one_step)
    hip.free()


def test_mixed_batch_and_the_partitioned_form(orc, dev, corpora):
    """relevance queries between grouped ones come out as the narrow merge gives them; sort and order queries leave declined; the
    _part form writes its own rows only"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    c = corpora[4]
    root2, prox = shapes(m)["and2"][0], shapes(m)["prox2"][0]
    rel = [m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10), m.Query(shapes(m)["one"][0], ranker=m.SPH_RANK_BM25, max_matches=1024),
           m.Query(prox, ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=7)]
    srt = m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10, sort=m.Sort(C64 * 32, 32))
    odr = m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10, order=m.Order([m.OrderPart(C16 * 32, 32), m.OrderPart(AUX * 32, 32, desc=False)]))
    qs = [c.globalize(q) for q in (Q(m, "and2", C64, K=16, by=GROUPSORT_COUNT), rel[0], srt, Q(m, "prox2", C16, K=8), rel[1], odr, Q(m, "one", C17, K=4), rel[2])]
    nq, S = len(qs), 3
    dev_rows = export(batch, hip, c.segs[S], qs)
    lists = hip.to_host(dev_rows, (S, nq, RW))
    got = merge(ctx, hip, dev_rows, S, nq)
    assert np.array_equal(got, mdist.merge_grows_np(lists, 1024))
    for qi in (0, 3):
        assert not gmc.check_merged(mdist, qs[qi], c.matches(orc, qs[qi]), got[qi], ("mixed", qi), True)
    assert gmc.check_merged(mdist, qs[6], c.matches(orc, qs[6]), got[6], ("mixed", 6), False)
    for qi in (2, 5):  # no list holds an order for them: declined, spec 0, in every list and merged
        for row in list(lists[:, qi]) + [got[qi]]:
            assert int(row[gmc.TOTAL]) == gmc.DECLINED and int(row[gmc.CNT]) == 0 and int(row[gmc.SPEC]) == 0 and not row[:G].any() and not row[gmc.PLANE:].any()
    # the relevance queries: words [0, K1), count and total as mrk_topk_merge_rows merges the same batch's narrow rows
    NW = m.ROW_WORDS
    narrow = hip.malloc(S * nq * NW * 8)
    for s, seg in enumerate(c.segs[S]):
        batch.submit(seg, qs)
        batch.wait()
        chk(lib.mrk_batch_export_rows(batch._h, C.c_void_p(narrow.value + s * nq * NW * 8)))
    nout = hip.malloc(nq * NW * 8)
    chk(lib.mrk_topk_merge_rows(ctx._h, narrow, S, nq, 1024, nout))
    nhost = hip.to_host(nout, (nq, NW))
    for qi in (1, 4, 7):
        assert np.array_equal(got[qi, :1024], nhost[qi, :1024]) and got[qi, gmc.CNT] == nhost[qi, 1024] and got[qi, gmc.TOTAL] == nhost[qi, 1025], qi
        assert int(got[qi, gmc.CNT]) == min(1024, int(lists[:, qi, gmc.CNT].sum())) >= qs[qi].max_matches and int(got[qi, gmc.SPEC]) == 0 and not got[qi, 1024:G].any() and not got[qi, gmc.PLANE:].any()
    # _part: lists of stride nq, queries [2, 7) of each -> out rows [1, 6); every other row stays 0xEE
    out = hip.malloc((nq + 1) * RW * 8)
    hip.fill(out, 0xEE, (nq + 1) * RW * 8)
    chk(lib.mrk_topk_merge_grows_part(ctx._h, off(dev_rows, 2 * RW * 8), S, nq, 1, 5, 1024, out))
    part = hip.to_host(out, (nq + 1, RW))
    assert np.array_equal(part[1:6], got[2:7])
    assert (part[0] == np.uint64(0xEEEEEEEEEEEEEEEE)).all() and (part[6:] == np.uint64(0xEEEEEEEEEEEEEEEE)).all()
    hip.free()


def test_flags_whichever_list_carries_the_fault(dev, limits):
    """a list with RERUN, one with DECLINED, a hostile entry count, a spec word nobody writes: the same merged row whichever list it
    is; spec mismatches (sort_by, desc, K), a grouped list next to a spec-0 one, a max_matches above the call's k, counts past 2^32 - 1"""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    c = limits
    q = c.globalize(Q(m, "one", D16, K=4, by=GROUPSORT_WEIGHT, desc=False))
    relq = c.globalize(m.Query(shapes(m)["one"][0], ranker=m.SPH_RANK_BM25, max_matches=5))
    dev_rows = export(batch, hip, c.segs[3], [q, relq])
    base = hip.to_host(dev_rows, (3, 2, RW))
    spec, R, D = gmc.spec_of(q), gmc.RERUN, gmc.DECLINED
    good = merge(ctx, hip, dev_rows, 3, 2)
    assert int(good[0, gmc.TOTAL]) == 16 and int(good[0, gmc.SPEC]) == spec
    buf = hip.malloc(3 * 2 * RW * 8)

    def run(rows, k=1024):
        hip.to_dev(buf, rows)
        got = merge(ctx, hip, buf, 3, 2, k)
        assert np.array_equal(got, mdist.merge_grows_np(rows, k))
        assert k != 1024 or np.array_equal(got[1], good[1]), "the batch's other query is untouched"
        return got[0]

    def empty(row, flags, sp=spec):
        return int(row[gmc.TOTAL]) == flags and int(row[gmc.CNT]) == 0 and int(row[gmc.SPEC]) == sp and not row[:G].any() and not row[gmc.PLANE:gmc.SPEC].any()

    def rerun(row):
        row[:gmc.CNT + 1], row[gmc.PLANE:gmc.SPEC], row[gmc.TOTAL] = 0, 0, R

    def declined(row):
        row[:], row[gmc.TOTAL] = 0, D

    def too_many(row):
        row[gmc.CNT] = G + 1

    def huge(row):
        row[gmc.CNT] = 0xFFFFFFFFFFFFFFFF

    def bad_spec(row):
        row[gmc.SPEC] = spec | (1 << 40)

    for fault, flags in ((rerun, R), (declined, D), (too_many, D), (huge, D), (bad_spec, D)):
        got = []
        for l in range(3):
            rows = base.copy()
            fault(rows[l, 0])
            got.append(run(rows))
        assert empty(got[0], flags) and np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), fault.__name__
    rows = base.copy()
    rerun(rows[0, 0]), declined(rows[2, 0])
    assert empty(run(rows), R | D)
    for other in (mdist.group_spec_word(GROUPSORT_COUNT, 0, 32, 4), mdist.group_spec_word(GROUPSORT_WEIGHT, 1, 32, 4), mdist.group_spec_word(GROUPSORT_WEIGHT, 0, 32, 5)):
        for l in range(3):
            rows = base.copy()
            rows[l, 0, gmc.SPEC] = other
            assert empty(run(rows), D, other if l == 0 else spec), (hex(other), l)
    rows = base.copy()
    rows[1, 0] = base[1, 1]  # a relevance row among the grouped ones
    assert empty(run(rows), D)
    assert empty(run(base.copy(), k=3), D), "max_matches above the call's k"
    # counts: a sum of exactly 2^32 - 1 is a count; one more declines -- never wrapped, never saturated
    rows = base.copy()
    v = int(rows[0, 0, gmc.PLANE]) >> 32
    rows[0, 0, gmc.PLANE] = (v << 32) | 0xFFFFFFFE
    rows[1, 0, gmc.PLANE] = (v << 32) | 1  # (list 1's first group now adds to list 0's: 6 + 4 + 5 values)
    got = run(rows)
    assert int(got[gmc.TOTAL]) == 15 and ((v << 32) | 0xFFFFFFFF) in [int(x) for x in got[gmc.PLANE:gmc.PLANE + 15]]
    rows[1, 0, gmc.PLANE] += np.uint64(1)
    assert empty(run(rows), D), "a count of 2^32"
    hip.free()


def test_a_rerun_leaves_with_its_repaired_groups(orc, dev):
    """test_gpu_group's overflow setup: the match queue overflows, mrk_batch_wait reruns each query alone over the retry batch's
    table; the row exported after the wait equals the row of a run that did not overflow"""
    m, ctx, batch, hip = dev
    n_docs = 200_000
    hi = m.synth_index(n_docs, [1.0, 0.9, 0.8], seed=31, skiplist_block_size=128, max_pos=12)
    rows = make_rows(n_docs)
    seg = m.Segment(ctx, hi, rowid_base=1000)
    try:
        seg.set_attrs(rows)
        hits = [Q(m, "prox2", C16, K=8, by=GROUPSORT_COUNT), Q(m, "phrase", C64, K=100), Q(m, "sph04_3", C2, K=2), Q(m, "prox2", C17, K=4),
                m.Query(shapes(m)["prox2"][0], ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=9)]
        with Settings(ctx, mq_max_chunks=1):
            a = hip.to_host(export(batch, hip, [seg], hits, want_status=[[0, 0, 0, -2, 0]]), (len(hits), RW))
            assert batch.stats()["n_rerun"] > 0
        b = hip.to_host(export(batch, hip, [seg], hits, want_status=[[0, 0, 0, -2, 0]]), (len(hits), RW))
        assert batch.stats()["n_rerun"] == 0
        assert np.array_equal(a, b)
        assert not (b[[0, 1, 2, 4], gmc.TOTAL] & np.uint64(gmc.RERUN | gmc.DECLINED)).any() and b[:3, gmc.CNT].all()
        assert int(b[3, gmc.TOTAL]) == gmc.DECLINED and int(b[3, gmc.SPEC]) == gmc.spec_of(hits[3]) and int(b[0, gmc.TOTAL]) == 16
    finally:
        seg.close()
        hip.free()


@pytest.mark.parametrize("part", [1, 0])
def test_shard_exchange_grows_one_rank(part):
    """mrk_shard_exchange_grows at world_size 1 over RCCL (exchange_self_rccl), partitioned and all-gather, in a fresh process"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(here, "dist_group_exchange_worker.py"), str(part)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "group exchange ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
