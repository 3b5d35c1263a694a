"""GPU: GROUP BY a multi-value attribute (Group(mva_bits=32, ...); mrk_batch_submit_mva) against group_mva_expect -- the numpy model of
MVAGroupSorter_T::Push over the oracle's full match set and the blob pool, itself pinned on the reference's recorded results
(tests/test_group_mva_cpu.py).  Every comparison is bit for bit: head rowid, head weight, group key, @count, total_found, order.
A query whose model answer is DECLINED (more than 4 * max_matches distinct values) must come back MRK_E_UNSUPPORTED; any other
decline is a failure, and every case asserts that it is what the test designates (check(..., must=)).

Rows (dwords): a constant; rowid % 10; the blob row's offset (2, 3); 16 scrambled values (a row attribute to group by); rowid % 70.
MVAs: the number of values per doc cycles by rowid over 0, 1, 2, 3, 63, 64, 65 (63 / 64 values straddle the 1- / 2-byte length class
where the MVA is the row's only blob attribute), drawn from a domain of D values that holds 0 and 0xFFFFFFFF, in an order that is
not sorted and with a value stored twice on every fifth doc."""
import dataclasses

import numpy as np
import pytest

import group_mva_expect as gme
from group_expect import DECLINED, GROUPSORT_COUNT, GROUPSORT_KEY, GROUPSORT_WEIGHT, expected_group
from helpers import build_blob_pool, synth_postings
from test_gpu_group import E_UNSUPPORTED, N_DOCS, ORDERS, PROBS, Settings, last_error, scr, shapes
from test_gpu_parity import orc_index_of, to_orc

pytestmark = pytest.mark.gpu

C1, AUX, BLOB, BLOB_HI, C16, M70 = range(6)
STRIDE = 6
CYCLE = (0, 1, 2, 3, 63, 64, 65)
CUTS = [0, 2000, 6001, N_DOCS]


def domain(D):
    return np.concatenate([np.array([0, 0xFFFFFFFF], np.uint32), scr(np.arange(D - 2, dtype=np.uint64))])[:D]


def cycle_values(D, mult=7):
    dom = domain(D)

    def f(r):
        n = CYCLE[r % 7]
        v = dom[(r * mult + np.arange(n) * 13) % D]
        if n >= 2 and r % 5 == 0:
            v[1] = v[0]
        return v
    return f


def const_values(*by_row, default=()):
    table = dict(by_row)
    return lambda r: np.array(table.get(r, default), np.uint32)


def u32(v):
    return np.asarray(v, "<u4").tobytes()


def make_rows(n_docs):
    r = np.arange(n_docs, dtype=np.uint64)
    rows = np.zeros((n_docs, STRIDE), np.uint32)
    rows[:, C1], rows[:, AUX], rows[:, C16], rows[:, M70] = 7, (r % 10).astype(np.uint32), scr(r % 16), (r % 70).astype(np.uint32)
    return rows


class Index:
    """the postings of one corpus, shared by its segments"""

    def __init__(self, m, orc, n_fields, seed=5):
        rng = np.random.default_rng(seed + n_fields)
        self.W, self.R, self.H = synth_postings(rng, N_DOCS, PROBS, n_fields=n_fields, max_pos=6)
        self.m, self.n_fields = m, n_fields
        self.hi = self.cut(0, N_DOCS)
        self.oi = orc_index_of(orc, self.hi)
        self.gdocs = {t: int(self.hi.dict[t]["docs"]) for t in range(len(PROBS))}

    def cut(self, lo, hi):
        sel = (self.R >= lo) & (self.R < hi)
        return self.m.index_from_hits(self.W[sel], self.R[sel] - np.uint32(lo), self.H[sel], n_terms=len(PROBS), total_docs=hi - lo, n_fields=self.n_fields)


class Corpus:
    """a segment over an Index whose blob rows hold len(attrs) blob attributes: attrs[a](r) = the bytes of attribute a of row r"""

    def __init__(self, m, ctx, ix, attrs, rowid_base=0):
        self.ix, self.n_docs, self.n_blob = ix, N_DOCS, len(attrs)
        self.rows = make_rows(N_DOCS)
        self.pool, offs = build_blob_pool([[bytes(a(r)) for a in attrs] for r in range(N_DOCS)])
        self.rows[:, BLOB] = np.array(offs, np.uint64).astype(np.uint32)
        self.seg = m.Segment(ctx, ix.hi, rowid_base=rowid_base)
        self.seg.set_attrs(self.rows)
        self.seg.set_blobs(self.pool, self.n_blob, self.rows)
        self.oi = ix.oi
        self.values, self.cache = {}, {}

    def bind(self):
        """the shared oracle index reads THIS corpus's rows and pool"""
        self.oi.attrs, self.oi.blobs, self.oi.dead_rows = self.rows, self.pool, None

    def values_of(self, blob_id):
        if blob_id not in self.values:  # (read from the pool by the model's own reader, once per row)
            self.values[blob_id] = [gme.mva_values(self.pool, int(self.rows[r, BLOB]), blob_id, self.n_blob) for r in range(self.n_docs)]
        return self.values[blob_id]

    def close(self):
        self.seg.close()


def mva_of(fn):
    return lambda r: u32(fn(r))


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    yield m, ctx, batch
    batch.close()
    ctx.close()


@pytest.fixture(scope="module")
def indexes(orc, dev):
    m, _, _ = dev
    return {4: Index(m, orc, 4), 17: Index(m, orc, 17)}


# blob attributes of the `many` corpus
A_D4, A_D8, A_TIES, A_EXTRA, A_ALONE, A_ALL65, A_EMPTY63 = range(7)
TIE_LO, TIE_HI, TIE_OTHER = 2, 8, 5


def many_attrs():
    d4 = domain(4)
    # 2 and 8 are carried by exactly the same docs (so they share count and head); 5 by other docs (so it never joins their tie)
    ties = lambda r: np.array([[TIE_HI, TIE_LO], [TIE_LO, TIE_HI], [TIE_OTHER], [TIE_OTHER]][r % 4], np.uint32)
    extra = lambda r: np.array([77], np.uint32) if r == 4500 else d4[(r + np.arange(CYCLE[r % 7])) % 4]        # a fifth value on one other doc
    alone = const_values((4500, [10, 0xFFFFFFFF, 0, 30, 20]))                                                   # one doc carries five values alone
    all65 = lambda r: d4[(r + np.arange(65)) % 4]                                                               # every buffer expands 65-fold
    empty63 = lambda r: np.zeros(0, np.uint32) if r % 70 == 63 else np.array([r % 3], np.uint32)
    return [mva_of(f) for f in (cycle_values(4), cycle_values(8), ties, extra, alone, all65, empty63)]


@pytest.fixture(scope="module")
def corpora(dev, indexes):
    m, ctx, _ = dev
    cs = {"d80": Corpus(m, ctx, indexes[4], [mva_of(cycle_values(80))]),  # the MVA is the row's only blob attribute
          "many": Corpus(m, ctx, indexes[4], many_attrs()),
          "w80": Corpus(m, ctx, indexes[17], [mva_of(cycle_values(80))])}
    yield cs
    for c in cs.values():
        c.close()


def QM(m, shape, K=20, by=GROUPSORT_KEY, desc=True, blob_id=0, n_blob=1, **kwa):
    root, ranker = shapes(m)[shape]
    return m.Query(root, ranker=ranker, max_matches=K, group=m.Group(0, 0, sort_by=by, desc=desc, mva_bits=32, blob_attr_id=blob_id, n_blob_attrs=n_blob), **kwa)


def pushes(orc, c, q):
    """(rowid, weight, value) per push of query q, from the oracle's full match set and the pool"""
    key = (repr(q.root), q.ranker, q.index_weight, repr(q.filters), repr(q.weight_filters), q.group.blob_attr_id, q.total_docs)
    if key not in c.cache:
        full = gme.all_matches(orc, c.oi, dataclasses.replace(q, group=None), c.n_docs)
        vals = c.values_of(q.group.blob_attr_id)
        c.cache[key] = gme.expand(full.rowid, full.weight, lambda r: vals[r])
    return c.cache[key]


def check(orc, c, queries, got, what="", must=None, cached=True):
    """must: per query True = the model must answer, False = must decline.  -> the number of declines"""
    c.bind()
    if not cached:
        c.cache = {}
    n_decl = 0
    for i, (q, g) in enumerate(zip(queries, got)):
        if q.group is None:
            want = to_orc(orc, q).run(c.oi)
            assert g.status == 0 and g.group_key is None and g.group_count is None, (what, i)
            assert g.total_found == want.total_found and np.array_equal(g.rowid, want.rowid) and np.array_equal(g.weight, want.weight), (what, i)
            continue
        if q.group.mva_bits:
            want = gme.expected_groups_mva(*pushes(orc, c, q), q.group.sort_by, bool(q.group.desc), q.max_matches)
        else:
            want = expected_group(orc, c.oi, q, c.rows, c.n_docs)
        if must is not None and must[i] is not None:
            assert (want is not DECLINED) == must[i], (what, i, "the case is not what the test designates")
        if want is DECLINED:
            n_decl += 1
            assert g.status == E_UNSUPPORTED and len(g.rowid) == 0 and g.total_found == 0 and g.group_key is None, (what, i, g.status)
            continue
        assert g.status == 0, (what, i, q.group, q.max_matches, "a device decline where the model answers")
        r, w, k, cnt, total = want
        assert g.total_found == total, (what, i, g.total_found, total)
        assert np.array_equal(g.group_key, k), (what, i, q.group, q.max_matches, g.group_key[:8], k[:8])
        assert np.array_equal(g.group_count, cnt), (what, i, g.group_count[:8], cnt[:8])
        assert np.array_equal(g.rowid, r), (what, i, g.rowid[:8], r[:8])
        assert np.array_equal(g.weight, w), (what, i, g.weight[:8], w[:8])
        assert g.sort_key is None and g.order_key is None
    return n_decl


SCAN_SHAPES, RANK_SHAPES = ("one", "and2", "tree"), ("phrase", "prox2")


@pytest.mark.parametrize("K", [1, 2, 20, 1024])
def test_orders_shapes_and_k(orc, dev, corpora, K):
    """all six orders x the shapes that take the scan's flush and the rank kernel's, the domain inside 4 K"""
    m, ctx, batch = dev
    c, blob_id = {1: (corpora["many"], A_D4), 2: (corpora["many"], A_D8), 20: (corpora["d80"], 0), 1024: (corpora["d80"], 0)}[K]
    qs = [QM(m, sh, K, by, desc, blob_id, c.n_blob) for sh in SCAN_SHAPES + RANK_SHAPES for by, desc in ORDERS]
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, f"orders K={K}", [True] * len(qs)) == 0
    assert batch.stats()["packed"] == 1
    assert got[0].total_found == {1: 4, 2: 8, 20: 80, 1024: 80}[K] and len(got[0].rowid) == min(K, got[0].total_found)  # (keyword 0 is in every doc)
    if K == 20:
        assert {0, 0xFFFFFFFF} <= set(got[0].group_key.tolist()) | set(got[1].group_key.tolist())  # keys 0 and 0xFFFFFFFF: first under desc, under asc


def test_wide_segment(orc, dev, corpora):
    """17 fields: the instances of the packed-mask path"""
    m, ctx, batch = dev
    c = corpora["w80"]
    qs = [QM(m, sh, 20, by, desc) for sh in SCAN_SHAPES + RANK_SHAPES for by, desc in ORDERS]
    assert check(orc, c, qs, batch.search(c.seg, qs), "wide", [True] * len(qs)) == 0


def test_ties_leave_by_the_smaller_value(orc, dev, corpora):
    """two values carried by exactly the same docs tie under @count and under the head's weight, in both directions: the smaller value
    first, whatever desc says; K = 1 or 2 cuts between the two, K = 20 is above them"""
    m, ctx, batch = dev
    c = corpora["many"]
    qs = [QM(m, sh, K, by, desc, A_TIES, c.n_blob) for sh in ("one", "prox2") for by in (GROUPSORT_COUNT, GROUPSORT_WEIGHT) for desc in (True, False) for K in (1, 2, 20)]
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, "ties", [True] * len(qs)) == 0
    n_cut = 0
    for q, g in zip(qs, got):
        assert gme.has_tie(*pushes(orc, c, q), q.group.sort_by, bool(q.group.desc))
        keys = g.group_key.tolist()
        assert g.total_found == 3 and TIE_LO in keys or keys == [TIE_OTHER]
        if TIE_HI in keys:
            assert keys.index(TIE_LO) + 1 == keys.index(TIE_HI)
        elif TIE_LO in keys:
            n_cut += 1  # the cut fell between the two: the smaller value stayed
    assert n_cut == 8  # 2 and 8 are neighbours in every order, so of K = 1 and K = 2 exactly one cuts between them


def test_empty_mvas(orc, dev, corpora):
    m, ctx, batch = dev
    c = corpora["many"]
    only = [m.Filter(M70 * 32, 32, values=[63])]  # exactly the docs whose MVA is empty
    qs = [QM(m, sh, 20, GROUPSORT_COUNT, True, A_EMPTY63, c.n_blob, filters=only) for sh in ("one", "prox2")] + [QM(m, "one", 20, GROUPSORT_COUNT, True, A_EMPTY63, c.n_blob)]
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, "empty", [True] * 3) == 0
    for g in got[:2]:
        assert g.status == 0 and len(g.rowid) == 0 and g.total_found == 0 and g.group_key is not None and len(g.group_key) == 0
    assert got[2].total_found == 3


def test_the_limit(orc, dev, corpora):
    """exactly 4 K distinct values answer; one more declines -- on another doc, or with one doc carrying all 4 K + 1 alone; an
    expansion of 65 pairs per match (>= 64 rounds per full buffer) answers"""
    m, ctx, batch = dev
    c = corpora["many"]
    qs, must = [], []
    for sh in ("one", "prox2"):
        qs += [QM(m, sh, 1, GROUPSORT_COUNT, True, A_D4, c.n_blob), QM(m, sh, 2, GROUPSORT_KEY, False, A_D8, c.n_blob), QM(m, sh, 1, GROUPSORT_COUNT, True, A_ALL65, c.n_blob)]
        must += [True, True, True]
    qs += [QM(m, "one", 1, GROUPSORT_COUNT, True, A_D8, c.n_blob), QM(m, "one", 1, GROUPSORT_COUNT, True, A_EXTRA, c.n_blob), QM(m, "one", 1, GROUPSORT_KEY, True, A_ALONE, c.n_blob),
           QM(m, "one", 2, GROUPSORT_COUNT, True, A_EXTRA, c.n_blob), QM(m, "one", 2, GROUPSORT_COUNT, False, A_ALONE, c.n_blob)]
    must += [False, False, False, True, True]
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, "limit", must) == 3
    assert "distinct groups" in last_error() and "max_matches" in last_error()  # the run-time decline names the limit
    assert got[2].total_found == 4 and len(got[2].group_count) == 1 and 4 * int(got[2].group_count[0]) == 65 * N_DOCS  # keyword 0: every doc, 65 pushes, four values equally often
    assert got[-1].group_key.tolist() == [0, 10, 20, 30, 0xFFFFFFFF][:2] and got[-1].total_found == 5  # five groups of one doc: all tie, by value


@pytest.mark.parametrize("blob_id", [0, 1, 2])
def test_blob_attribute_position(orc, dev, indexes, blob_id):
    """the MVA as attribute 0, 1 and 2 of 3, next to a string of odd length and a 64-bit MVA; row 100 has a 70 000-byte string, so its
    blob row is in the 4-byte length class while its MVA has three values"""
    m, ctx, batch = dev
    vals, dom = cycle_values(80, mult=11), domain(80)
    mva = lambda r: u32(dom[[1, 0, 2]] if r == 100 else vals(r))
    string = lambda r: b"s" * (70000 if r == 100 else 1 + 2 * (r % 4))
    mva64 = lambda r: np.arange(r % 3, dtype="<i8").tobytes()
    attrs = [string, mva64]
    attrs.insert(blob_id, mva)
    c = Corpus(m, ctx, indexes[4], attrs)
    try:
        assert c.pool[int(c.rows[100, BLOB])] == 2 and c.pool[int(c.rows[101, BLOB])] in (0, 1)
        qs = [QM(m, sh, 20, by, True, blob_id, 3) for sh in ("one", "and2", "prox2") for by in (GROUPSORT_KEY, GROUPSORT_COUNT)]
        assert check(orc, c, qs, batch.search(c.seg, qs), f"position {blob_id}", [True] * len(qs)) == 0
    finally:
        c.close()


def test_in_front_of_the_sorter(orc, dev, corpora):
    """a row filter, an MVA ANY filter on the grouped attribute itself (the groups still come from ALL values of a passing doc), a weight
    filter, dead rows and index_weight: rejected matches are absent from the counts"""
    m, ctx, batch = dev
    c = corpora["d80"]
    dom = domain(80)
    flt = [m.Filter(AUX * 32, 32, values=[1, 3, 5, 7, 8])]
    anyf = [m.Filter(0, 0, values=[int(dom[3]), int(dom[40])], mva_bits=32, blob_attr_id=0, n_blob_attrs=1)]
    wf = [m.Filter(0, 0, min=1600, max=1 << 30)]
    qs = []
    for sh in ("one", "and2", "tree", "prox2", "phrase"):
        qs += [QM(m, sh, 20, GROUPSORT_COUNT, filters=flt), QM(m, sh, 20, GROUPSORT_KEY, filters=anyf), QM(m, sh, 100, GROUPSORT_WEIGHT, weight_filters=wf),
               QM(m, sh, 20, GROUPSORT_COUNT, False, filters=flt + anyf, weight_filters=wf, index_weight=3)]
    got = batch.search(c.seg, qs)
    assert check(orc, c, qs, got, "filters", [True] * len(qs)) == 0
    assert got[1].total_found > 2, "the ANY filter chose the docs, not the values that form groups"
    everything = batch.search(c.seg, [dataclasses.replace(qs[0], filters=None)])[0]
    assert 0 < int(got[0].group_count.sum()) < int(everything.group_count.sum())
    rng = np.random.default_rng(3)
    dead = np.zeros((N_DOCS + 31) // 32, np.uint32)
    killed = rng.choice(N_DOCS, N_DOCS // 5, replace=False).astype(np.uint32)
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    c.seg.set_dead_rows(dead)
    try:
        got = batch.search(c.seg, qs)
        c.bind()
        c.oi.dead_rows = dead
        saved, c.cache = c.cache, {}
        for i, (q, g) in enumerate(zip(qs, got)):
            r, w, k, cnt, total = gme.expected_groups_mva(*pushes(orc, c, q), q.group.sort_by, bool(q.group.desc), q.max_matches)
            assert g.status == 0 and g.total_found == total and np.array_equal(g.group_key, k) and np.array_equal(g.group_count, cnt) and np.array_equal(g.rowid, r) and np.array_equal(g.weight, w), ("dead", i)
        c.cache = saved
    finally:
        c.seg.set_dead_rows(None)
        c.oi.dead_rows = None


def test_rowid_base(orc, dev, indexes):
    m, ctx, batch = dev
    c = Corpus(m, ctx, indexes[4], [mva_of(cycle_values(64))], rowid_base=0xFFFF0000 - N_DOCS)  # 64 values: exactly 4 K
    try:
        qs = [QM(m, sh, 16, by, desc) for sh in ("one", "prox2") for by, desc in ORDERS]
        assert check(orc, c, qs, batch.search(c.seg, qs), "rowid_base", [True] * len(qs)) == 0
    finally:
        c.close()


# ---- segments: the corpus cut into three, GROUP rows exported and merged
S_TIE, S_FOUR, S_FIVE, S_D80 = range(4)


def segment_attrs():
    lo1, lo2 = CUTS[1], CUTS[2]
    # S_TIE: values 2 and 8 share the head (row 0) and count 2, but their second docs lie in different segments
    tie = lambda r: np.array({0: [TIE_HI, TIE_LO], lo1 + 7: [TIE_LO], lo2 + 7: [TIE_HI]}.get(r, [100 + r % 2]), np.uint32)
    seg_of = lambda r: 0 if r < lo1 else 1 if r < lo2 else 2
    four = lambda r: np.array([[1000 + r % 2], [2000], [3000]][seg_of(r)], np.uint32)      # 2 + 1 + 1 values: 4 K at K = 1
    five = lambda r: np.array([[1000 + r % 2], [2000], [3000 + r % 2]][seg_of(r)], np.uint32)  # 2 + 1 + 2: every list inside its limit, the merge past it
    return [mva_of(f) for f in (tie, four, five, cycle_values(80))]


def test_segments_merge_to_the_unsegmented_answer(orc, dev, indexes):
    m, ctx, batch = dev
    import group_merge_common as gmc
    from manticoresearch_amd import dist as mdist
    from test_gpu_group_merge import export, merge
    from test_gpu_order_merge import Hip
    from test_gpu_sort_merge import off

    ix = indexes[4]
    hip = Hip()
    c = Corpus(m, ctx, ix, segment_attrs())
    segs = []
    try:
        for lo, hi in zip(CUTS[:-1], CUTS[1:]):
            seg = m.Segment(ctx, ix.cut(lo, hi), rowid_base=lo)
            rows = np.ascontiguousarray(c.rows[lo:hi])
            seg.set_attrs(rows)
            seg.set_blobs(c.pool, c.n_blob, rows)
            segs.append(seg)
        G = lambda q: dataclasses.replace(q, total_docs=N_DOCS, local_docs=dict(ix.gdocs))
        none = lambda K, by, desc, a: G(m.Query(shapes(m)["none"][0], ranker=m.SPH_RANK_NONE, max_matches=K, group=m.Group(0, 0, sort_by=by, desc=desc, mva_bits=32, blob_attr_id=a, n_blob_attrs=4)))
        qs = [none(K, by, desc, S_TIE) for by in (GROUPSORT_COUNT, GROUPSORT_WEIGHT) for desc in (True, False) for K in (1, 20)]
        must = [True] * len(qs)
        qs += [none(1, GROUPSORT_COUNT, True, S_FOUR), none(1, GROUPSORT_COUNT, True, S_FIVE)]
        must += [True, False]
        qs += [G(QM(m, sh, 20, by, desc, S_D80, 4)) for sh in ("and2", "prox2") for by, desc in ORDERS[:4]]
        must += [True] * 8
        nq = len(qs)
        RW = gmc.WORDS
        whole = hip.to_host(export(batch, hip, [c.seg], qs), (nq, RW))
        dev_rows = export(batch, hip, segs, qs, want_status=[[0] * nq] * 3)
        lists = hip.to_host(dev_rows, (3, nq, RW))
        assert not (lists[:, :, gmc.TOTAL] & np.uint64(gmc.RERUN | gmc.DECLINED)).any(), "every list alone is inside its limit"
        one_step = merge(ctx, hip, dev_rows, 3, nq)
        assert np.array_equal(one_step, whole), [qi for qi in range(nq) if not np.array_equal(one_step[qi], whole[qi])]
        assert np.array_equal(one_step, mdist.merge_grows_np(lists, 1024)), "kernel != numpy mirror"
        ab = merge(ctx, hip, dev_rows, 2, nq)
        stage = hip.malloc(2 * nq * RW * 8)
        hip.to_dev(stage, ab)
        hip.d2d(off(stage, nq * RW * 8), off(dev_rows, 2 * nq * RW * 8), nq * RW * 8)
        assert np.array_equal(merge(ctx, hip, stage, 2, nq), one_step), "staged != one step"
        c.bind()
        for qi, q in enumerate(qs):
            row = one_step[qi]
            assert int(row[gmc.SPEC]) == mdist.group_spec_word(q.group.sort_by, bool(q.group.desc), 32, q.max_matches), (qi, "the spec word of a 32-bit key")
            want = gme.expected_groups_mva(*pushes(orc, c, q), q.group.sort_by, bool(q.group.desc), q.max_matches)
            assert (want is not DECLINED) == must[qi], (qi, "the case is not what the test designates")
            if want is DECLINED:
                assert int(row[gmc.TOTAL]) == gmc.DECLINED and int(row[gmc.CNT]) == 0 and not row[:gmc.G].any()
                continue
            r, w, k, cnt, total = want
            gr, gw, gk, gc, gt = mdist.grow_groups(row)
            assert gt == total and np.array_equal(gr, r) and np.array_equal(gw, w) and np.array_equal(gk, k) and np.array_equal(gc, cnt), (qi, gk[:8], k[:8])
        # the tie is one: merged, 2 and 8 have count 2 and the head row 0; no single list holds the tie
        assert gme.has_tie(*pushes(orc, c, qs[1]), GROUPSORT_COUNT, True)
        gk = mdist.grow_groups(one_step[1])[2].tolist()
        assert gk.index(TIE_LO) + 1 == gk.index(TIE_HI)
        for s in range(3):
            k_s, c_s = mdist.grow_groups(lists[s, 1])[2:4]
            cnt_of = dict(zip(k_s.tolist(), c_s.tolist()))
            assert cnt_of.get(TIE_LO, 0) != cnt_of.get(TIE_HI, 0) or s == 0
        # the other four row kinds decline an MVA-grouped query as they decline every grouped one
        batch.search(c.seg, qs[:2])
        for kind in ("rows", "srows", "orows"):
            from test_gpu_row_kinds import export as export_kind

            rows = export_kind(m, hip, batch, kind, 2)
            assert all(int(rows[i, 1024 + 1]) == 1 << 62 and int(rows[i, 1024]) == 0 and not rows[i, :1024].any() for i in range(2)), kind
    finally:
        hip.free()
        for s in segs:
            s.close()
        c.close()


def test_mixed_batch_and_a_reused_batch(orc, dev, corpora):
    """MVA-grouped, row-grouped, with aggregates, sorted and relevance queries in one batch: each equals its answer alone"""
    m, ctx, batch = dev
    c = corpora["d80"]
    root2, prox = shapes(m)["and2"][0], shapes(m)["prox2"][0]
    others = [m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10), m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10, sort=m.Sort(C16 * 32, 32)),
              m.Query(prox, ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=7), m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=16, group=m.Group(C16 * 32, 32, sort_by=GROUPSORT_COUNT)),
              m.Query(prox, ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=16, group=m.Group(C16 * 32, 32), aggrs=[m.Aggr(m.AGGR_SUM, AUX * 32, 32), m.Aggr(m.AGGR_MAX, M70 * 32, 32)])]
    mvas = [QM(m, "and2", 20, GROUPSORT_COUNT), QM(m, "prox2", 100, GROUPSORT_WEIGHT, False), QM(m, "one", 5, GROUPSORT_KEY)]  # (80 values at K = 5: declined)
    alone = [batch.search(c.seg, [q])[0] for q in others]
    mixed_q = [mvas[0], others[0], others[1], mvas[1], others[2], others[3], mvas[2], others[4]]
    mixed = batch.search(c.seg, mixed_q)
    check(orc, c, mvas, [mixed[0], mixed[3], mixed[6]], "mixed", [True, True, False])
    for a, g in zip(alone, [mixed[1], mixed[2], mixed[4], mixed[5], mixed[7]]):
        assert a.status == g.status == 0 and a.total_found == g.total_found and np.array_equal(a.rowid, g.rowid) and np.array_equal(a.weight, g.weight)
        for f in ("sort_key", "order_key", "group_key", "group_count", "aggr"):
            assert (getattr(a, f) is None) == (getattr(g, f) is None) and (getattr(a, f) is None or np.array_equal(getattr(a, f), getattr(g, f))), f
    # the same batch again with other groups: the tables were cleared; then without any MVA group
    again = [QM(m, "and2", 100, GROUPSORT_KEY, False), QM(m, "prox2", 20, GROUPSORT_COUNT), QM(m, "one", 20, GROUPSORT_WEIGHT)]
    assert check(orc, c, again, batch.search(c.seg, again), "resubmit", [True] * 3) == 0
    for a, g in zip(alone, batch.search(c.seg, others)):
        assert a.total_found == g.total_found and np.array_equal(a.rowid, g.rowid) and (a.group_count is None or np.array_equal(a.group_count, g.group_count))


def test_rerun_after_a_match_queue_overflow(orc, dev):
    """mq_max_chunks = 1 under 180 K matches of hit-ranked MVA-grouped queries: the match queue overflows, mrk_batch_wait reruns each
    query alone over a CLEARED table -- nothing is counted twice"""
    m, ctx, batch = dev
    n_docs = 200_000
    hi = m.synth_index(n_docs, [1.0, 0.9, 0.8], seed=31, skiplist_block_size=128, max_pos=12)
    r = np.arange(n_docs, dtype=np.uint64)
    dom = domain(16)
    # two values per doc, written straight into a pool of fixed-size blob rows: [kind 0][len 8][v0][v1] = 10 bytes
    pool = np.zeros(8 + 10 * n_docs, np.uint8)
    rec = pool[8:].reshape(n_docs, 10)
    rec[:, 0], rec[:, 1] = 0, 8
    v = np.stack([dom[(r % 16).astype(np.int64)], dom[((r * 5 + 3) % 16).astype(np.int64)]], axis=1).astype("<u4")
    rec[:, 2:] = v.view(np.uint8).reshape(n_docs, 8)
    rows = np.zeros((n_docs, STRIDE), np.uint32)
    offs = 8 + 10 * r
    rows[:, BLOB], rows[:, BLOB_HI] = (offs & 0xFFFFFFFF).astype(np.uint32), (offs >> 32).astype(np.uint32)
    seg = m.Segment(ctx, hi)
    try:
        seg.set_attrs(rows)
        seg.set_blobs(pool, 1, rows)
        from test_gpu_parity import orc_index_of

        oi = orc_index_of(orc, hi)
        oi.attrs, oi.blobs = rows, pool
        hits = [QM(m, "prox2", 8, GROUPSORT_COUNT), QM(m, "phrase", 100, GROUPSORT_KEY), QM(m, "prox2", 3, GROUPSORT_KEY)]  # (16 values at K = 3: declined)
        with Settings(ctx, mq_max_chunks=1):
            got = batch.search(seg, hits)
            n_rerun = batch.stats()["n_rerun"]
        assert n_rerun > 0
        again = batch.search(seg, hits)
        assert batch.stats()["n_rerun"] == 0
        wants = []
        for q in hits:
            full = gme.all_matches(orc, oi, dataclasses.replace(q, group=None), n_docs)
            push = (np.repeat(full.rowid, 2), np.repeat(full.weight.astype(np.int64), 2), v[full.rowid].reshape(-1))
            assert np.array_equal(gme.mva_values(pool, int(offs[int(full.rowid[0])]), 0, 1), v[int(full.rowid[0])])  # (the pool holds what the pushes say)
            wants.append(gme.expected_groups_mva(*push, q.group.sort_by, bool(q.group.desc), q.max_matches))
        for what, res in (("rerun", got), ("no rerun", again)):
            for i, (want, g) in enumerate(zip(wants, res)):
                assert (want is DECLINED) == (i == 2), (what, i)
                if want is DECLINED:
                    assert g.status == E_UNSUPPORTED
                    continue
                rr, w, k, cnt, total = want
                assert g.status == 0 and g.total_found == total and np.array_equal(g.group_key, k) and np.array_equal(g.group_count, cnt) and np.array_equal(g.rowid, rr) and np.array_equal(g.weight, w), (what, i)
    finally:
        seg.close()


def test_declines(orc, dev, corpora, indexes):
    m, ctx, batch = dev
    from manticoresearch_amd._lib import MrkError

    c = corpora["d80"]
    root, ranker = shapes(m)["and2"]
    G = lambda **kwa: m.Group(0, 0, **{**dict(mva_bits=32, blob_attr_id=0, n_blob_attrs=1), **kwa})
    base = lambda **kwa: m.Query(root, ranker=ranker, max_matches=20, **kwa)
    unsupported = [base(group=G(), aggrs=[m.Aggr(m.AGGR_SUM, AUX * 32, 32)]), base(group=G(mva_bits=64)), base(group=G(), sort=m.Sort(C16 * 32, 32)), base(group=G(), cutoff=5)]
    got = batch.search(c.seg, unsupported + [base(group=G(desc=False))])
    assert [g.status for g in got] == [E_UNSUPPORTED] * len(unsupported) + [0]
    assert all(g.group_key is None and len(g.rowid) == 0 for g in got[:-1])
    for bad in (G(mva_bits=16), G(blob_attr_id=1), G(blob_attr_id=-1), G(n_blob_attrs=2), G(n_blob_attrs=0), G(sort_by=3), G(desc=2)):
        with pytest.raises(MrkError):
            batch.search(c.seg, [base(), base(group=bad)])
    # a segment that never had a pool; a pool dropped by a later set_attrs
    seg = m.Segment(ctx, indexes[4].hi)
    try:
        seg.set_attrs(c.rows)
        assert batch.search(seg, [base(group=G())])[0].status == E_UNSUPPORTED and "blob pool" in last_error()
        seg.set_blobs(c.pool, 1, c.rows)
        assert batch.search(seg, [base(group=G())])[0].status == 0
        seg.set_attrs(c.rows)
        assert batch.search(seg, [base(group=G())])[0].status == E_UNSUPPORTED and "blob pool" in last_error()
    finally:
        seg.close()
