"""Corpora, attribute columns, queries and the expectation of the SORTED top-K selection's edge tests (csrc/mrk_sortsel.hip:
sort_select_kernel with sortsel_compact / sortsel_sort, and the bin filter cand_bin of csrc/mrk_sortkey.h), shared by
test_sortsel_edges_cpu.py (which asserts that every case has the structure it names) and test_gpu_sortsel_edges.py (which runs them
on the device).  Everything is deterministic: the indexes come from explicit hits (select_edges_common's builders), the columns are
functions of the rowid r and of j = r // 4.

Corpus S: 32 768 rowids; the matches of AND(a, b) are the rowids 4 j, j < 8192; b's tf is 3 / 2 / 1 on 300 / 500 / 7392 of them (three
weight classes), placed "even" or "high" in rowid order.  8192 candidates overfill the kernel's buffer of CAND = 2048 four times.
Corpus L: 16 384 rowids, rare keywords of exactly LIST_COUNTS docs and two disjoint ones.

The expectation is the numpy models the other sorted tests use (sorted_expect.expected_sort / expected_order,
weight_first_expect.expected_weight_first) applied to the oracle's full match list -- never the library's key map."""
import numpy as np

from select_edges_common import _hits_of, _index, oracle_index  # noqa: F401  (oracle_index: re-exported to the two test files)
from sorted_expect import all_matches, expected_order, expected_sort, part_key, raw_of
from weight_first_expect import expected_weight_first

# the kernel's constants the cases are tied to (csrc/mrk_dev.h); test_sortsel_edges_cpu.py reads them out of the header
WG, KCAP, CAND, NBINS = 256, 1024, 2048, 1024

S_DOCS, S_MATCHES = 32_768, 8_192
LADDER = (300, 500, 7_392)  # docs of class 3 (b's tf 3: the heaviest; key value 3) / 2 / 1
PLACEMENTS = ("low", "high", "even")
LADDER_KS = (1, 299, 300, 301, 799, 800, 801, 1000, 1024)
FALLBACK_FIELD_WEIGHTS = (2_200_000, 1)  # select_edges_common.FALLBACK_FIELD_WEIGHTS: bins_by_weight's estimate leaves int32
NEGATIVE_FIELD_WEIGHTS = (1, -3)         # every hit lies in field 1: every weight is negative
S_BASES = (2**32 - S_DOCS, 2**31 - S_DOCS // 2)  # case 9: the segment ends at global rowid 2^32 - 1; bit 31 of ~rowid flips half way through it

# ---- dwords of a row of corpus S
LAD_LOW, LAD_HIGH, LAD_EVEN, CONST, FULL32, SPAN1023, SPAN1024, SPAN1025, BAND, BITS_A, BITS_B, FLTD, FLTA, I64, CAT4, R255, R256 = (
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17)
S_STRIDE = 18
LAD = {"low": LAD_LOW, "high": LAD_HIGH, "even": LAD_EVEN}
SPAN_LO = 0x12345000
BAND_LO = 0x7FFF0000
R_LO = 1_000_000
I64_VALUES = (-2**63, 2**63 - 1, -1, 0, 1, 0x7FFFFFFF, 0x80000000, -0x80000000, -0x80000001)
ZEROS = 1000      # rows of -0.0, and as many of +0.0
FLT_ABOVE = 500   # matches above the zero class of FLTD (below it in FLTA = -FLTD)
FLT_KS = (1, 500, 501, 1000, 1024)
FLT_EDGES = (0x7F800000, 0x7F7FFFFF, 0x007FFFFF, 0x00000001)  # +inf, FLT_MAX, the largest and the least denormal; | 0x80000000: the negatives

INT, FLOAT, INT64 = 0, 1, 2  # m.SORTKEY_*
# name -> (bit offset, bit count, kind)
COLS = {"lad_low": (LAD_LOW * 32, 32, INT), "lad_high": (LAD_HIGH * 32, 32, INT), "lad_even": (LAD_EVEN * 32, 32, INT), "const": (CONST * 32, 32, INT),
        "full32": (FULL32 * 32, 32, INT), "span1023": (SPAN1023 * 32, 32, INT), "span1024": (SPAN1024 * 32, 32, INT), "span1025": (SPAN1025 * 32, 32, INT),
        "band": (BAND * 32, 32, INT), "bit31": (BITS_B * 32 + 31, 1, INT), "bit0": (BITS_A * 32, 1, INT), "bits31at1": (BITS_A * 32 + 1, 31, INT),
        "bits5at27": (BITS_B * 32 + 27, 5, INT), "fltd": (FLTD * 32, 32, FLOAT), "flta": (FLTA * 32, 32, FLOAT), "i64": (I64 * 32, 64, INT64),
        "cat4": (CAT4 * 32, 32, INT), "r255": (R255 * 32, 32, INT), "r256": (R256 * 32, 32, INT)}


def ladder(placement, n=S_MATCHES):
    """the class (3 / 2 / 1) of every match in rowid order: LADDER's sizes, the better classes at low rowids, at high ones or spread evenly"""
    best, second, rest = LADDER
    assert best + second + rest == n
    c = np.ones(n, np.int64)
    if placement == "low":
        c[:best], c[best:best + second] = 3, 2
    elif placement == "high":
        c[n - best:], c[n - best - second:n - best] = 3, 2
    else:
        c[(np.arange(best, dtype=np.int64) * n) // best] = 3
        left = np.flatnonzero(c == 1)
        c[left[(np.arange(second, dtype=np.int64) * left.size) // second]] = 2
    assert (np.bincount(c, minlength=4)[1:] == (rest, second, best)).all()
    return c


def key_ladder(placement):
    """the LAD column of the matches.  "even" runs backwards, or it would BE the weight ladder placed "even": key and weight independent"""
    return ladder(placement)[::-1].copy() if placement == "even" else ladder(placement)


def s_index(m, placement):
    """corpus S with the weight ladder placed `placement`"""
    rows = np.arange(S_MATCHES, dtype=np.uint32) * 4
    return _index(m, [_hits_of(0, rows, np.ones(rows.size, np.int64), 1), _hits_of(1, rows, ladder(placement), 2)], 2, S_DOCS)


def full32_values():
    """0, 2^32 - 1, and the two keys on either side of every boundary of the 1024 bins of shift 22"""
    c = np.arange(1, NBINS, dtype=np.uint64) << np.uint64(22)
    v = np.concatenate([[0, 0xFFFFFFFF], c - np.uint64(1), c]).astype(np.uint32)
    assert v.size == 2 * NBINS and np.unique(v).size == v.size
    return v


def fltd_values():
    """FLTD of the matches by j: 2 * ZEROS zeros at j = 4 i, -0.0 and +0.0 taking turns; FLT_ABOVE positive rows at j = 4 i + 1, the
    edges among them; every other match negative, the negated edges among them"""
    j = np.arange(S_MATCHES, dtype=np.int64)
    v = (-(1.0 + (j % 977)) * 0.25).astype(np.float32).view(np.uint32).copy()
    pos = np.flatnonzero((j % 4 == 1) & (j < 4 * FLT_ABOVE))
    v[pos] = ((1.0 + (pos * 37) % 1000) * 0.5).astype(np.float32).view(np.uint32)
    zero = np.flatnonzero((j % 4 == 0) & (j < 8 * ZEROS))
    v[zero] = np.where((zero // 4) % 2 == 0, 0x80000000, 0).astype(np.uint32)
    for i, e in enumerate(FLT_EDGES):  # each edge twice, far apart in the list
        v[pos[[7 + 3 * i, pos.size - 5 - 3 * i]]] = e
    neg = np.flatnonzero(j % 4 == 2)
    for i, e in enumerate(FLT_EDGES):
        v[neg[[11 + 5 * i, neg.size - 9 - 5 * i]]] = e | 0x80000000
    return v


def s_rows():
    """the attribute rows of corpus S.  Rows with r % 4 != 0 match nothing: they hold a value inside the matches' range, except BAND,
    where they hold the 32-bit extremes (the planner's range is taken over all rows)"""
    r = np.arange(S_DOCS, dtype=np.uint64)
    j = np.arange(S_MATCHES, dtype=np.uint64)
    rows = np.zeros((S_DOCS, S_STRIDE), np.uint32)
    hit = np.arange(S_MATCHES) * 4

    def put(col, matches, others):
        rows[:, col] = others
        rows[hit, col] = matches

    for p in PLACEMENTS:
        put(LAD[p], key_ladder(p), 1)
    put(CONST, 42, 42)
    put(FULL32, full32_values()[(j * np.uint64(1237)) % np.uint64(2 * NBINS)], 0x80000000)  # (1237 is odd: every value on four matches)
    put(SPAN1023, SPAN_LO + j % np.uint64(1024), SPAN_LO)
    put(SPAN1024, SPAN_LO + j % np.uint64(1025), SPAN_LO)
    put(SPAN1025, SPAN_LO + j % np.uint64(1026), SPAN_LO)
    put(BAND, BAND_LO + j % np.uint64(1025), np.where(r % np.uint64(2) == 1, 0, 0xFFFFFFFF).astype(np.uint32))
    rows[:, BITS_A] = ((r * np.uint64(2654435761)) >> np.uint64(3)).astype(np.uint32)  # noise: every bit of either dword varies over the matches
    rows[:, BITS_B] = ((r * np.uint64(40503) * np.uint64(65537)) ^ (r << np.uint64(25))).astype(np.uint32)
    put(FLTD, fltd_values(), np.float32(1.0).view(np.uint32))
    put(FLTA, fltd_values() ^ np.uint32(0x80000000), np.float32(1.0).view(np.uint32))
    big = np.zeros(S_DOCS, np.int64)
    big[hit] = np.array([v if v < 2**63 else v - 2**64 for v in I64_VALUES], np.int64)[np.arange(S_MATCHES) % len(I64_VALUES)]
    rows[:, I64:I64 + 2] = big.view(np.uint32).reshape(S_DOCS, 2)
    put(CAT4, j % np.uint64(4), 0)
    put(R255, R_LO + (j * np.uint64(7)) % np.uint64(256), R_LO)
    put(R256, R_LO + (j * np.uint64(7)) % np.uint64(257), R_LO)
    return rows


# ---- corpus L: the list lengths around the compaction trigger CAND - WG = 1792 and around CAND
L_DOCS = 16_384
LIST_COUNTS = (1, 255, 256, 257, 1791, 1792, 1793, 2047, 2048, 2049, 4097)
L_EVEN, L_ODD = len(LIST_COUNTS), len(LIST_COUNTS) + 1  # two disjoint keywords: rowids 8 i and 8 i + 1
L_CONST, L_DIST, L_STRIDE = 0, 1, 2
L_COLS = {"const": (L_CONST * 32, 32, INT), "dist": (L_DIST * 32, 32, INT)}


def list_rows_of(t):
    """the docs of keyword t of corpus L: a fixed pseudo-random draw (as select_edges_common.slice_rows draws)"""
    if t >= len(LIST_COUNTS):
        return np.arange(L_DOCS // 8, dtype=np.uint32) * 8 + (t - L_EVEN)
    return np.sort(np.random.default_rng(1000 + t).choice(L_DOCS, LIST_COUNTS[t], replace=False)).astype(np.uint32)


def l_index(m):
    parts = [_hits_of(t, list_rows_of(t), np.ones(list_rows_of(t).size, np.int64), 1) for t in range(len(LIST_COUNTS) + 2)]
    return _index(m, parts, len(LIST_COUNTS) + 2, L_DOCS)


def l_rows():
    rows = np.zeros((L_DOCS, L_STRIDE), np.uint32)
    rows[:, L_CONST] = 42
    rows[:, L_DIST] = (np.arange(L_DOCS, dtype=np.uint64) * np.uint64(2654435761)).astype(np.uint32)  # (an odd multiplier: distinct values)
    return rows


# ---- queries
def root_ab(m):
    k = m.XQNode.keyword
    return m.XQNode.AND(k(0, 1), k(1, 2))


def part(m, name, desc, cols=COLS):
    off, cnt, kind = cols[name]
    return m.OrderPart(off, cnt, desc=desc, kind=kind)


def q_sort(m, name, K, desc, tie, ranker=None, root=None, cols=COLS, **kw):
    off, cnt, kind = cols[name]
    return m.Query(root or root_ab(m), ranker=m.SPH_RANK_BM25 if ranker is None else ranker, max_matches=K,
                   sort=m.Sort(off, cnt, desc=desc, then_weight=tie, kind=kind), **kw)


def q_order(m, parts, K, tie=1, wf=0, ranker=None, **kw):
    """parts: [(column, desc)]; wf: Order.weight_first (then the tie rule is none)"""
    o = m.Order([part(m, n, d) for n, d in parts], weight_first=wf) if wf else m.Order([part(m, n, d) for n, d in parts], then_weight=tie)
    return m.Query(root_ab(m), ranker=m.SPH_RANK_BM25 if ranker is None else ranker, max_matches=K, order=o, **kw)


def case1(m, ranker, placements=PLACEMENTS):
    """key ladders: every K around the class edges, both directions, three tie rules"""
    return [q_sort(m, "lad_" + p, K, desc, tie, ranker) for p in placements for desc in (True, False) for tie in (0, 1, 2) for K in LADDER_KS]


def case2(m, ranker):
    return [q_sort(m, "const", K, desc, tie, ranker) for tie in (0, 1, 2) for K in (1, 2, 300, 301, 1024) for desc in ((True, False) if K == 300 else (True,))]


GEOMETRY_COLS = ("full32", "span1023", "span1024", "span1025", "band")


def case3(m):
    return [q_sort(m, c, K, desc, (i + k) % 3) for i, c in enumerate(GEOMETRY_COLS) for desc in (True, False) for k, K in enumerate((1, 10, 1024))]


BITFIELD_COLS = ("bit31", "bit0", "bits31at1", "bits5at27")


def case4(m):
    return [q_sort(m, c, K, desc, tie) for c in BITFIELD_COLS for tie in (0, 1) for desc in (True, False) for K in (1, 1000, 1024)]


def case5(m):
    return [q_sort(m, c, K, desc, tie) for c in ("fltd", "flta") for desc in (True, False) for tie in (0, 1) for K in FLT_KS]


TWO_PARTS = (("cat4", "full32"), ("full32", "cat4"), ("const", "span1024"), ("cat4", "r255"), ("cat4", "r256"), ("bit31", "fltd"))


def case6(m):
    qs = [q_order(m, [("i64", desc)], K, tie) for desc in (True, False) for tie in (0, 1, 2) for K in (1, 911, 1024)]
    for i, (a, b) in enumerate(TWO_PARTS):
        for j, (da, db) in enumerate(((True, True), (False, False), (True, False), (False, True))):
            qs.append(q_order(m, [(a, da), (b, db)], (1024, 1000, 10, 1)[(i + j) % 4], (i + j) % 3))
    return qs


WF_PARTS = ([], [("lad_low", False)], [("i64", True)], [("cat4", True), ("span1024", False)])
WF_KS = (1, 300, 301, 800, 801, 1024)


def case7(m, **kw):
    """weight-first: both directions over every shape of parts (no parts: weight ASC alone)"""
    return [q_order(m, p, K, wf=wf, **kw) for wf in (1, 2) for p in WF_PARTS if p or wf == 2 for K in WF_KS]


def case7_negative(m):
    fw = list(NEGATIVE_FIELD_WEIGHTS)
    return [q for q in case7(m, field_weights=fw) if q.max_matches in (300, 301, 1024)] + [
        q_sort(m, "lad_low", K, desc, tie, field_weights=fw) for tie in (1, 2) for desc in (True, False) for K in (301, 1024)]


def case8(m):
    """corpus L: every list length under CONST (everything passes the bin filter) and under distinct values, back to back; the two
    last queries match nothing"""
    k = m.XQNode.keyword
    qs = [q_sort(m, c, K, (t + K) % 2 == 0, 0, root=k(t, 1), cols=L_COLS) for t in range(len(LIST_COUNTS)) for c in ("const", "dist") for K in (1, 1024)]
    none = m.XQNode.AND(k(L_EVEN, 1), k(L_ODD, 2))
    return qs + [q_sort(m, "const", 1024, True, 0, root=none, cols=L_COLS), q_sort(m, "dist", 1, False, 0, root=none, cols=L_COLS)]


def case9(m):
    return [q_sort(m, "lad_high", K, True, tie) for tie in (0, 1, 2) for K in LADDER_KS] + [q_order(m, [("lad_low", False)], 801, wf=1)]


def case10(m):
    """one query of every candidate layout, and of the layouts sort_select_kernel leaves alone (relevance, grouped), each next to each
    other one: a sequence over the seven kinds in which every ordered pair of different kinds is adjacent once"""
    off, cnt, _ = COLS["cat4"]
    make = [lambda K: q_sort(m, "span1025", K, True, 1), lambda K: q_order(m, [("band", False)], K, 2), lambda K: q_order(m, [("i64", True)], K, 0),
            lambda K: q_order(m, [("cat4", True), ("full32", False)], K, 1), lambda K: q_order(m, [("lad_even", True)], K, wf=2),
            lambda K: m.Query(root_ab(m), ranker=m.SPH_RANK_BM25, max_matches=K),
            lambda K: m.Query(root_ab(m), ranker=m.SPH_RANK_BM25, max_matches=K, group=m.Group(off, cnt, sort_by=m.GROUPSORT_COUNT, desc=True))]
    seq, n = [], len(make)
    for d in range(1, n):  # (a, a + d) for every a: with d over 1..n-1 every ordered pair of different kinds
        for a in range(n):
            seq += [a, (a + d) % n]
    return seq, [make[kind]((1, 301, 1024)[i % 3]) for i, kind in enumerate(seq)]


# ---- the expectation
def expect(orc, oi, q, rows):
    """(rowid, weight, raw sort / order key or None, total_found) by the numpy model of q's kind, on the oracle's full list"""
    f = expected_sort if q.sort is not None else expected_weight_first if q.order.weight_first else expected_order
    return f(orc, oi, q, rows, rows.shape[0])


def bin_keys(q, full, rows):
    """per match of the full list, the columns of the quantity the pruning bins are taken from: the whole attribute key of a sort or an
    order (floats as floats: the two zeros are one key), the weight of a weight-first order"""
    if q.sort is not None:
        s = q.sort
        return [part_key(raw_of(rows, full.rowid, s.bit_offset, s.bit_count), s.kind, s.desc)]
    o = q.order
    if o.weight_first:
        return [full.weight.astype(np.int64)]
    if o.parts[0].kind == INT64:
        item = o.parts[0].bit_offset >> 5
        return [np.ascontiguousarray(rows[full.rowid, item:item + 2]).view(np.int64).reshape(-1)]
    return [part_key(raw_of(rows, full.rowid, p.bit_offset, p.bit_count), p.kind, p.desc) for p in o.parts]


def tie_floor(q, full, rows, want_rowid):
    """how many matches tie the expected K-th row on the binned quantity: under any monotone bin map they share its bin, so every one
    of them must be in the candidate list.  Fewer than K matches: all of them"""
    if len(want_rowid) < q.max_matches or not len(want_rowid):
        return int(full.total_found)
    at = int(np.flatnonzero(full.rowid == want_rowid[-1])[0])
    same = np.ones(len(full.rowid), bool)
    for k in bin_keys(q, full, rows):
        same &= k == k[at]
    return int(same.sum())


class Corpora:
    """the corpora by name, each built once per module: ("S", weight placement) and ("L",) -> (host index, oracle index, rows); and the
    oracle's full list per (corpus, base query), left unchanged"""

    def __init__(self, m, orc):
        self.m, self.orc, self._built, self._full = m, orc, {}, {}

    def get(self, *name):
        if name not in self._built:
            hi, rows = (s_index(self.m, name[1]), s_rows()) if name[0] == "S" else (l_index(self.m), l_rows())
            oi = oracle_index(self.orc, hi)
            oi.attrs = rows
            rows.setflags(write=False)
            self._built[name] = (hi, oi, rows)
        return self._built[name]

    def full(self, name, q):
        """q's full match list (every match with its weight)"""
        key = (name, repr(q.root), q.ranker, tuple(q.field_weights or ()))
        if key not in self._full:
            hi, oi, rows = self.get(*name)
            r = all_matches(self.orc, oi, q, rows.shape[0])
            r.rowid.setflags(write=False), r.weight.setflags(write=False)
            self._full[key] = r
        return self._full[key]

    def want(self, name, q):
        hi, oi, rows = self.get(*name)
        return expect(self.orc, oi, q, rows)

    def floor(self, name, q, want):
        return tie_floor(q, self.full(name, q), self.get(*name)[2], want[0])
