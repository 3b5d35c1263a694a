"""Shared by tests/test_rank_edges_cpu.py and tests/test_gpu_rank_edges.py: an independent model of the six state rankers, the
hand-made corpora that put one doc on every edge of them, the queries sorted by rank pass, and a restatement of the weight bounds
(prox_bounds, csrc/mrk_kprune.h).  Nothing here runs on the device.

THE MODEL.  The Update / Finalize pairs of sphinxsearch.cpp:1320-1668, restated from that text alone in Python integers with
explicit masks, over an explicit hit stream of (hitpos, qpos, weight, spanlen): hitpos = field << 24 | END | position as it is
stored.  A state object lives as long as a query: the very first doc meets the Init values (m_iExpDelta = -INT_MAX), every later
one the values Finalize left (-1; SPH04's m_uMinExpPos is NOT reset and keeps the last hit of the doc in front).  The device
(RankStateT::reset, hit_rank_prox) starts every doc afresh and claims that this cannot show; the model is what tests that claim.

For a flat AND / OR of keywords the stream is sorted((raw hitpos, qpos)), hits outside a keyword's field limit left out
(hit_edges_common.stream).  Node folding (a phrase's hits becoming one hit of weight n and spanlen n) is NOT modelled: the folded
streams of the golden pin are written out by hand, and the folded queries of route F are held against the oracle and the
hand-stated cell answers only.

THE BM25 PART.  PROXIMITY_BM25 and SPH04 return bm25 + 1000 x rank.  The model takes bm25 from the oracle: under SPH_RANK_BM25 the
oracle's weight is bm25 + 1000 x (sum of the weights of the matched fields), so

    bm25(doc) = oracle weight under SPH_RANK_BM25 at index_weight 1  -  1000 x sum(weights[f] for f in the fields of the doc's stream)

and the model's weight is int32((bm25 + 1000 x rank) x index_weight) (PROXIMITY, MATCHANY, WORDCOUNT, FIELDMASK: int32(rank x
index_weight)).  That is the only thing the model takes from the oracle.

THE CORPORA.  One doc per named cell (CELLS): a row names its edge, the line it aims at, its hits by ROLE and the hand-stated
per-field figures under the query shapes it is made for.  Roles are fields: "0" = field 0, "x" < "y" < "z" = three fields in the middle,
"top" = the last field; SEGMENTS gives them per segment -- 8 fields and 32, lone hits inline and through .spp -- so that in the
32-field segments the interesting fields are 7, 8, 16 and 30 / 31: all four words of FieldBytes<4>.  The rowids are a fixed permutation
of the cells, so neighbouring lanes differ; test_rank_edges_cpu.py reads every cell's structure back from the hits.

WHAT CANNOT BE REACHED (test_rank_edges_cpu.py shows the first with the model over these streams, it is not assumed):
  * a byte-wide LCS wrapping at 256.  A run grows by one per hit whose position is new, and only while position - query position stays
    the same, so its length is bounded by the number of query positions (8 keywords) plus the shared-position cases (a keyword pair
    flagged apart adds one): the longest run of these corpora is 8.  Folded hits add their word count, still within the query.
  * `delta < 32` of the repeated-keyword update at 31: a match needs query position = tail's + delta, so delta = 31 needs a query position
    of 32 or more, which `1UL << qpos` stored into a DWORD drops.  The docs at distances 30, 31, 32 are here all the same (2, 1, 1).
  * MATCHANY with a query position of 33 and above: `1 << (qpos - 1)` is an undefined shift in the reference.  Left out: the shapes
    with such positions run under the other rankers only.
  * a field-limited keyword in front of prox_bounds: scan_bt_kernel takes keywords that are unrestricted in fields only
    (tree_kernel_usable, mrk_plan.cpp), so such a query is the block scan's, without the bounds; the GPU test asserts that route."""
import dataclasses
import functools
from typing import Dict, Tuple

import numpy as np

END = 1 << 23
POS_MASK = END - 1
INT_MAX = (1 << 31) - 1
U32 = 0xFFFFFFFF
MAX_FIELDS = 256  # SPH_MAX_FIELDS
A, B, C, D, E, F, G, H, Z = range(9)
N_TERMS = 9
PRIMES = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131]


def i32(v):
    v &= U32
    return v - (1 << 32) if v >> 31 else v


def field_of(h):
    return (h >> 24) & 0xFF


def pos_with_field(h):
    return h & ~END & U32


def pos_of(h):
    return h & POS_MASK


def is_end(h):
    return bool(h & END)


# --------------------------------------------------------------------------- the model
class Proximity:
    """RankerState_Proximity_fn<USE_BM25, HANDLE_DUPES> (:1320-1438)"""

    def __init__(self, n_fields, weights, dupes=False, use_bm25=True, **_):
        self.n_fields, self.w, self.dupes, self.use_bm25 = n_fields, weights, dupes, use_bm25
        self.lcs = [0] * MAX_FIELDS
        self.cur = 0
        self.exp_delta = -INT_MAX
        self.last = -INT_MAX
        self.tail_pos = self.tail_mask = self.cur_mask = self.cur_pos = 0
        self.longest = 0  # (not the reference's: the longest run before the byte mask, for the unreachability statement)

    def grow(self, v):
        self.longest = max(self.longest, v)
        return v & 0xFF

    def update(self, hitpos, qpos, weight=1, spanlen=1):
        f = field_of(hitpos)
        if not self.dupes:
            pwf = i32(pos_with_field(hitpos))
            delta = pwf - qpos
            if pwf > self.last:
                self.cur = self.grow((self.cur if delta == self.exp_delta else 0) + (weight & 0xFF))
            if self.cur > self.lcs[f]:
                self.lcs[f] = self.cur
            self.last = pwf
            self.exp_delta = delta + spanlen - 1
            return
        upos = pos_with_field(hitpos)
        if field_of(self.cur_pos) != f:
            self.cur_mask = 0
        if upos != self.cur_pos:
            if self.cur < 2:
                self.tail_pos, self.tail_mask, self.cur = self.cur_pos, self.cur_mask, 1
            self.cur_mask, self.cur_pos = 0, upos
            if self.lcs[f] < weight:
                self.lcs[f] = weight & 0xFF
        assert qpos < 64, "1UL << qpos: 64 and above is an undefined shift"
        self.cur_mask |= (1 << qpos) & U32
        d = i32(self.cur_pos - self.tail_pos)
        assert d >= 0, "the stream ascends inside a doc and Finalize zeroes both positions"
        if d and d < 32 and (self.cur_mask >> d) & self.tail_mask:
            self.tail_mask, self.tail_pos = (1 << qpos) & U32, self.cur_pos
            self.cur = self.grow(self.cur + weight)
            self.cur_mask = 0
            if self.cur > self.lcs[f]:
                self.lcs[f] = self.cur

    def reset_run(self):
        self.cur, self.exp_delta, self.last = 0, -1, -1
        if self.dupes:
            self.tail_pos = self.tail_mask = self.cur_mask = self.cur_pos = 0

    def finalize(self, bm25=0):
        self.reset_run()
        rank = sum(self.lcs[i] * self.w[i] for i in range(self.n_fields))
        self.lcs = [0] * MAX_FIELDS
        return rank, (bm25 + rank * 1000 if self.use_bm25 else rank)


class Sph04:
    """RankerState_ProximityBM25Exact_fn (:1443-1530)"""

    def __init__(self, n_fields, weights, max_qpos=0, **_):
        self.n_fields, self.w, self.max_qpos = n_fields, weights, max_qpos
        self.lcs = [0] * MAX_FIELDS
        self.cur, self.exp_delta, self.last, self.min_exp, self.head, self.exact = 0, -INT_MAX, -1, 0, 0, 0
        self.longest = 0
        self.stale_min_exp_decided = 0  # docs whose first hit took the `if` branch because of the state a doc in front left

    def update(self, hitpos, qpos, weight=1, spanlen=1):
        f, pwf = field_of(hitpos), i32(pos_with_field(hitpos))
        delta = pwf - qpos
        bit = (1 << f) & U32
        if delta == self.exp_delta and pos_with_field(hitpos) >= self.min_exp:
            if self.last == -1 and self.cur == 0:
                self.stale_min_exp_decided += 1
            if pwf > self.last:
                self.cur = (self.cur + weight) & 0xFF
            if is_end(hitpos) and qpos == self.max_qpos and pos_of(hitpos) == self.max_qpos:
                self.exact |= bit
        else:
            if pwf > self.last:
                self.cur = weight & 0xFF
            if pos_of(hitpos) == 1:
                self.head |= bit
                if is_end(hitpos) and self.max_qpos == 1:
                    self.exact |= bit
        self.longest = max(self.longest, self.cur)
        if self.cur > self.lcs[f]:
            self.lcs[f] = self.cur
        self.exp_delta = delta + spanlen - 1
        self.last = pwf
        self.min_exp = (pos_with_field(hitpos) + 1) & U32

    def finalize(self, bm25=0):
        self.cur, self.exp_delta, self.last = 0, -1, -1
        rank = sum((4 * self.lcs[i] + 2 * ((self.head >> i) & 1) + ((self.exact >> i) & 1)) * self.w[i] for i in range(self.n_fields))
        self.lcs = [0] * MAX_FIELDS
        self.head = self.exact = 0
        return rank, bm25 + rank * 1000


class MatchAny(Proximity):
    """RankerState_MatchAny_fn (:1578-1616)"""

    def __init__(self, n_fields, weights, n_qwords=0, **_):
        super().__init__(n_fields, weights, dupes=False, use_bm25=False)
        self.phrase_k = sum(weights[i] * n_qwords for i in range(n_fields))
        self.mask = [0] * MAX_FIELDS

    def update(self, hitpos, qpos, weight=1, spanlen=1):
        super().update(hitpos, qpos, weight, spanlen)
        assert 1 <= qpos <= 32, "1 << (qpos - 1) on an int: 33 and above is an undefined shift"
        self.mask[field_of(hitpos)] |= (1 << (qpos - 1)) & 0xFF

    def finalize(self, bm25=0):
        self.reset_run()
        rank = 0
        for i in range(self.n_fields):
            if self.mask[i]:
                rank += (bin(self.mask[i]).count("1") + (self.lcs[i] - 1) * self.phrase_k) * self.w[i]
        self.mask = [0] * MAX_FIELDS
        self.lcs = [0] * MAX_FIELDS
        return rank, rank


class Wordcount:
    """RankerState_Wordcount_fn (:1620-1643)"""

    def __init__(self, n_fields, weights, **_):
        self.w, self.rank = weights, 0

    def update(self, hitpos, qpos, weight=1, spanlen=1):
        self.rank += self.w[field_of(hitpos)]

    def finalize(self, bm25=0):
        r, self.rank = self.rank, 0
        return r, r


class Fieldmask:
    """RankerState_Fieldmask_fn (:1647-1668)"""

    def __init__(self, n_fields, weights, **_):
        self.rank = 0

    def update(self, hitpos, qpos, weight=1, spanlen=1):
        self.rank |= (1 << field_of(hitpos)) & U32

    def finalize(self, bm25=0):
        r, self.rank = self.rank, 0
        return i32(r), i32(r)


def state_of(m, ranker, n_fields, field_weights, dupes, max_qpos, n_qwords):
    """the ranker state of one query; field weights bind as BindWeights does (sphinx.cpp:13903-13943): 1 for a field past the given ones"""
    w = [(field_weights[i] if field_weights is not None and i < len(field_weights) else 1) for i in range(n_fields)] + [0] * (MAX_FIELDS - n_fields)
    kw = dict(max_qpos=max_qpos, n_qwords=n_qwords)
    if ranker in (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_PROXIMITY):
        return Proximity(n_fields, w, dupes=dupes, use_bm25=ranker == m.SPH_RANK_PROXIMITY_BM25), w
    cls = {m.SPH_RANK_SPH04: Sph04, m.SPH_RANK_MATCHANY: MatchAny, m.SPH_RANK_WORDCOUNT: Wordcount, m.SPH_RANK_FIELDMASK: Fieldmask}[ranker]
    return cls(n_fields, w, **kw), w


def uses_bm25(m, ranker):
    return ranker in (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_SPH04)


# --------------------------------------------------------------------------- flat queries over doc hits
def queried(mask, hit):
    return (mask >> field_of(hit)) & 1 != 0


def keywords_of(root):
    """[(term, qpos, field limit)] of a keyword or a flat AND / OR of keywords"""
    if root.word is not None:
        return [(root.word.term_id, root.word.atom_pos, root.field_mask)]
    return [(c.word.term_id, c.word.atom_pos, c.field_mask) for c in root.children]


def is_flat(m, root):
    return root.word is not None or (root.op in (m.SPH_QUERY_AND, m.SPH_QUERY_OR) and all(c.word is not None and not c.term_pos() for c in root.children))


def stream(hits, kws):
    """the merged hit stream of one doc (hits: term -> raw hit positions): by the raw position, end flag included, then the query position"""
    return sorted((h, qp) for t, qp, mask in kws for h in hits.get(t, ()) if queried(mask, h))


def matches(hits, kws, match_all):
    have = [any(queried(mask, h) for h in hits.get(t, ())) for t, _, mask in kws]
    return all(have) if match_all else any(have)


def model_flat(m, ranker, kws, match_all, docs_hits, n_fields, field_weights=None, index_weight=1, bm25_of=None):
    """-> ({rowid: (rank part, weight)}, the state): a flat AND (match_all) / OR of kws over the docs in rowid order, ONE state for all of them.
    bm25_of: rowid -> the BM25 part (see the module's doc); not read where the ranker adds none."""
    terms = [t for t, _, _ in kws]
    dupes = len(set(terms)) < len(terms)
    st, _ = state_of(m, ranker, n_fields, field_weights, dupes, max(qp for _, qp, _ in kws), len(set(terms)))
    out = {}
    for rowid, hits in enumerate(docs_hits):
        if not matches(hits, kws, match_all):
            continue
        for hp, qp in stream(hits, kws):
            st.update(hp, qp)
        rank, weight = st.finalize(bm25_of[rowid] if uses_bm25(m, ranker) else 0)
        out[rowid] = (i32(rank), i32(i32(weight) * index_weight))
    return out, st


def model_run(m, q, docs_hits, n_fields, bm25_of=None):
    return model_flat(m, q.ranker, keywords_of(q.root), q.root.word is not None or q.root.op == m.SPH_QUERY_AND, docs_hits, n_fields, q.field_weights,
                      q.index_weight, bm25_of)


def bound_weights(field_weights, n_fields):
    return [(field_weights[i] if field_weights is not None and i < len(field_weights) else 1) for i in range(n_fields)]


def stream_fields_weight(hits, kws, w):
    return sum(w[f] for f in {field_of(h) for h, _ in stream(hits, kws)})


def top_k(per_doc, k):
    """-> (rowids, weights) in the sorter's order: weight descending, rowid ascending"""
    rows = sorted((-wt, r) for r, (_, wt) in per_doc.items())[:k]
    return np.array([r for _, r in rows], np.uint32), np.array([-wt for wt, _ in rows], np.int32)


# --------------------------------------------------------------------------- the segments and their roles
# name, n_fields, hit_format (1 = lone hits inline), skiplist block, (x, y, z)
SEGMENTS = [("N-inline-128", 8, 1, 128, (1, 2, 5)), ("N-plain-128", 8, 0, 128, (3, 4, 6)), ("W-inline-128", 32, 1, 128, (7, 8, 16)),
            ("W-plain-128", 32, 0, 128, (8, 16, 30)), ("W-inline-32", 32, 1, 32, (7, 16, 30))]
SEGMENT_IDS = [s[0] for s in SEGMENTS]
PERM_SEED = 5


def roles_of(name):
    _, nf, _, _, (x, y, z) = next(s for s in SEGMENTS if s[0] == name)
    return {"0": 0, "x": x, "y": y, "z": z, "top": nf - 1}


def weight_sets(name):
    """None; primes; a set with a 0 and a negative; one shorter than the field count (the fields from y on weigh 1); one that sums to less than 0"""
    _, nf, _, _, (x, y, z) = next(s for s in SEGMENTS if s[0] == name)
    return {"none": None, "primes": PRIMES[:nf], "mixed": [(3, 0, -2, 5)[i % 4] for i in range(nf)], "short": [(3, 0, -2, 5)[i % 4] for i in range(y)],
            "negsum": [(1, -2, 0, -1)[i % 4] for i in range(nf)]}


# --------------------------------------------------------------------------- the cells
@dataclasses.dataclass
class Cell:
    name: str
    edge: str                      # the edge and the source line it aims at
    hits: Tuple                    # (term, role, position, flagged)
    expect: Dict = dataclasses.field(default_factory=dict)  # (shape, ranker family) -> {role: figure}: see cell_rank
    note: str = ""


def h(term, role, *positions, end=None):
    """hits of one keyword in one field; end = the position that carries the END flag"""
    return tuple((term, role, p, p == end) for p in positions)


PROX, SPH, ANY, WC, FM = "prox", "sph04", "matchany", "wordcount", "fieldmask"

CELLS = [
    # ---- runs
    Cell("run2", "keywords in query order: LCS 2; sphinxsearch.cpp:1360, mrk_khits.h:352, 921", h(A, "x", 5) + h(B, "x", 6),
         {("ab", PROX): {"x": 2}, ("ab", SPH): {"x": (2, 0, 0)}, ("ab", ANY): {"x": (2, 2)}, ("ab", WC): {"x": 2}, ("ab", FM): {"x": 1}, ("a1b3", PROX): {"x": 1}}),
    Cell("run3", "three keywords in query order: LCS 3; :1360, hit_rank_prox<3>", h(A, "y", 5) + h(B, "y", 6) + h(C, "y", 7), {("abc", PROX): {"y": 3}, ("ab", PROX): {"y": 2}}),
    Cell("run4", "LCS 4; a field-limited b on the run's second position: a, c, d keep one delta and run to 3 without it (:1360)",
         h(A, "y", 5) + h(B, "y", 6) + h(C, "y", 7) + h(D, "y", 8) + h(B, "x", 20),
         {("abcd", PROX): {"y": 4, "x": 1}, ("a bX c d", PROX): {"y": 3, "x": 1}, ("abc", PROX): {"y": 3, "x": 1}}),
    Cell("run8", "LCS 5..8 on the generic route (gen_eval feeds RankStateT::update, mrk_khits.h:352-355); every bit of MATCHANY's byte, :1596, mrk_khits.h:353", tuple(x for i, t in enumerate((A, B, C, D, E, F, G, H)) for x in h(t, "z", 10 + i)),
         {("a-e", PROX): {"z": 5}, ("a-f", PROX): {"z": 6}, ("a-g", PROX): {"z": 7}, ("a-h", PROX): {"z": 8}, ("a-h", ANY): {"z": (8, 8)}, ("abcd", PROX): {"z": 4}}),
    Cell("slack", "one position of slack breaks the delta: 1; :1360", h(A, "x", 5) + h(B, "x", 7), {("ab", PROX): {"x": 1}, ("a1b3", PROX): {"x": 2}, ("ab", SPH): {"x": (1, 0, 0)}},
         note="under a@1 b@3 the gap of the query positions is the gap of the positions: 2"),
    Cell("reversed", "the keywords in reversed order: 1; :1360", h(B, "x", 5) + h(A, "x", 6), {("ab", PROX): {"x": 1}, ("ab", ANY): {"x": (2, 1)}}),
    Cell("tail_of_x", "the best run on field x's last hits, one hit behind it in y: cur_f changes, mrk_khits.h:923-925", h(A, "x", 2, 8) + h(B, "x", 4, 9, end=9) + h(A, "y", 3),
         {("ab", PROX): {"x": 2, "y": 1}}),
    Cell("head_of_y", "the best run on field y's first hits, behind a lone hit in x: f_best restarts with the field, mrk_khits.h:923-927", h(B, "x", 7) + h(A, "y", 1, 5) + h(B, "y", 2),
         {("ab", PROX): {"x": 1, "y": 2}, ("ab", SPH): {"x": (1, 0, 0), "y": (2, 1, 0)}}),
    Cell("last_field", "the best run in the doc's last field: the weigh-in behind the loop, mrk_khits.h:951", h(A, "x", 3) + h(A, "top", 4) + h(B, "top", 5),
         {("ab", PROX): {"x": 1, "top": 2}, ("ab", FM): {"x": 1, "top": 1}}),
    Cell("only_top", "every hit in the last field: nothing is weighed in inside the loop, mrk_khits.h:951", h(A, "top", 1) + h(B, "top", 2, end=2),
         {("ab", PROX): {"top": 2}, ("ab", SPH): {"top": (2, 1, 1)}}),
    Cell("two_fields", "equal runs in two fields with different weights: :1363-1364, 1432, mrk_khits.h:924, 951", h(A, "x", 5) + h(B, "x", 6) + h(A, "z", 9) + h(B, "z", 10), {("ab", PROX): {"x": 2, "z": 2}}),
    Cell("shared_pos_flag", "a@1, a@2, b@2, b@3|END -- the END flag on the field's last POSITION: hits on position 2 arrive in query order, a@2 restarts the run and "
         "b@2 is no new position: 1; :1359-1360, mrk_khits.h:352, 922", h(A, "x", 1, 2) + h(B, "x", 2, 3, end=3), {("ab", PROX): {"x": 1}, ("ab", WC): {"x": 4}}),
    Cell("shared_kw_flag", "a@1, b@2, a@2|END, b@3|END -- the flag on each keyword's own last hit puts b@2 in FRONT of a@2|END: a@1 b@2 run to 2, a@2 sets the expected "
         "delta without growing, b@3 carries on: 3 with two keywords; mrk_kprune.h:213-220", h(A, "x", 1, 2, end=2) + h(B, "x", 2, 3, end=3),
         {("ab", PROX): {"x": 3}, ("ab", WC): {"x": 4}}),
    Cell("lim_between", "a field whose only hit is filtered, between two fields that count: `q && f != cur_f`, mrk_khits.h:923",
         h(A, "x", 3) + h(B, "x", 4) + h(B, "y", 1) + h(A, "z", 7) + h(B, "z", 8), {("a bXZ", PROX): {"x": 2, "z": 2}, ("ab", PROX): {"x": 2, "y": 1, "z": 2}}),
    Cell("lim_second", "a field-limited keyword whose filtered hit sits on the run's second position: AddHit searchnode.cpp:3032-3043, mrk_khits.h:917-922", h(A, "y", 5) + h(B, "y", 6) + h(B, "x", 20),
         {("a bX", PROX): {"y": 1, "x": 1}, ("ab", PROX): {"y": 2, "x": 1}}),
    # ---- SPH04
    Cell("head_0", "head hit in field 0: `1u << (f & 31)`, mrk_khits.h:320", h(A, "0", 1) + h(B, "0", 5), {("ab", SPH): {"0": (1, 1, 0)}}),
    Cell("head_x", "head hit in field x (7 / 8 in the wide segments): :1497-1499, mrk_khits.h:319-320", h(A, "x", 1) + h(B, "x", 5), {("ab", SPH): {"x": (1, 1, 0)}}),
    Cell("head_top", "head hit in the last field (31: the mask's top bit): :1499, 1522, mrk_khits.h:320, 375", h(B, "top", 1) + h(A, "top", 5), {("ab", SPH): {"top": (1, 1, 0)}, ("ab", FM): {"top": 1}}),
    Cell("head_shared", "position 1 reached by two keywords at once: :1497-1499, mrk_khits.h:319-320", h(A, "y", 1) + h(B, "y", 1), {("ab", SPH): {"y": (1, 1, 0)}}),
    Cell("exact", "the field is the whole query: exact hit, :1487-1491, mrk_khits.h:316", h(A, "x", 1) + h(B, "x", 2) + h(C, "x", 3, end=3),
         {("abc", SPH): {"x": (3, 1, 1)}, ("ab", SPH): {"x": (2, 1, 0)}}),
    Cell("exact_longer", "the field is one word longer: no exact hit, `GetPos == m_iMaxQuerypos` holds but the flag is on d; :1487-1489, mrk_khits.h:316", h(A, "x", 1) + h(B, "x", 2) + h(C, "x", 3) + h(D, "x", 4, end=4), {("abc", SPH): {"x": (3, 1, 0)}}),
    Cell("exact_azc", "the field is `a z c` for the query a b c: c keeps a's delta, so the delta test passes without b and the reference gives the exact bit; :1483, 1487-1491, mrk_khits.h:314-316",
         h(A, "x", 1) + h(Z, "x", 2) + h(C, "x", 3, end=3) + h(B, "z", 9), {("abc", SPH): {"x": (2, 1, 1), "z": (1, 0, 0)}}),
    Cell("single_flagged", "max_qpos == 1: a flagged lone hit at position 1 is head and exact, :1497-1501, mrk_khits.h:321", h(A, "y", 1, end=1), {("a", SPH): {"y": (1, 1, 1)}}),
    Cell("single_plain", "... an unflagged one is head only: :1500, mrk_khits.h:321", h(A, "y", 1) + h(Z, "y", 2, end=2), {("a", SPH): {"y": (1, 1, 0)}}),
    Cell("min_exp", "the second hit on the first one's position with the expected delta: `hp >= min_exp_pos` fails, the else branch, :1483, mrk_khits.h:314",
         h(A, "x", 1) + h(C, "x", 3) + h(B, "x", 3, end=3), {("a b@3 c@3", SPH): {"x": (2, 1, 0)}},
         note="b and c both at query position 3: b@3|END follows c@3 with c's delta but on c's position: else branch, no exact bit"),
    Cell("afresh_front", "the doc in front of `afresh`: its last hit lies in field 0 below position 9; Finalize keeps m_uMinExpPos, :1515-1517", h(A, "0", 2) + h(B, "0", 4), {("a b@10", SPH): {"0": (1, 0, 0)}}),
    Cell("afresh", "a first hit with delta -1 (field 0, position 9, query position 10) right behind a doc whose last hit lies below it: Finalize left "
         "m_iExpDelta = -1 and the old m_uMinExpPos, so the reference takes the `if` branch here; the device starts afresh (mrk_khits.h:293-295, 314)",
         h(B, "0", 9) + h(A, "0", 20), {("a b@10", SPH): {"0": (1, 0, 0)}}),
    # ---- MATCHANY
    Cell("any_lcs1", "a field with a mask but LCS 1: (lcs - 1) x phrase_k = 0, :1609", h(A, "x", 5) + h(B, "z", 5), {("ab", ANY): {"x": (1, 1), "z": (1, 1)}, ("a|b", ANY): {"x": (1, 1), "z": (1, 1)}}),
    Cell("any_hi_qpos", "query positions 9 and 32 fall off the byte: `& 0xffu`, mrk_khits.h:353", h(A, "x", 5) + h(B, "x", 13) + h(C, "y", 2),
         {("a b@9 c@32", ANY): {"x": (1, 2), "y": (0, 1)}}, note="a@5 q1 and b@13 q9 share a delta: LCS 2 with ONE bit; field y has a hit and no bit: it adds nothing"),
    # ---- repeated keywords
    Cell("dup_aba", "a b a over `a b a`: RankerState_Proximity_fn<.., true>, :1372-1411, mrk_khits.h:330-349", h(A, "x", 5, 7) + h(B, "x", 6),
         {("aba", PROX): {"x": 3}, ("aba", WC): {"x": 5}, ("aba", FM): {"x": 1}, ("aba", SPH): {"x": (1, 0, 0)}, ("aba", ANY): {"x": (3, 1)}},
         note="HC.dupes is true for the proximity pair only: SPH04 and MATCHANY see every position of a twice and the second arrival resets the expected delta, 1"),
    Cell("dup_aaaa", "a a / a a b over `a a a a b`: the run reaches 2 on the second position and is never reset (`cur_lcs < 2` is the only restart, :1383): its tail "
         "stays on position 4, query position 2, and neither a later a nor the b lines up with it", h(A, "x", 3, 4, 5, 6) + h(B, "x", 7),
         {("aa", PROX): {"x": 2}, ("aab", PROX): {"x": 2}, ("aab", ANY): {"x": (3, 2)}}, note="MATCHANY (the update without duplicates): a@6 at query position 2 and b@7 run to 2, three bits, and phrase_k "
         "counts the two DISTINCT words, :1588.  a a b finds 2, not the 3 of a@5 a@6 b@7: the reference's FIXME at :1382"),
    Cell("dup_abab", "a b a b over `a b a b`: 4; :1399-1410, mrk_khits.h:342-348", h(A, "y", 5, 7) + h(B, "y", 6, 8), {("abab", PROX): {"y": 4}}),
    Cell("dup_next_field", "a run that would continue into the next field: the mask resets, :1376", h(A, "x", 5) + h(B, "x", 6, end=6) + h(A, "y", 7), {("aba", PROX): {"x": 2, "y": 1}}),
    Cell("dup_third", "the `cur_lcs < 2` rule on the third position: a run of 2 keeps its tail when a stray hit comes, :1383", h(A, "x", 5, 9) + h(B, "x", 6, 10),
         {("aba", PROX): {"x": 2}}),
    Cell("dup_far30", "tail distance 30: query position 31 is the mask's last bit, :1396-1400", h(A, "x", 5) + h(B, "x", 35), {("a a b@31", PROX): {"x": 2}}),
    Cell("dup_far31", "tail distance 31: query position 32 adds no bit; :1396, mrk_khits.h:341", h(A, "x", 5) + h(B, "x", 36), {("a a b@32", PROX): {"x": 1}}),
    Cell("dup_far32", "tail distance 32: `delta < 32`; :1400, mrk_khits.h:343", h(A, "x", 5) + h(B, "x", 37), {("a a b@33", PROX): {"x": 1}}),
    Cell("dup_q30", "query positions 30, 31 and 32 (31, 32, 33) next to each other: `1ull << (hq & 63)` into a DWORD, mrk_khits.h:341", h(A, "y", 5, 7) + h(B, "y", 6),
         {("a@30 b@31 a@32", PROX): {"y": 2}, ("a@31 b@32 a@33", PROX): {"y": 1}}),
    # ---- WORDCOUNT / FIELDMASK
    Cell("fm_top_only", "a hit in the last field: FIELDMASK's weight is negative with 32 fields, `(int)fmask`, mrk_khits.h:361", h(A, "top", 3) + h(B, "top", 9), {("ab", FM): {"top": 1}}),
    Cell("tf300", "300 hits of one keyword over three fields: the tf escape counts all of them; exc_tf mrk_kprune.h:248-259, :1634", h(A, "x", *range(2, 202, 2)) + h(A, "y", *range(2, 202, 2)) + h(A, "z", *range(2, 202, 2)) + h(B, "z", 3),
         {("ab", WC): {"x": 100, "y": 100, "z": 101}, ("ab", PROX): {"x": 1, "y": 1, "z": 2}}),
    Cell("tf255", "255 hits of one keyword in one field: ktf = 255 stands for 255 or more; mrk_kprune.h:230, 259", h(A, "y", *range(2, 512, 2)) + h(B, "y", 600), {("ab", WC): {"y": 256}, ("ab", PROX): {"y": 1}}),
    # ---- folded hits (queue 1): compared with the oracle and these figures, not with the flat model
    Cell("fold_abc", '"a b" c over `a b c`: the phrase folds into ONE hit on a\'s position with weight 2 and spanlen 2 (searchnode.cpp:3932-3939), so the ranker expects '
         "the next delta one HIGHER (:1367, `why spanlen??`) and the c directly behind the phrase does not continue the run: 2, not 3",
         h(A, "x", 5) + h(B, "x", 6) + h(C, "x", 7), {('"a b" c', PROX): {"x": 2}, ('"a b" c', SPH): {"x": (2, 0, 0)}, ('"a b" c', WC): {"x": 2}, ('"a b c"~2', PROX): {"x": 3}, ('"a b c"~2', WC): {"x": 1}}),
    Cell("fold_ab_c", '... `a b _ c`: the c one position further is the one that continues the folded hit: weight 2 plus 1 = one run of 3; :1367, mrk_khits.h:357; under "a b c"~2 two of the three words keep the query\'s offsets: 2',
         h(A, "y", 5) + h(B, "y", 6) + h(C, "y", 8), {('"a b" c', PROX): {"y": 3}, ('"a b" c', SPH): {"y": (3, 0, 0)}, ('"a b c"~2', PROX): {"y": 2}, ('"a b c"~2', WC): {"y": 1}}),
    Cell("fold_acb", '`a c b`: "a b c"~2 out of order -- no two words keep the query\'s offsets, the one folded hit weighs 1 (the three possible weights: fold_abc 3, '
         "fold_ab_c 2, this 1); searchnode.cpp:4055, mrk_khits.h:667", h(A, "y", 5) + h(C, "y", 6) + h(B, "y", 7), {('"a b c"~2', PROX): {"y": 1}, ('"a b c"~2', WC): {"y": 1}}),
    Cell("fold_near", "a NEAR/2 b feeding SPH04: ONE hit of weight 2 on a's position 1 -- LCS 2, the head bit, no exact bit (max_qpos is 2, the folded hit's query position 1); "
         "searchnode.cpp:4255-4270, :1496-1499, mrk_khits.h:318-320", h(A, "z", 1) + h(B, "z", 3, end=3),
         {("a near/2 b", PROX): {"z": 2}, ("a near/2 b", SPH): {"z": (2, 1, 0)}, ("a near/2 b", WC): {"z": 1}, ("a near/2 b", FM): {"z": 1}}),
]
CELL_BY_NAME = {c.name: c for c in CELLS}
FILLERS = 24  # docs that hold z alone, between the cells: no query here matches them


@functools.lru_cache(maxsize=None)
def corpus(name):
    """-> (docs_hits in rowid order: [{term: [raw hit]}], {cell name: rowid})"""
    roles = roles_of(name)
    docs = []
    for c in CELLS:
        hits = {}
        for t, role, p, flagged in c.hits:
            hits.setdefault(t, []).append((roles[role] << 24) | (END if flagged else 0) | p)
        docs.append((c.name, {t: sorted(v) for t, v in hits.items()}))
    perm = np.random.default_rng(PERM_SEED + len(name)).permutation(len(docs))
    docs = [docs[i] for i in perm]
    # `afresh` stands right behind `afresh_front`: the pair is moved to the end as a pair
    pair = [d for d in docs if d[0] == "afresh_front"] + [d for d in docs if d[0] == "afresh"]
    docs = [d for d in docs if d[0] not in ("afresh_front", "afresh")]
    out, names = [], {}
    for i, (nm, hits) in enumerate(docs + pair):
        if i % 2 and len(out) < len(docs) + FILLERS and nm != "afresh":
            out.append({Z: [(roles["x"] << 24) | 3]})
        names[nm] = len(out)
        out.append(hits)
    assert len(out) <= 1000 and names["afresh"] == names["afresh_front"] + 1
    return out, names


def hits_arrays(docs_hits):
    rows = sorted((t + 1, r, hp) for r, hits in enumerate(docs_hits) for t, hs in hits.items() for hp in hs)
    a = np.array(rows, np.uint64)
    return a[:, 0].copy(), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def segment(name):
    """-> (HostIndex, docs_hits, {cell: rowid})"""
    import manticoresearch_amd as m

    _, nf, fmt, block, _ = next(s for s in SEGMENTS if s[0] == name)
    docs, names = corpus(name)
    W, R, Hh = hits_arrays(docs)
    return m.index_from_hits(W, R, Hh, n_terms=N_TERMS, total_docs=len(docs), skiplist_block_size=block, hit_format=fmt, n_fields=nf), docs, names


# --------------------------------------------------------------------------- the query shapes
def shapes(m, name):
    """-> {shape: (root, route under the proximity pair, route under SPH04 / WORDCOUNT / MATCHANY / FIELDMASK, rankers it may not run under)}
    routes: P = hit_rank_prox<2/3/4>, L = hit_rank_plain, F = hit_pass, G = the generic evaluator, B = no hit pass at all"""
    r = roles_of(name)
    kw = m.XQNode.keyword
    AND = m.XQNode.AND

    def OR(*k):
        return m.XQNode(m.SPH_QUERY_OR, list(k))

    def mask(*roles):
        return sum(1 << r[x] for x in roles)

    no_any = (m.SPH_RANK_MATCHANY,)
    out = {
        "ab": (AND(kw(A, 1), kw(B, 2)), "P", "L", ()),
        "ba": (AND(kw(B, 1), kw(A, 2)), "P", "L", ()),
        "a1b3": (AND(kw(A, 1), kw(B, 3)), "P", "L", ()),
        "a|b": (OR(kw(A, 1), kw(B, 2)), "P", "L", ()),
        "abc": (AND(kw(A, 1), kw(B, 2), kw(C, 3)), "P", "L", ()),
        "abcd": (AND(kw(A, 1), kw(B, 2), kw(C, 3), kw(D, 4)), "P", "L", ()),
        "a bX": (AND(kw(A, 1), kw(B, 2, mask("x"))), "P", "L", ()),
        "a bXZ": (AND(kw(A, 1), kw(B, 2, mask("x", "z"))), "P", "L", ()),
        "a bX c d": (AND(kw(A, 1), kw(B, 2, mask("x")), kw(C, 3), kw(D, 4)), "P", "L", ()),
        "a": (kw(A, 1), "B", "L", ()),
        "a b@3 c@3": (AND(kw(A, 1), kw(B, 3), kw(C, 3)), "P", "L", ()),
        "a b@10": (AND(kw(A, 1), kw(B, 10)), "P", "L", ()),
        "a b@9 c@32": (AND(kw(A, 1), kw(B, 9), kw(C, 32)), "P", "L", ()),
        "aba": (AND(kw(A, 1), kw(B, 2), kw(A, 3)), "L", "L", ()),
        "aa": (AND(kw(A, 1), kw(A, 2)), "L", "L", ()),
        "aab": (AND(kw(A, 1), kw(A, 2), kw(B, 3)), "L", "L", ()),
        "abab": (AND(kw(A, 1), kw(B, 2), kw(A, 3), kw(B, 4)), "L", "L", ()),
        "a a b@31": (AND(kw(A, 1), kw(A, 2), kw(B, 31)), "L", "L", ()),
        "a a b@32": (AND(kw(A, 1), kw(A, 2), kw(B, 32)), "L", "L", ()),
        "a a b@33": (AND(kw(A, 1), kw(A, 2), kw(B, 33)), "L", "L", no_any),
        "a@30 b@31 a@32": (AND(kw(A, 30), kw(B, 31), kw(A, 32)), "L", "L", ()),
        "a@31 b@32 a@33": (AND(kw(A, 31), kw(B, 32), kw(A, 33)), "L", "L", no_any),
    }
    for n, key in ((5, "a-e"), (6, "a-f"), (7, "a-g"), (8, "a-h")):
        out[key] = (AND(*[kw(t, t + 1) for t in range(n)]), "G", "G", ())
    # folded hits
    ph = m.XQNode(m.SPH_QUERY_PHRASE, [kw(A, 1), kw(B, 2)])
    no_hits = (m.SPH_RANK_BM25, m.SPH_RANK_NONE)  # (without a hit ranker a phrase leaf is decided inside the scan: another pass, not this suite's)
    out['"a b" c'] = (AND(ph, kw(C, 3)), "F", "F", no_hits)
    out['"a b c"~2'] = (m.XQNode(m.SPH_QUERY_PROXIMITY, [kw(A, 1), kw(B, 2), kw(C, 3)], None, m.ALL_FIELDS, 2), "F", "F", no_hits)
    out["a near/2 b"] = (m.XQNode(m.SPH_QUERY_NEAR, [kw(A, 1), kw(B, 2)], None, m.ALL_FIELDS, 2), "F", "F", no_hits)
    return out


def ranker_family(m):
    return {m.SPH_RANK_PROXIMITY_BM25: PROX, m.SPH_RANK_PROXIMITY: PROX, m.SPH_RANK_SPH04: SPH, m.SPH_RANK_MATCHANY: ANY, m.SPH_RANK_WORDCOUNT: WC,
            m.SPH_RANK_FIELDMASK: FM}


def all_rankers(m):
    return (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_BM25, m.SPH_RANK_NONE, m.SPH_RANK_WORDCOUNT, m.SPH_RANK_PROXIMITY, m.SPH_RANK_MATCHANY, m.SPH_RANK_FIELDMASK,
            m.SPH_RANK_SPH04)


def route_of(m, shape_row, ranker):
    _, prox_route, plain_route, _ = shape_row
    if ranker in (m.SPH_RANK_BM25, m.SPH_RANK_NONE):
        return "B"  # (no hit pass: 5..8 keywords under BM25 are the block scan's too)
    return prox_route if ranker in (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_PROXIMITY) else plain_route


def queries(m, name, max_matches=(1000, 3, 1), sets=None, index_weights=(1,)):
    """-> {route: [(shape, weight set, Query)]}: every shape x every ranker it may run under x max_matches (>= the docs, 3 and 1) x weight set at the first
    index weight, and once more per further index weight (max_matches 1000, the set with a 0 and a negative)"""
    out = {}
    ws = weight_sets(name)
    combos = [(mm, wname, index_weights[0]) for mm in max_matches for wname in sets or ws] + [(1000, "mixed", iw) for iw in index_weights[1:]]
    for shape, row in shapes(m, name).items():
        for rk in all_rankers(m):
            if rk in row[3]:
                continue
            for mm, wname, iw in combos:
                out.setdefault(route_of(m, row, rk), []).append((shape, wname, m.Query(row[0], ranker=rk, max_matches=mm, field_weights=ws[wname], index_weight=iw)))
    # FIELDMASK's weight is negative where a hit lies in field 31: max_matches that cut exactly between the positive and the negative weights, and one row on
    for shape in ("ab", "a|b"):
        row = shapes(m, name)[shape]
        k = fieldmask_positive(m, name, row[0])
        for mm in (k, k + 1):
            out[route_of(m, row, m.SPH_RANK_FIELDMASK)].append((shape, "none", m.Query(row[0], ranker=m.SPH_RANK_FIELDMASK, max_matches=mm)))
    return out


def fieldmask_positive(m, name, root):
    """the matches of a flat query whose FIELDMASK weight is positive: no hit of the stream lies in field 31"""
    docs, _ = corpus(name)
    kws = keywords_of(root)
    match_all = root.word is not None or root.op == m.SPH_QUERY_AND
    return sum(1 for hits in docs if matches(hits, kws, match_all) and all(field_of(hp) != 31 for hp, _ in stream(hits, kws)))


def cell_rank(m, name, cell, shape, ranker, field_weights, n_qwords):
    """the hand-stated rank part of a cell under (shape, ranker), from the row's per-role figures:
    prox {role: lcs}; sph04 {role: (lcs, head, exact)}; matchany {role: (bits, lcs)}; wordcount {role: hits}; fieldmask {role: 1}"""
    fam = ranker_family(m)[ranker]
    figures = cell.expect[(shape, fam)]
    r, nf = roles_of(name), next(s for s in SEGMENTS if s[0] == name)[1]
    w = [(field_weights[i] if field_weights is not None and i < len(field_weights) else 1) for i in range(nf)]
    if fam == FM:
        return i32(sum(1 << r[role] for role in figures))
    if fam == ANY:
        pk = sum(w) * n_qwords
        return sum((bits + (lcs - 1) * pk) * w[r[role]] for role, (bits, lcs) in figures.items() if bits)
    if fam == SPH:
        return sum((4 * l + 2 * hd + ex) * w[r[role]] for role, (l, hd, ex) in figures.items())
    return sum(v * w[r[role]] for role, v in figures.items())


# --------------------------------------------------------------------------- prox_bounds, restated (csrc/mrk_kprune.h)
def popcount(v):
    return bin(v).count("1")


def prox_bounds(kf, ktf, emit, fw, by_keywords):
    """-> (lo, hi) of the rank part sum_f LCS[f] x w[f]: kf[k] = the fields keyword k occurs in (its doclist entry's mask), ktf[k] = min(hits, 255),
    emit = bit k: keyword k's hits reach the ranker, fw = the weights of the fields the bound walks"""
    room = [(1 if by_keywords else ktf[k] - popcount(kf[k]) + 1) if (emit >> k) & 1 else 0 for k in range(len(kf))]
    lo = hi = 0
    for f, w in enumerate(fw):
        hh = sum(room[k] for k in range(len(kf)) if (kf[k] >> f) & 1)
        one = 1 if hh > 0 else 0
        lo += w * one if w >= 0 else w * hh
        hi += w * hh if w >= 0 else w * one
    return lo, hi


def doc_bound_inputs(hits, terms):
    """what the doclists say of one doc: per keyword the field mask and min(hit count, 255)"""
    kf = [sum(1 << f for f in {field_of(x) for x in hits.get(t, ())}) for t in terms]
    ktf = [min(len(hits.get(t, ())), 255) for t in terms]
    emit = sum(1 << k for k, t in enumerate(terms) if hits.get(t))
    return kf, ktf, emit


def bounds_fit(fw, index_weight):
    """scan_bt_kernel's guard: the bounds are 32-bit like the weights (mrk_scan_bt.hip:131-133)"""
    return (sum(abs(w) for w in fw) * 1020 * 1000 + 1000) * index_weight < (1 << 32)


def tiny_docs(flag_by_position):
    """every doc of 2 keywords x 2 fields x positions 1..3: each keyword holds any subset of the six (field, position) places; the END flag
    stands on a field's last occupied POSITION, for every keyword there (the reference's indexer), or on each keyword's own last hit of a field"""
    places = [(f, p) for f in (0, 1) for p in (1, 2, 3)]
    subsets = [[pl for i, pl in enumerate(places) if (bits >> i) & 1] for bits in range(64)]
    for sa in subsets:
        for sb in subsets:
            if not sa and not sb:
                continue
            hits = {}
            for t, s in ((A, sa), (B, sb)):
                lst = []
                for f, p in s:
                    if flag_by_position:
                        last = max(pp for ff, pp in sa + sb if ff == f)
                    else:
                        last = max(pp for ff, pp in s if ff == f)
                    lst.append((f << 24) | (END if p == last else 0) | p)
                if lst:
                    hits[t] = sorted(lst)
            yield hits


# --------------------------------------------------------------------------- the bounds corpus (8 fields: the tree kernel is the narrow segments')
BOUNDS_DOCS = 6000          # three 2048-rowid windows: every wave of a work item adds more than 256 lower bounds and recomputes the threshold
BOUNDS_FIELD = 2
BOUNDS_FW = {"pos": [1, 1, 3, 1, 1, 1, 1, 1], "neg": [1, 1, -3, 1, 1, 1, 1, 1],
             "neglead": [-9, -9, -3, -9, -9, -9, -9, -9]}  # every weight negative, field 2 the least so: its docs LEAD and the swapped ends lie on the cut
BOUNDS_GAP_QPOS = 11        # a@1 b@11 turns the tables: the fillers (a@10, b@20) run to 2 and the adjacent pair to 1
BOUNDS_EDGE_ROWS = 8        # the attaining docs stand on the class's lowest and highest rowids, and two in the middle
BOUNDS_LOW = range(1000, 3000)


def bounds_corpus(flag_by_position):
    """-> (docs_hits, {kind: [rowids]}).  Every doc holds a and b; all but the tf docs hold each once or twice in ONE field, so the BM25 parts
    of a kind are identical and a kind's weights tie.
      filler    a@10, b@20 in field 2: LCS 1 = the lower end where the field's weight is positive, the upper end where it is negative
      low       the same in field 0 (weight 1): under BOUNDS_FW["pos"] its upper end (2) lies below the lower end of the field-2 docs (3) -- the docs the
                scan may drop; under "neg" it is the other way round
      adjacent  a@10 b@11 in field 2: LCS 2 = the hits of the field = the upper end by hits and by keywords (the lower end under "neg")
      shared3   a@1, b@2, a@2, b@3 in field 2.  Flagged by keyword (a@2|END, b@3|END) the run is 3 with two keywords: inside the bound by hits
                (4), ABOVE the bound by keywords (2).  Flagged by position (b@3|END alone) the same places run to 1
      tf255     a with 255 hits in field 2 (the packed tf saturates), tf300: a with 300 hits over fields 1, 2, 3 (the escape)"""
    f = BOUNDS_FIELD << 24
    docs = [{A: [f | 10], B: [f | 20]} for _ in range(BOUNDS_DOCS)]
    for r in BOUNDS_LOW:
        docs[r] = {A: [10], B: [20]}
    kinds = {"low": list(BOUNDS_LOW), "adjacent": [], "shared3": [], "tf255": [3600], "tf300": [3601]}
    edge = list(range(BOUNDS_EDGE_ROWS)) + list(range(BOUNDS_DOCS - BOUNDS_EDGE_ROWS, BOUNDS_DOCS)) + [3500, 3501]
    for i, r in enumerate(edge):
        kind = ("adjacent", "shared3")[i % 2]
        if kind == "adjacent":
            docs[r] = {A: [f | 10], B: [f | 11]}
        else:
            docs[r] = {A: [f | 1, f | (0 if flag_by_position else END) | 2], B: [f | 2, f | END | 3]}
        kinds[kind].append(r)
    docs[3600] = {A: [f | p for p in range(30, 30 + 2 * 255, 2)], B: [f | 20]}
    docs[3601] = {A: [(ff << 24) | p for ff in (1, 2, 3) for p in range(30, 230, 2)], B: [f | 20]}
    taken = {r for v in kinds.values() for r in v}
    kinds["filler"] = [r for r in range(BOUNDS_DOCS) if r not in taken]
    return docs, kinds


@functools.lru_cache(maxsize=None)
def bounds_segment(flag_by_position):
    import manticoresearch_amd as m

    docs, kinds = bounds_corpus(flag_by_position)
    W, R, Hh = hits_arrays(docs)
    return m.index_from_hits(W, R, Hh, n_terms=N_TERMS, total_docs=len(docs), skiplist_block_size=128, hit_format=1, n_fields=8), docs, kinds
