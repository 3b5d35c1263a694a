"""Shared by tests/test_gpu_runtime_declines.py and its ShardMerger worker: hand-made corpora around the caps of the phrase state
machines (PHRASE_STATES = 8 in mrk_khits.h, GEN_FSM_STATES = 32 in mrk_keval.h) and of the generic evaluator's hit-list memory,
the queries that reach them, and the exchange rows the oracle's answers make.  Nothing here runs on the device."""
import dataclasses

import numpy as np

import order_merge_common as omc
import sort_merge_common as smc
from sorted_expect import expected_order, expected_sort
from test_gpu_parity import kw, orc_index_of, to_orc

K1 = 1024
LIVE_STATES = "more live phrase states"
ARENA = "gen_spill_mb"
# the context defaults (mrk_host_int.h) of the keys these tests change
DEFAULTS = {"path": 0, "bitmap_inv": 64, "bt_phrase": 1, "bt_cover_inv": 1024, "gen_lane_hits": 256, "gen_spill_mb": 1024}


class Settings:
    """ctx.set() for the block, the defaults back afterwards whatever happens."""

    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set(k, DEFAULTS[k])


class Hits:
    """(term, row, field, position) hits gathered in any order -> index_from_hits' sorted arrays"""

    def __init__(self):
        self.hits = set()

    def add(self, term, row, positions, field=0):
        for p in positions:
            assert 0 < p < (1 << 23)
            self.hits.add((term + 1, row, (field << 24) | int(p)))

    def index(self, m, n_terms, n_docs, n_fields=2, block=128, fmt=1):
        a = np.array(sorted(self.hits), dtype=np.uint64).reshape(-1, 3)
        return m.index_from_hits(a[:, 0], a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32), n_terms=n_terms, total_docs=n_docs,
                                 skiplist_block_size=block, hit_format=fmt, n_fields=n_fields)

    def __len__(self):
        return len(self.hits)


def dead_map(n_docs, rows):
    dead = np.zeros((n_docs + 31) // 32, np.uint32)
    rows = np.asarray(sorted(rows), dtype=np.int64)
    if len(rows):
        np.bitwise_or.at(dead, rows >> 5, (np.uint32(1) << (rows & 31).astype(np.uint32)))
    return dead


def PHRASE(m, *words):
    return m.XQNode(m.SPH_QUERY_PHRASE, list(words))


# ------------------------------------------------------------------ 1. the specialised phrase path (PHRASE_STATES = 8)
A, B, C_, D = 0, 1, 2, 3  # keywords of the small-gap corpus: a ... b, c between them in the 3-word phrases, d for the AND
SMALL_GAPS = range(1, 8)


def small_gap_corpus():
    """-> (Hits, n_docs).  For every gap g in 1..7 and every run length r in {1, g, g+1, g+2, 8, 9, 20}: a doc with `a` at 1..r and
    one `b` at r+g (the phrase (1, 1+g) completes on the LAST a, whose state is the newest of the run's), one with the b at r+g+1 (no
    match), one with the b at 1+g inside the run (the FIRST a's state completes while later ones are live).  For "a c b" at (1, 2, 8)
    and (1, 7, 8): runs of a, one c or a run of c behind them, b where the last a's occurrence ends, or one further.  The longest
    run again in field 1 of docs of their own, and next to a short run in field 0.  d stands in every second doc."""
    H, row = Hits(), 0

    def doc(a_run, b_at, c_at=(), field=0):
        nonlocal row
        H.add(A, row, range(1, a_run + 1), field)
        H.add(B, row, b_at, field)
        H.add(C_, row, c_at, field)
        if row % 2 == 0:
            H.add(D, row, [50], 0)
        row += 1

    for g in SMALL_GAPS:
        for r in sorted({1, g, g + 1, g + 2, 8, 9, 20}):
            doc(r, [r + g])
            doc(r, [r + g + 1])
            if r >= g + 1:
                doc(r, [1 + g])
    for r in (1, 2, 7, 8, 9, 20):
        doc(r, [r + 7], [r + 1])                   # (1, 2, 8) on the last a
        doc(r, [r + 7], range(2, r + 2))           # ... a c behind every a: r states wait for their b
        doc(r, [r + 8], range(2, r + 2))           # ... and no b where any of them expects it
        doc(r, [r + 7], [r + 6])                   # (1, 7, 8) on the last a
        doc(r, [r + 7], range(7, r + 7))
        doc(r, [r + 8], range(7, r + 7))
    for g in (1, 7):
        doc(20, [20 + g], field=1)
        doc(20, [20 + g + 1], field=1)
    H.add(A, row, range(1, 10), 0), H.add(B, row, [16], 0), H.add(A, row, range(1, 21), 1), H.add(B, row, [28], 1)
    row += 1
    return H, row


def small_gap_queries(m):
    """-> (queries, spans): every 2-word gap and both 3-word phrases, BM25 and PROXIMITY_BM25, at the root and under an AND with d."""
    phrases = [((1, 1 + g), lambda g=g: PHRASE(m, kw(m, A, 1), kw(m, B, 1 + g))) for g in SMALL_GAPS]
    phrases.append(((1, 2, 8), lambda: PHRASE(m, kw(m, A, 1), kw(m, C_, 2), kw(m, B, 8))))
    phrases.append(((1, 7, 8), lambda: PHRASE(m, kw(m, A, 1), kw(m, C_, 7), kw(m, B, 8))))
    qs, spans = [], []
    for atoms, make in phrases:
        for rk in (m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25):
            qs.append(m.Query(make(), ranker=rk))
            qs.append(m.Query(m.XQNode.AND(make(), kw(m, D, 10)), ranker=rk))
            spans += [atoms[-1] - atoms[0]] * 2
    return qs, spans


# ------------------------------------------------------------------ 2. the generic evaluator (GEN_FSM_STATES = 32)
N_W = 5          # w0 .. w4: the words of the 5-word phrases
X, Y = 5, 6      # two ordinary keywords for the healthy queries
WIDE_GAPS = (30, 31, 32, 40)


def wide_runs(g):
    return (g, g + 1, g + 2, 64)


def add_healthy(H, rng, rows, atoms=None, every=9):
    """x and y at random places (1 - 3 hits each, most docs); every `every`-th doc also holds w0 .. w4 once, at `atoms`"""
    for i, row in enumerate(rows):
        if rng.random() < 0.8:
            H.add(X, row, rng.choice(np.arange(1, 30), int(rng.integers(1, 4)), replace=False), int(rng.integers(0, 2)))
        if rng.random() < 0.6 or i == 0:
            H.add(Y, row, rng.choice(np.arange(1, 30), int(rng.integers(1, 4)), replace=False), int(rng.integers(0, 2)))
        if atoms is not None and i % every == 0:
            for t in range(N_W):
                H.add(t, row, [100 + atoms[t]], 0)


def wide_atoms(g):
    return (1, 1 + g, 2 + g, 3 + g, 4 + g)


def wide_gap_corpus():
    """-> (Hits, n_docs, {(g, r): its rows}, healthy rows).  Per first gap g and run length r two docs: w0 at 1..r, then w1 .. w4 where
    the phrase (1, 1+g, 2+g, 3+g, 4+g) completes on the last w0 -- or one position late.  The other docs hold x / y and, some, the
    words once.  A w0 run trips every query with a wide gap, whatever g it was made for, so a case is run with the other cases' docs
    as dead rows."""
    H, rng, row, cases = Hits(), np.random.default_rng(7), 0, {}
    for g in WIDE_GAPS:
        for r in wide_runs(g):
            cases[(g, r)] = [row, row + 1]
            for late in (0, 1):
                H.add(0, row, range(1, r + 1))
                for t in range(1, N_W):
                    H.add(t, row, [r + g + (t - 1) + late])
                if late:
                    H.add(X, row, [3]), H.add(Y, row, [4])
                row += 1
    healthy = list(range(row, row + 150))
    add_healthy(H, rng, healthy, atoms=wide_atoms(30))
    return H, row + 150, cases, healthy


def phrase5(m, g):
    return PHRASE(m, *[kw(m, t, p) for t, p in enumerate(wide_atoms(g))])


def or_phrases(m, g):
    """'"w0 w1"(gap g) | "w2 w3"': two phrase nodes in one query run through the generic evaluator, whatever their spans"""
    return m.XQNode(m.SPH_QUERY_OR, [PHRASE(m, kw(m, 0, 1), kw(m, 1, 1 + g)), PHRASE(m, kw(m, 2, 2 + g), kw(m, 3, 3 + g))])


def prox5(m, qlen, dist=3):
    """'"w0 .. w4"~dist' whose query positions span qlen + 1"""
    pos = (1, qlen - 2, qlen - 1, qlen, qlen + 1)
    return m.XQNode(m.SPH_QUERY_PROXIMITY, [kw(m, t, p) for t, p in enumerate(pos)], opt=dist)


def healthy_and(m, **kwa):
    return m.Query(m.XQNode.AND(kw(m, X, 1), kw(m, Y, 2)), ranker=m.SPH_RANK_BM25, **kwa)


# ------------------------------------------------------------------ 3. exchange rows
KROWS = 50       # max_matches of every query of part 3, and the merges' k
ARENA_DOCS, ARENA_PER = 160, 20
FORMATS = ("narrow", "wide", "order")


def attr_rows(rng, n_docs):
    """[0] 0..9 (ties), [1] 0..999, [2..3] a unique 64-bit id"""
    rows = np.zeros((n_docs, 4), np.uint32)
    rows[:, 0] = rng.integers(0, 10, n_docs)
    rows[:, 1] = rng.integers(0, 1000, n_docs)
    rows[:, 2:4] = (np.int64(1 << 40) + np.arange(n_docs, dtype=np.int64) * 3).view(np.uint32).reshape(n_docs, 2)
    return rows


def the_sort(m):
    return m.Sort(0, 32, desc=True, then_weight=1)


def the_order(m):
    return m.Order([m.OrderPart(0, 32, desc=True), m.OrderPart(32, 32, desc=False)], then_weight=2)


@dataclasses.dataclass
class RowCorpus:
    """Two segments laid end to end: [0] holds what trips the declining query in front of healthy docs, [1] healthy docs only."""
    trigger: str
    his: list        # the two segments' indexes
    whole: object    # ... and the corpus in one index
    bases: list
    rows: np.ndarray  # attribute rows of the whole corpus
    n_trip: int
    gdocs: dict
    declining: object  # the tree of the declining query

    @property
    def n_docs(self):
        return len(self.rows)

    def seg_rows(self, s):
        return np.ascontiguousarray(self.rows[self.bases[s]:self.bases[s] + self.his[s].total_docs])

    def globalize(self, q):
        return dataclasses.replace(q, total_docs=self.n_docs, local_docs=dict(self.gdocs))


def row_corpus(m, trigger):
    """trigger "fsm": one doc with w0 at 1..64 under the phrase (1, 41, 42, 43, 44) -- 32 states opened by positions 1..32 are all
    live at position 33 (they expect w1 at 41..72), so GEN_FSM_STATES alone guarantees QF_FSM.  trigger "arena": ARENA_DOCS docs
    with ARENA_PER hits of each of w0 .. w4 under the phrase (1 .. 5), as test_gen_arena_limits_fail_loudly_then_recover builds
    them.  Per doc the evaluator takes 5 p hits for the words, 2 p + 3 p + 4 p + 5 p for their AND chain and 5 p for the phrase
    node, p = ARENA_PER: 24 p = 480, of which at most gen_lane_hits = 16 fit the lane's slice; the rest comes from the shared area,
    which is never handed back within a launch.  160 docs x 464 = 74 240 hits > the 65 536 that gen_spill_mb = 1 holds, for each
    query that runs the phrase on its own: the limit is met whatever the order of evaluation (142 docs would do; 160 leave 13 %)."""
    rng = np.random.default_rng(11 if trigger == "fsm" else 12)
    atoms = wide_atoms(40) if trigger == "fsm" else (1, 2, 3, 4, 5)
    n_trip = 1 if trigger == "fsm" else ARENA_DOCS
    n_a, n_b = n_trip + 120, 150
    parts, whole = [Hits(), Hits()], Hits()

    def both(s, term, row, positions, field=0):
        positions = list(positions)
        parts[s].add(term, row, positions, field)
        whole.add(term, row + (n_a if s else 0), positions, field)

    class Into:  # add_healthy writes through this
        def __init__(self, s):
            self.s = s

        def add(self, term, row, positions, field=0):
            both(self.s, term, row, positions, field)

    for row in range(n_trip):
        if trigger == "fsm":
            both(0, 0, row, range(1, 65))
            for t in range(1, N_W):
                both(0, t, row, [64 + 40 + t - 1])
        else:
            for t in range(N_W):
                both(0, t, row, [i * N_W + t + 1 for i in range(ARENA_PER)])
        both(0, X, row, [200]), both(0, Y, row, [201])
    add_healthy(Into(0), rng, range(n_trip, n_a), atoms=atoms)
    add_healthy(Into(1), rng, range(n_b), atoms=atoms)
    his = [parts[0].index(m, 7, n_a), parts[1].index(m, 7, n_b)]
    wi = whole.index(m, 7, n_a + n_b)
    gdocs = {t: int(wi.dict[t]["docs"]) for t in range(7)}
    assert all(gdocs[t] == int(his[0].dict[t]["docs"]) + int(his[1].dict[t]["docs"]) for t in range(7))
    return RowCorpus(trigger, his, wi, [0, n_a], attr_rows(np.random.default_rng(13), n_a + n_b), n_trip, gdocs,
                     lambda: PHRASE(m, *[kw(m, t, p) for t, p in enumerate(atoms)]))


def row_queries(m, c, with_declining=True):
    """-> (queries, indexes of the declining ones).  Healthy relevance queries in front and behind, a healthy Sort and a healthy
    Order; the declining phrase by relevance, sorted and ordered (a sorted / ordered query's wide and order rows are
    sort_select_kernel's, a relevance query's are pack_xrows_kernel's).  Without the declining ones: healthy queries in their place."""
    P = m.SPH_RANK_PROXIMITY_BM25
    bad = (lambda **kwa: m.Query(c.declining(), ranker=P, max_matches=KROWS, **kwa)) if with_declining else (lambda **kwa: healthy_and(m, max_matches=KROWS, **kwa))
    qs = [healthy_and(m, max_matches=KROWS), bad(), healthy_and(m, max_matches=KROWS, sort=the_sort(m)), bad(sort=the_sort(m)),
          healthy_and(m, max_matches=KROWS, order=the_order(m)), bad(order=the_order(m)),
          m.Query(m.XQNode(m.SPH_QUERY_OR, [kw(m, X, 1), kw(m, Y, 2)]), ranker=P, max_matches=KROWS)]
    return [c.globalize(q) for q in qs], ([1, 3, 5] if with_declining else [])


def words_of(mdist, fmt):
    return {"narrow": mdist.ROW_WORDS, "wide": mdist.SROW_WORDS, "order": mdist.OROW_WORDS}[fmt]


def carries(fmt, q):
    """whether the format has room for the query's order: narrow rows merge by relevance only, a wide row has no 64-bit key"""
    return fmt == "order" or (q.sort is None and q.order is None) or (fmt == "wide" and q.order is None)


def spec_word(mdist, fmt, q):
    if fmt == "narrow" or not carries(fmt, q):
        return 0
    if fmt == "wide":
        return mdist.sort_spec_word(q.sort.kind, q.sort.desc, q.sort.then_weight, q.sort.bit_count) if q.sort is not None else 0
    return omc.spec_of(mdist, q)


def declined_row(mdist, fmt, q, run_time):
    """No keys, count 0, MRK_ROW_DECLINED alone, a zero plane.  A query the format cannot carry leaves with spec word 0 (the host
    marks it at submit); one that was declined while it ran keeps the spec word it was planned under."""
    row = np.zeros(words_of(mdist, fmt), np.uint64)
    row[K1 + 1] = mdist.ROW_DECLINED
    if fmt != "narrow" and run_time:
        row[-1] = spec_word(mdist, fmt, q)
    return row


def answer_row(mdist, orc, fmt, oi, q, rows, base):
    """The exchange row of a healthy query from the oracle's answer on one index (global docids)."""
    if not carries(fmt, q):
        return declined_row(mdist, fmt, q, False)
    rid, w, mapped, raw, total = omc.answer(orc, to_orc, expected_order, expected_sort, oi, q, rows, len(rows))
    docid = rid.astype(np.int64) + base
    if fmt == "order":
        return omc.pack_orow(mdist, docid, w, total, omc.spec_of(mdist, q), mapped)
    wide = smc.pack_srow(mdist, docid, w, total, q.sort, raw)
    return wide if fmt == "wide" else np.ascontiguousarray(wide[:mdist.ROW_WORDS])


def expected_rows(mdist, orc, fmt, hi, qs, declining, rows, base):
    oi = orc_index_of(orc, hi)
    oi.attrs = rows
    return np.stack([declined_row(mdist, fmt, q, carries(fmt, q)) if i in declining else answer_row(mdist, orc, fmt, oi, q, rows, base) for i, q in enumerate(qs)])


def merge_model(mdist, fmt, rows_all, k):
    if fmt == "order":
        return mdist.merge_orows_np(rows_all, k)
    if fmt == "wide":
        return mdist.merge_srows_np(rows_all, k)
    wide = np.zeros(rows_all.shape[:2] + (mdist.SROW_WORDS,), np.uint64)  # (narrow rows: spec 0 and a zero plane)
    wide[..., :mdist.ROW_WORDS] = rows_all
    return np.ascontiguousarray(mdist.merge_srows_np(wide, k)[:, :mdist.ROW_WORDS])


def assert_declined_row(mdist, row, what, flags_allowed=None):
    """count 0, no keys, a zero plane; the total_found word one of flags_allowed (default: MRK_ROW_DECLINED alone)"""
    tot = int(row[K1 + 1])
    assert tot & (mdist.ROW_RERUN | mdist.ROW_DECLINED), (what, "a row without a flag", hex(tot), int(row[K1]))
    assert tot in (flags_allowed or (mdist.ROW_DECLINED,)), (what, hex(tot))
    assert int(row[K1]) == 0 and not row[:K1].any(), (what, "keys behind a flag", int(row[K1]))
    assert not row[K1 + 2:len(row) - (1 if len(row) > mdist.ROW_WORDS else 0)].any(), (what, "a plane behind a flag")


def assert_rows_equal(mdist, got, want, what):
    """row by row, the flags first: a flag that is missing or stale says more than a word offset"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for i in range(len(want)):
        g, w = int(got[i, K1 + 1]), int(want[i, K1 + 1])
        mask = mdist.ROW_RERUN | mdist.ROW_DECLINED
        assert g & mask == w & mask, (what, i, "flags", hex(g), hex(w), "count", int(got[i, K1]))
        assert int(got[i, K1]) == int(want[i, K1]) and g == w, (what, i, "count / total", int(got[i, K1]), int(want[i, K1]), g & ~mask, w & ~mask)
        bad = np.flatnonzero(got[i] != want[i])
        assert not len(bad), (what, i, "words", bad[:6].tolist(), [hex(int(x)) for x in got[i, bad[:3]]], [hex(int(x)) for x in want[i, bad[:3]]])
