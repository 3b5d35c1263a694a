"""Shared by tests/test_gen_edges_cpu.py and tests/test_gpu_gen_edges.py: hand-made corpora, queries and case tables around the
places where the generic per-doc evaluator (gen_eval, csrc/mrk_keval.h) can be off by one -- a second operand at
last + matchlen + dist - 1 and at + dist, pairs across a field boundary, the end flag (bit 23) inside a chain, two keywords on one
position, the orders in which a three-stream merge runs dry, rows around a quorum keyword's last doc, hit lists on the lane
arena's last slot, term frequencies around the 8-bit escape 255, and fields 8-31 of the WIDE instance.  Nothing here runs on the
device.

One doc is one cell of a ladder: Corpus.cells maps a cell's name to its row, and test_gen_edges_cpu.py checks every cell against
the position its name states.  Every corpus is built in the two forms of FORMS, so that a lone hit travels inline in the doclist
entry (ref >> 31) and through .spp; the corpora of parts 1-4 and 9 also in the layouts "wide17" and "wide32", where the chain
under test lies in field 16 / 31 (fb) and the field before it (fa).

Two shapes per case.  Where the planner (mrk_plan.cpp, build_tree) has a specialised path for the bare shape the case is asked
bare and wrapped: wrap() ORs a phrase over two keywords that never stand next to each other IN FRONT of the node.  The phrase comes
first because build_tree refuses a NEAR / NOTNEAR / BEFORE node behind a PHRASE leaf, while a NOTNEAR in front of one is accepted.
Whether a (tree, ranker) goes to the generic evaluator is stated here by route(), a restatement of build_tree / shape() for the
shapes of these tables; tests/cpp/gen_route.cpp asks mrk::plan_query itself for tree_flags & TF_GEN, and the CPU test compares
the two for every query, so the GPU test can sort the queries into pure batches and assert mrk_batch_stats.mq_chunks on each.
Where the route depends on the ranker (a quorum or a three-keyword AND below another operator, five and more keywords: generic
under the hit rankers only) the same tree is asked in both kinds of batch.

N.flags & 1 (the re-sort by descending query position, mrk_keval.h:202) is set by build_gen on the last AND of every PHRASE /
PROXIMITY / NEAR chain, so every wrapped n-way node reaches it; the docs of part 4 give it ties to sort.

A row's `matches` / `misses` name cells whose answer is stated by hand; the CPU test asks the oracle for them.  Part 5's three field
limits all hold the lowest field, so every order of running dry is a match of every part-5 row and reaches the merge.

Part 6: a real quorum of 8 keywords has no room for a second node (MRK_MAX_AND_TERMS = 8 keywords per query), so k = 8 is asked
at the root only.  Below AND / OR / MAYBE a quorum is generic under PROXIMITY_BM25 and specialised (scan_pk's quorum order code)
under BM25; below BEFORE it is generic under both.

Part 8, the search for a weight that depends on the docs in front: found under MATCHANY, whose weight counts the distinct query
positions of the folded hits -- TWO_ORDERS below is the doc, test_gen_edges_cpu.py asserts the dependence on the oracle, and the
ring corpus holds the doc directly behind an inserting doc and more than 2048 rows behind one, so a broken near_tab fails the
GPU test.  The other seven rankers showed no dependence on the same docs (a folded hit's query position reaches them through the
LCS delta only, and two chains of one doc never continue each other's LCS)."""
import dataclasses
import itertools
from typing import Callable, Optional, Tuple

import numpy as np

import runtime_declines_common as rd
from test_gpu_parity import kw

FORMS = [(128, 1), (32, 0)]
LAYOUTS = {"narrow": (3, 0), "wide17": (17, 15), "wide32": (32, 30)}  # name -> (n_fields, fa); fb = fa + 1
END = 1 << 23
MAXPOS = END - 1

# keywords
A, B, C = 0, 1, 2          # the operands of the ladders; C is the second word of a two-word phrase operand
E, F, G = 3, 4, 5          # the three-word proximity operand
P = (6, 7, 8, 9, 10)       # five words: the long proximity, the five-keyword AND, the quorum ties
X, Y = 11, 12              # the wrapper's words: never next to each other
DOT = 13                   # the unit keyword of SENTENCE / PARAGRAPH
NODOC = 15                 # in the dictionary's range, in no doc
N_TERMS = 16
Q8 = tuple(range(8))       # part 6: the quorum keywords of a corpus of their own

MAX_DOCS, MAX_HITS, MAX_BATCH = 2000, 100000, 256


class EndHits(rd.Hits):
    """Hits with hits that carry the end flag.  A flagged hit sorts behind every other hit of its field, so it has to be its
    keyword's last one there: index() asserts it."""

    def add_end(self, term, row, p, field=0):
        assert 0 < p < (1 << 23)
        self.hits.add((term + 1, row, (field << 24) | END | int(p)))

    def index(self, m, n_terms, n_docs, n_fields=2, block=128, fmt=1):
        last = {}
        for t, r, h in sorted(self.hits):
            key = (t, r, h >> 24)
            assert not last.get(key, 0) & END, ("a hit behind a flagged one", t - 1, r, h >> 24)
            last[key] = h
        return super().index(m, n_terms, n_docs, n_fields, block, fmt)


class Corpus:
    def __init__(self, key, layout="narrow"):
        self.key, self.layout = key, layout
        self.n_fields, self.fa = LAYOUTS[layout]
        self.fb, self.fz = self.fa + 1, (self.fa + 2) % self.n_fields
        self.H, self.cells, self.n, self.total_docs = EndHits(), {}, 0, None

    def doc(self, cell, wrap_words=True):
        """the next row becomes the cell; two rows of three hold x, two of three y, far apart in the third field"""
        assert cell not in self.cells, cell
        row = self.cells[cell] = self.n
        self.n += 1
        if wrap_words and row % 3 != 2:
            self.H.add(X, row, [900], self.fz)
        if wrap_words and row % 3 != 1:
            self.H.add(Y, row, [950], self.fz)
        return row

    def put(self, row, term, positions, field=None, end=False):
        field = self.fb if field is None else field
        positions = list(positions)
        if end:
            self.H.add(term, row, positions[:-1], field)
            self.H.add_end(term, row, positions[-1], field)
        else:
            self.H.add(term, row, positions, field)

    def hits_of(self, row, term):
        """[(field, position, flagged)] of one keyword in one doc, in index order"""
        return [(h >> 24, h & MAXPOS, bool(h & END)) for t, r, h in sorted(self.H.hits) if t == term + 1 and r == row]

    def index(self, m, block, fmt):
        return self.H.index(m, N_TERMS, self.total_docs or self.n, self.n_fields, block, fmt)

    def field_weights(self):
        return [(3, 0, -2, 5)[i % 4] for i in range(self.n_fields)]


# ------------------------------------------------------------------ trees
def PHRASE(m, *k, mask=0xFFFFFFFF):
    return m.XQNode(m.SPH_QUERY_PHRASE, list(k), None, mask)


def PROX(m, dist, *k):
    return m.XQNode(m.SPH_QUERY_PROXIMITY, list(k), opt=dist)


def NEAR(m, dist, *k):
    return m.XQNode(m.SPH_QUERY_NEAR, list(k), opt=dist)


def NOTNEAR(m, dist, a, b):
    return m.XQNode(m.SPH_QUERY_NOTNEAR, [a, b], opt=dist)


def BEFORE(m, *k):
    return m.XQNode(m.SPH_QUERY_BEFORE, list(k))


def QUORUM(m, thr, *k):
    return m.XQNode(m.SPH_QUERY_QUORUM, list(k), opt=thr)


def OR(m, *k):
    return m.XQNode(m.SPH_QUERY_OR, list(k))


def AND(m, *k):
    return m.XQNode(m.SPH_QUERY_AND, list(k))


def MAYBE(m, a, b):
    return m.XQNode(m.SPH_QUERY_MAYBE, [a, b])


def UNIT(m, op, unit_term, *k):
    return m.XQNode(op, list(k), unit_term=unit_term)


def wrap(m, node_from):
    """'"x y" | node': node_from(first free query position) -> the node"""
    return OR(m, PHRASE(m, kw(m, X, 1), kw(m, Y, 2)), node_from(3))


def keywords_of(n):
    return [n] if n.word is not None else [k for c in n.children for k in keywords_of(c)]


def route(m, root, ranker):
    """'G' = the generic evaluator (TF_GEN), 'S' = a specialised path: build_tree's and shape()'s declines (mrk_plan.cpp) for the
    shapes of these tables.  test_gen_edges_cpu.py holds it against plan_query for every query."""
    hit = ranker not in (m.SPH_RANK_NONE, m.SPH_RANK_BM25)
    nway = (m.SPH_QUERY_PHRASE, m.SPH_QUERY_PROXIMITY, m.SPH_QUERY_NEAR)
    st = {"ph": False, "notnear": False, "quorum_inner": False, "and3_inner": False, "gen": False, "termpos": False}

    def terms_only(n):
        return all(c.word is not None for c in n.children)

    def walk(n, is_root):
        if n.word is not None:
            st["termpos"] |= bool(n.term_pos())
            return
        k = len(n.children)
        if n.op in (m.SPH_QUERY_SENTENCE, m.SPH_QUERY_PARAGRAPH):
            st["gen"] = True
        elif n.op in nway:
            pos = [c.word.atom_pos for c in n.children if c.word is not None]
            if st["ph"] or not terms_only(n) or k > 4 or (n.op == m.SPH_QUERY_NEAR and k != 2) or (n.op != m.SPH_QUERY_NEAR and pos[-1] - pos[0] >= 8):
                st["gen"] = True
            st["ph"] = True
        elif n.op == m.SPH_QUERY_BEFORE:
            if st["ph"] or not terms_only(n) or k > 4:
                st["gen"] = True
            st["ph"] = True
        elif n.op == m.SPH_QUERY_NOTNEAR:
            if st["ph"] or st["notnear"] or not terms_only(n):
                st["gen"] = True
            st["notnear"] = True
        elif n.op == m.SPH_QUERY_QUORUM:
            if n.opt != 1 and n.opt < k:
                st["quorum_inner"] |= not is_root
                if any(c.field_mask != 0xFFFFFFFF for c in n.children):
                    st["gen"] = True  # (declined by both planners in fact: no such case in the tables)
        elif n.op == m.SPH_QUERY_AND and terms_only(n) and k > 1:
            st["and3_inner"] |= k == 3 and not is_root
        else:
            for c in n.children:
                walk(c, False)
            return
        for c in n.children:
            walk(c, False)

    walk(root, True)
    n = len(keywords_of(root))
    inner_ph = st["ph"] and root.op not in nway
    if st["gen"] or (hit and (n > 4 or st["quorum_inner"] or st["and3_inner"])) or ((inner_ph or st["notnear"] or st["termpos"]) and n > 4):
        return "G"
    return "S"


@dataclasses.dataclass
class Case:
    part: int
    name: str
    corpus: str                       # key of CORPORA
    make: Callable                    # (m, Corpus) -> XQNode
    edge: str                         # the edge, and the line of mrk_keval.h it aims at
    rankers: Optional[Tuple] = None   # None = all eight
    matches: Tuple = ()               # cells the tree must match, by hand (the CPU test asks the oracle)
    misses: Tuple = ()                # ... and cells it must not


def all_rankers(m):
    return (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_BM25, m.SPH_RANK_NONE, m.SPH_RANK_WORDCOUNT, m.SPH_RANK_PROXIMITY, m.SPH_RANK_MATCHANY,
            m.SPH_RANK_FIELDMASK, m.SPH_RANK_SPH04)


def queries_of(m, case, c):
    """every ranker x max_matches 1000 / 3 x field weights None / one set with a 0 and a negative"""
    out = []
    for rk in case.rankers or all_rankers(m):
        for mm in (1000, 3):
            for fw in (None, c.field_weights()):
                out.append(m.Query(case.make(m, c), ranker=rk, max_matches=mm, field_weights=fw))
    return out


def batches_of(m, cases, c):
    """-> [(route, [(case, Query)])]: pure batches of at most MAX_BATCH queries, and the number of queries in all"""
    by_route = {"S": [], "G": []}
    for case in cases:
        for q in queries_of(m, case, c):
            by_route[route(m, q.root, q.ranker)].append((case, q))
    out = []
    for r, qs in by_route.items():
        out += [(r, qs[i:i + MAX_BATCH]) for i in range(0, len(qs), MAX_BATCH)]
    return out, sum(len(v) for v in by_route.values())


def both(part, name, corpus, node_from, edge, rankers=None, matches=(), misses=()):
    """the case bare and wrapped"""
    return [Case(part, name, corpus, lambda m, c: node_from(m, c, 1), edge, rankers, matches, misses),
            Case(part, name + " wrapped", corpus, lambda m, c: wrap(m, lambda p: node_from(m, c, p)), edge, rankers, matches, misses)]


# ------------------------------------------------------------------ 1. distance ladders
DISTS = (1, 3)
BASE = 20
COMBOS = ("kk", "pk", "kp", "xk", "kx")   # left / right operand: k keyword, p two-word phrase, x three-word proximity
X_SPANS = (3, 4, 5)
OFFSETS = (0, 1, 2, 3)                      # the second operand starts at first + matchlen + D - 2 + o: o <= 1 is near enough
PX_DIST = 3                                 # of the three-word proximity operand: spans 3..5 lie within qlen + dist = 5


def operand_len(kind, span):
    return {"k": 1, "p": 2, "x": span}[kind]


def put_operand(c, row, kind, side, start, span):
    """left: a / "a c" / e f g;  right: b / "b c" / e f g"""
    if kind == "k":
        c.put(row, A if side == 0 else B, [start])
    elif kind == "p":
        c.put(row, A if side == 0 else B, [start]), c.put(row, C, [start + 1])
    else:
        c.put(row, E, [start]), c.put(row, F, [start + 1]), c.put(row, G, [start + span - 1])


def ladder_cells():
    for combo in COMBOS:
        for span in (X_SPANS if "x" in combo else (0,)):
            for D in DISTS:
                for behind in (True, False):
                    for o in OFFSETS:
                        yield combo, span, D, behind, o


def ladder_starts(combo, span, D, behind, o):
    """(start of the left operand, start of the right operand)"""
    ll, lr = operand_len(combo[0], span), operand_len(combo[1], span)
    return (BASE, BASE + ll + D - 2 + o) if behind else (BASE, BASE - lr - D + 2 - o)


def ladders(layout):
    c = Corpus("ladders", layout)
    for cell in ladder_cells():
        combo, span, D, behind, o = cell
        row = c.doc(("lad",) + cell)
        sl, sr = ladder_starts(*cell)
        put_operand(c, row, combo[0], 0, sl, span), put_operand(c, row, combo[1], 1, sr, span)
    for g in (1, 2, 3, 4):  # "a b a b" at the boundary distance of NEAR/1 .. NEAR/4: overlapping chains
        row = c.doc(("abab", g))
        c.put(row, A, [BASE, BASE + 2 * g]), c.put(row, B, [BASE + g, BASE + 3 * g])
    for D in DISTS:  # NOTNEAR: the not-hit on the must-hit's own position; (only in front of it: the ladders' front cells)
        row = c.doc(("nn_same", D))
        c.put(row, A, [BASE]), c.put(row, B, [BASE])
    for D in DISTS:  # '"p0 .. p4"~D': p1 .. p4 at 40 .. 43, p0 exactly at hpf - qlen - dist (dropped) and one later (kept)
        for kept in (0, 1):
            row = c.doc(("px_drop", D, kept))
            c.put(row, P[0], [43 - 4 - D + kept])
            for i in range(1, 5):
                c.put(row, P[i], [39 + i])
    for n, at in PX_WEIGHT_DOCS.items():  # n of the five words keep the query's relative offsets
        row = c.doc(("px_w", n))
        for i in range(5):
            c.put(row, P[i], [at[i]])
    return c


PX_WEIGHT_DOCS = {5: (30, 31, 32, 33, 34), 4: (30, 31, 32, 33, 35), 3: (30, 31, 32, 34, 36), 2: (31, 32, 34, 36, 30)}


def operand_node(m, kind, side, p):
    """-> (node, next free query position)"""
    if kind == "k":
        return kw(m, A if side == 0 else B, p), p + 1
    if kind == "p":
        return PHRASE(m, kw(m, A if side == 0 else B, p), kw(m, C, p + 1)), p + 2
    return PROX(m, PX_DIST, kw(m, E, p), kw(m, F, p + 1), kw(m, G, p + 2)), p + 3


def pair_node(m, op, D, combo, p, swap=False):
    if swap:  # (query positions ascend along the operands)
        l, p = operand_node(m, combo[1], 1, p)
        r, p = operand_node(m, combo[0], 0, p)
    else:
        l, p = operand_node(m, combo[0], 0, p)
        r, p = operand_node(m, combo[1], 1, p)
    return NEAR(m, D, l, r) if op == "near" else NOTNEAR(m, D, l, r)


def part1_cases():
    out = []
    for D in DISTS:
        for combo in COMBOS:
            out += both(1, f"near/{D} {combo}", "ladders", lambda m, c, p, D=D, combo=combo: pair_node(m, "near", D, combo, p),
                        "second operand at last + matchlen + dist - 1 / + dist, matchlen > 1: the new-chain test, mrk_keval.h:577")
            out += both(1, f"notnear/{D} {combo}", "ladders", lambda m, c, p, D=D, combo=combo: pair_node(m, "notnear", D, combo, p),
                        "not-hit at must + matchlen - 1 + dist and one later, on the must-hit, in front of it: mrk_keval.h:256")
        out += both(1, f"near/{D} kk swapped", "ladders", lambda m, c, p, D=D: pair_node(m, "near", D, "kk", p, True),
                    "the operands in the other query order: first_npos / first_qpos, mrk_keval.h:567, 604")
        out += both(1, f"notnear/{D} kk swapped", "ladders", lambda m, c, p, D=D: pair_node(m, "notnear", D, "kk", p, True),
                    "b as the must side: the ladders' front cells become its back cells, mrk_keval.h:255-256")
        out += both(1, f"proximity/{D} kk", "ladders", lambda m, c, p, D=D: PROX(m, D, kw(m, A, p), kw(m, B, p + 1)),
                    "two words at qlen + dist and one further: min_pos, mrk_keval.h:383-390")
        out.append(Case(1, f"proximity/{D} five words", "ladders", lambda m, c, D=D: PROX(m, D, *[kw(m, P[i], i + 1) for i in range(5)]),
                        "a word exactly at hpf - qlen - dist is dropped, one later kept; 2..5 words on the query's offsets: the delta sort, "
                        "mrk_keval.h:383-390, 399-424"))
    for D in (2, 4):
        out += both(1, f"near/{D} abab", "ladders", lambda m, c, p, D=D: NEAR(m, D, kw(m, A, p), kw(m, B, p + 1)),
                    "overlapping chains of a two-operand NEAR: a complete chain shifts, mrk_keval.h:601-608")
    return out


# ------------------------------------------------------------------ 2. field boundaries
def fields_corpus(layout):
    c = Corpus("fields", layout)
    row = c.doc("end_next")      # a on the last hit of field fa (flagged), b at position 1 of fb
    c.put(row, A, [7], c.fa, end=True), c.put(row, B, [1], c.fb)
    row = c.doc("end_next_c")    # ... with c as a's neighbour in fa: "a c"'s partner is in the next field
    c.put(row, A, [6], c.fa), c.put(row, C, [7], c.fa, end=True), c.put(row, B, [1], c.fb)
    for d in (0, 1):             # the same in-field position (and the next one) in neighbouring fields
        row = c.doc(("same_pos", d))
        c.put(row, A, [5], c.fa), c.put(row, B, [5 + d], c.fb)
    row = c.doc("maxpos")        # lone hits at 2^23 - 1: b closes "a b", and stands inside a < b < c by query position
    c.put(row, A, [MAXPOS - 1]), c.put(row, B, [MAXPOS]), c.put(row, C, [MAXPOS])
    row = c.doc("maxpos_end")    # ... flagged
    c.put(row, A, [MAXPOS - 1]), c.put(row, B, [MAXPOS], end=True)
    row = c.doc("bf_split")      # a in fa only, b in fb only
    c.put(row, A, [3], c.fa), c.put(row, B, [5], c.fb)
    row = c.doc("bf_started")    # a run started in fa, a complete one in fb
    c.put(row, A, [3], c.fa), c.put(row, A, [2], c.fb), c.put(row, B, [4], c.fb)
    for f in ("fa", "fb"):       # "a c b": c's field limit (fa only) cuts the chain's middle hit in fb
        row = c.doc(("cut_mid", f))
        for t, p in ((A, 5), (C, 6), (B, 7)):
            c.put(row, t, [p], getattr(c, f))
    row = c.doc("both_fields")   # first occurrence in fa, the chain in fb: FIELDMASK is 1 << field of the first occurrence
    c.put(row, A, [9], c.fa), c.put(row, A, [5], c.fb), c.put(row, B, [6], c.fb)
    return c


def part2_cases():
    out = []
    ab = {"phrase": lambda m, c, p: PHRASE(m, kw(m, A, p), kw(m, B, p + 1)), "proximity/2": lambda m, c, p: PROX(m, 2, kw(m, A, p), kw(m, B, p + 1)),
          "near/2": lambda m, c, p: NEAR(m, 2, kw(m, A, p), kw(m, B, p + 1)), "notnear/2": lambda m, c, p: NOTNEAR(m, 2, kw(m, A, p), kw(m, B, p + 1)),
          "before": lambda m, c, p: BEFORE(m, kw(m, A, p), kw(m, B, p + 1))}
    for name, f in ab.items():
        out += both(2, name + " a b", "fields", f, "a on field fa's last (flagged) hit, b at position 1 of fb; equal in-field positions in neighbouring fields; "
                    "2^23 - 1: positions compare with the field and without the flag, gen_pwf mrk_keval.h:56, 321, 377, 565; BEFORE's field test :691")
    out += both(2, "phrase a c b, c limited to fa", "fields", lambda m, c, p: PHRASE(m, kw(m, A, p), kw(m, C, p + 1, 1 << c.fa), kw(m, B, p + 2)),
                "a per-keyword field limit cuts the chain's middle hit: gen_term's field_queried, mrk_keval.h:99")
    out += both(2, "near/1 (a c) b across the boundary", "fields", lambda m, c, p: NEAR(m, 1, PHRASE(m, kw(m, A, p), kw(m, C, p + 1)), kw(m, B, p + 2)),
                "a phrase operand on the field's last hits, the keyword at position 1 of the next field: mrk_keval.h:577")
    out.append(Case(2, "near/2 a c b (the ring form)", "fields", lambda m, c: NEAR(m, 2, kw(m, A, 1), kw(m, C, 2), kw(m, B, 3)),
                    "the ring across a field boundary and at 2^23 - 1 on a shared position: mrk_keval.h:473-488", matches=(("cut_mid", "fa"), ("cut_mid", "fb")), misses=("end_next_c",)))
    out += both(2, "and a c b", "fields", lambda m, c, p: AND(m, kw(m, A, p), kw(m, C, p + 1, 1 << c.fa), kw(m, B, p + 2)),
                "the field test of the three-stream merge on a shared position 2^23 - 1: mrk_keval.h:179-185")
    return out


# ------------------------------------------------------------------ 3. the end flag inside chains
def flags_corpus(layout):
    c = Corpus("flags", layout)
    for which in (None, 0, 1, 2):   # "a c b" at 5, 6, 7: the flagged hit is the chain's first, middle, last element
        row = c.doc(("flag", which))
        for i, t in enumerate((A, C, B)):
            c.put(row, t, [5 + i], end=which == i)
    for flagged in (0, 1):          # a (flagged) directly in front of a dot, b behind the dot
        row = c.doc(("unit_flag", flagged))
        c.put(row, A, [5], end=bool(flagged)), c.put(row, DOT, [6]), c.put(row, B, [7])
    row = c.doc("sph04_exact")      # the phrase is the whole field and ends on its last hit
    c.put(row, A, [1]), c.put(row, B, [2], end=True)
    row = c.doc("flag_then_chain")  # a flagged a in fa, the chain in fb
    c.put(row, A, [4], c.fa, end=True), c.put(row, A, [5]), c.put(row, C, [6]), c.put(row, B, [7], end=True)
    return c


def part3_cases():
    out = []
    acb = lambda m, p: (kw(m, A, p), kw(m, C, p + 1), kw(m, B, p + 2))
    edge = "a flagged hit as the first, a middle, the last element of the chain: every comparison strips bit 23, mrk_keval.h:56, "
    out += both(3, "phrase a c b", "flags", lambda m, c, p: PHRASE(m, *acb(m, p)), edge + "321",
                # (the words' AND chain merges by RAW position, IsHitLess mrk_keval.h:110: a flagged first or middle hit arrives behind the chain's
                # later hits and the phrase does not line up; in an index the reference wrote a flagged hit is the field's last)
                matches=(("flag", None), ("flag", 2), "flag_then_chain"), misses=(("flag", 0), ("flag", 1)))
    out += both(3, "proximity/2 a c b", "flags", lambda m, c, p: PROX(m, 2, *acb(m, p)), edge + "377")
    out += both(3, "near/2 a c", "flags", lambda m, c, p: NEAR(m, 2, kw(m, A, p), kw(m, C, p + 1)), edge + "565")
    out += both(3, "near/2 c b", "flags", lambda m, c, p: NEAR(m, 2, kw(m, C, p), kw(m, B, p + 1)), edge + "565")
    out += both(3, "notnear/2 a b", "flags", lambda m, c, p: NOTNEAR(m, 2, kw(m, A, p), kw(m, B, p + 1)), "a flagged must-hit, a flagged not-hit two behind it: mrk_keval.h:254-256")
    out += both(3, "notnear/1 c a", "flags", lambda m, c, p: NOTNEAR(m, 1, kw(m, C, p), kw(m, A, p + 1)), "a flagged not-hit IN FRONT of the must-hit is no later hit: mrk_keval.h:255")
    out.append(Case(3, "near/2 a c b (the ring form)", "flags", lambda m, c: NEAR(m, 2, *acb(m, 1)), edge + "473, 488, 511, 530",
                    matches=(("flag", None), ("flag", 2), "flag_then_chain")))
    out.append(Case(3, "near/2 b c a (the ring form, the other arrival order)", "flags", lambda m, c: NEAR(m, 2, kw(m, B, 1), kw(m, C, 2), kw(m, A, 3)), edge + "473, 488",
                    matches=(("flag", None), ("flag", 2))))
    out += both(3, "before a c b", "flags", lambda m, c, p: BEFORE(m, *acb(m, p)), edge + "686, 690")
    out += both(3, "phrase a b", "flags", lambda m, c, p: PHRASE(m, kw(m, A, p), kw(m, B, p + 1)), "SPH04: a phrase that ends on the field's last hit, the flag goes to "
                "the ranker apart from the position: mrk_keval.h:746")
    for op in ("SENTENCE", "PARAGRAPH"):
        out.append(Case(3, op.lower() + " a b, flagged a in front of a dot", "flags",
                        lambda m, c, op=op: UNIT(m, getattr(m, "SPH_QUERY_" + op), DOT, kw(m, A, 1), kw(m, B, 2)),
                        "GN_UNIT compares raw positions: the flag counts, mrk_keval.h:287-302"))
    return out


# ------------------------------------------------------------------ 4. shared positions
AA_DOCS = ((10,), (10, 11), (10, 12), (10, 13), (10, 11, 12), (10, 12, 14), (10, 11, 13), (10, 13, 16))


def shared_corpus(layout):
    c = Corpus("shared", layout)
    for d in (0, 1, 2, 3):       # a and b on one position, and 1..3 apart
        row = c.doc(("ab", d))
        c.put(row, A, [10]), c.put(row, B, [10 + d])
    row = c.doc("ab_end")        # ... a's hit flagged, b's not
    c.put(row, A, [10], end=True), c.put(row, B, [10])
    for pre in (0, 1):           # a and "a c" start on one position; with an a in front there is a pre-last hit to roll back to
        row = c.doc(("rollback", pre))
        c.put(row, A, [8, 10] if pre else [10]), c.put(row, C, [11])
    for at in AA_DOCS:
        c.put(c.doc(("aa", at)), A, at)
    for name, at in AND5_DOCS.items():
        row = c.doc(("and5", name))
        for i in range(5):
            c.put(row, P[i], [at[i]])
    row = c.doc("q_flag_first")  # p0 (flagged) in front of p1 and p2: by raw position it would come last
    c.put(row, P[0], [10], end=True), c.put(row, P[1], [11]), c.put(row, P[2], [12])
    row = c.doc("q_tie")         # p0 (flagged) and p1 on one position: the quorum's merge goes by gen_pwf, then query position
    c.put(row, P[0], [10], end=True), c.put(row, P[1], [10]), c.put(row, P[2], [11])
    return c


AND5_DOCS = {"all_one": (10, 10, 10, 10, 10), "pairs": (10, 10, 11, 11, 12), "reversed": (14, 13, 12, 11, 10), "ends": (10, 12, 12, 12, 10)}


def part4_cases():
    out = []
    out += both(4, "near/2 a b", "shared", lambda m, c, p: NEAR(m, 2, kw(m, A, p), kw(m, B, p + 1)), "two keywords on one position: npos < first_npos, mrk_keval.h:566-569")
    out += both(4, "near/2 b a", "shared", lambda m, c, p: NEAR(m, 2, kw(m, B, p), kw(m, A, p + 1)), "... in the other query order: the dupe is not the leftmost, mrk_keval.h:570-575")
    out += both(4, "near/2 a (a c)", "shared", lambda m, c, p: NEAR(m, 2, kw(m, A, p), PHRASE(m, kw(m, A, p + 1), kw(m, C, p + 2))),
                "a and \"a c\" on the same start: the roll-back to the pre-last hit, mrk_keval.h:570-573")
    out.append(Case(4, "near/2 a (a c), the phrase at the lower query positions", "shared",
                    lambda m, c: NEAR(m, 2, kw(m, A, 3), PHRASE(m, kw(m, A, 1), kw(m, C, 2))),
                    "the roll-back itself: the chain's last AND emits ties in descending query position, so the phrase's hit arrives behind the keyword's "
                    "only when its query position is the lower one; then npos >= first_npos and prelast_p is set, mrk_keval.h:570-573"))
    out += both(4, "near/2 a a", "shared", lambda m, c, p: NEAR(m, 2, kw(m, A, p), kw(m, A, p + 1)), "a repeated keyword: every hit comes twice, mrk_keval.h:566-569, 591-599")
    out.append(Case(4, "near/2 a a a", "shared", lambda m, c: NEAR(m, 2, kw(m, A, 1), kw(m, A, 2), kw(m, A, 3)), "the ring form's dupe branch, mrk_keval.h:474-487"))
    out.append(Case(4, "and of five", "shared", lambda m, c: AND(m, *[kw(m, P[i], i + 1) for i in range(5)]), "ties of the k-stream merge go by query position, mrk_keval.h:179"))
    out.append(Case(4, "and of five, descending query positions", "shared", lambda m, c: AND(m, *[kw(m, P[i], 5 - i) for i in range(5)]),
                    "... with the operands given in descending query position, mrk_keval.h:179"))
    for thr in (2, 3):
        out += both(4, f"quorum {thr} of p0 p1 p2 p3", "shared", lambda m, c, p, thr=thr: QUORUM(m, thr, *[kw(m, P[i], p + i) for i in range(4)]),
                    "the quorum's merge: gen_pwf first, then query position, mrk_keval.h:658", matches=("q_flag_first", "q_tie"))
    out += both(4, "phrase a b", "shared", lambda m, c, p: PHRASE(m, kw(m, A, p), kw(m, B, p + 1)), "the re-sort by descending query position on a tie (N.flags & 1), mrk_keval.h:202-212")
    out += both(4, "proximity/2 b a", "shared", lambda m, c, p: PROX(m, 2, kw(m, B, p), kw(m, A, p + 1)), "... and the proximity node behind it, mrk_keval.h:202-212, 379-381")
    return out


# ------------------------------------------------------------------ 5. the three-stream merge
MERGE_TERMS = (A, B, C, E, F, G, P[0], P[1])


def merge_corpus(layout):
    """Per order in which the streams 0, 1, 2 (a, b, c) run dry: the first to end has hits in the lowest field only, the second in the two
    lowest, the third in all three; two hits per field, the three keywords interleaved.  Twice: the hits apart, and on shared
    positions.  The other five keywords (k = 5..8) stand once in every doc."""
    c = Corpus("merge", layout)
    fields = sorted((c.fa, c.fb, c.fz))
    for perm in itertools.permutations(range(3)):
        for tied in (0, 1):
            row = c.doc(("dry", perm, tied), wrap_words=False)
            for rank, stream in enumerate(perm):
                for f in fields[:rank + 1]:
                    c.put(row, MERGE_TERMS[stream], [3, 9] if tied else [3 + stream, 9 + stream], f)
            for i, t in enumerate(MERGE_TERMS[3:]):
                c.put(row, t, [20 + i], fields[i % 3])
            if row % 2 == 0:
                c.put(row, X, [900], fields[0])
            c.put(row, Y, [950], fields[0])
    return c


def part5_cases():
    def masks(c):
        # three different limits that all hold the lowest field: the stream that runs dry first stands there only, so every cell is
        # a match of every case and reaches the merge
        lo, mid, hi = sorted((c.fa, c.fb, c.fz))
        return ((1 << lo) | (1 << mid), (1 << lo) | (1 << hi), 1 << lo)

    dry = tuple(("dry", perm, tied) for perm in itertools.permutations(range(3)) for tied in (0, 1))
    out = both(5, "and a b c, three field limits", "merge", lambda m, c, p: AND(m, *[kw(m, MERGE_TERMS[i], p + i, masks(c)[i]) for i in range(3)]),
               "stream 0, 1, 2 runs dry first, the other two end in either order: phase 0 -> 1 -> 2 and the MergeHits3 field test, mrk_keval.h:163-185", matches=dry)
    out += both(5, "and a b, two field limits", "merge", lambda m, c, p: AND(m, *[kw(m, MERGE_TERMS[i], p + i, masks(c)[i]) for i in range(2)]), "k = 2: no quirk, mrk_keval.h:163",
                matches=dry)
    for k in (5, 6, 7, 8):
        out.append(Case(5, f"and of {k}, field limits", "merge", lambda m, c, k=k: AND(m, *[kw(m, MERGE_TERMS[i], i + 1, masks(c)[i % 3] if i < 4 else 0xFFFFFFFF) for i in range(k)]),
                        "k = 5..8: phase 2 from the start, every hit tested against its own keyword's fields, mrk_keval.h:163, 183-185", matches=dry))
    return out


# ------------------------------------------------------------------ 6. quorum order
Q_LAST = tuple(5 + 6 * j for j in range(8))  # keyword j's last doc: the rows at which an event reorders m_dChildren
Q_DOCS = Q_LAST[-1] + 4
QY = 8                                       # a keyword of every doc but each fifth, for AND / OR / MAYBE / BEFORE
Q_TERMS = 10


def quorum_corpus():
    """Keyword j stands in row r iff r <= Q_LAST[j] and (r % 6 != 1 and r % 6 != 2 or (r + j) % 4): dense lists that end at different rows (5, 11, ..: r % 6 = 5), and the rows
    last - 1, last and last + 1 of every keyword hold every list that still runs.  Hit counts 1..3."""
    H = EndHits()
    for r in range(Q_DOCS):
        for j in range(8):
            if j in quorum_present(r):
                H.add(j, r, [2 + 3 * j + i * 40 for i in range(1 + (r + 2 * j) % 3)], (r + j) % 2)
        if r % 5:
            H.add(QY, r, [100 + r % 7], r % 2)
    return H


def quorum_present(r):
    return [j for j in range(8) if r <= Q_LAST[j] and (r % 6 != 1 and r % 6 != 2 or (r + j) % 4)]


def quorum_trees(m):
    """-> [(name, tree)]: k = 3, 5, 8 at the root; k = 3, 5 below AND / OR / MAYBE / BEFORE; thresholds 1, 2, k - 1, k; one keyword absent"""
    out = []
    for k in (3, 5, 8):
        words = Q8[8 - k:] if k < 8 else Q8  # (the longest lists: the quorum still matches at the late events)
        for thr in sorted({1, 2, k - 1, k}):
            q = lambda p, words=words, thr=thr: QUORUM(m, thr, *[kw(m, t, p + i) for i, t in enumerate(words)])
            out.append((f"quorum {thr}/{k} at the root", q(1)))
            if k < 8:
                out.append((f"quorum {thr}/{k} and y", AND(m, q(1), kw(m, QY, k + 1))))
                out.append((f"y or quorum {thr}/{k}", OR(m, kw(m, QY, 1), q(2))))
                out.append((f"quorum {thr}/{k} maybe y", MAYBE(m, q(1), kw(m, QY, k + 1))))
                out.append((f"quorum {thr}/{k} before y", BEFORE(m, q(1), kw(m, QY, k + 1))))
        absent = lambda thr, words=words: QUORUM(m, thr, *[kw(m, -1 if i == 1 else t, 1 + i) for i, t in enumerate(words)])
        out.append((f"quorum 2/{k}, one keyword absent from the dictionary", absent(2)))
        if k < 8:
            out.append((f"quorum {k - 1}/{k}, one absent, and y", AND(m, absent(k - 1), kw(m, QY, k + 1))))
    return out


QUORUM_EDGE = "a row on either side of a keyword's last doc: the child order of the tfidf sum, mrk_keval.h:629-644 (generic), qr_row / qr_ord in mrk_scan_pk.hip"


def quorum_queries(m):
    qs = []
    for name, tree in quorum_trees(m):
        for rk in (m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25):
            for mm in (1000, 3):
                for fw in (None, [3, -1]):
                    qs.append((name, m.Query(tree, ranker=rk, max_matches=mm, field_weights=fw)))
    return qs


# ------------------------------------------------------------------ 7. list memory and the tf escape
TF_LADDER = range(1, 21)
TF_ESCAPE = (254, 255, 256, 300)


def memory_corpus():
    """Rows 0..19: a has 1..20 hits, b one, c two, in one field -- under '"x y" | "a b"' (x, y in no doc here) the evaluator takes tf(a),
    1, tf(a) + 1 and tf(a) + 1 hits in the chain's order, so tf = 16 and 17 put the first take on the lane's last slot and one past
    it, tf = 15 and 16 the second, tf = 7 and 8 the third (2 tf + 2 = 16, 18).  Rows 20..23: a has 254, 255, 256 and 300 hits, the
    first hundred in field 0, the rest in field 1; b and c once."""
    c = Corpus("memory")
    for tf in TF_LADDER:
        row = c.doc(("tf", tf), wrap_words=False)
        c.put(row, A, range(2, 2 + 2 * tf, 2), 0), c.put(row, B, [2 * tf + 1], 0), c.put(row, C, [1, 50], 0)
    for tf in TF_ESCAPE:
        row = c.doc(("tf", tf), wrap_words=False)
        c.put(row, A, range(2, 202, 2), 0), c.put(row, A, range(2, 2 + 2 * (tf - 100), 2), 1)
        c.put(row, B, [3], 0), c.put(row, B, [2 * (tf - 100) + 1], 1), c.put(row, C, [5], 1)
    return c


def part7_cases():
    out = []
    for name, mask in (("", 0xFFFFFFFF), (", a limited to field 1", 2)):
        out.append(Case(7, "phrase a b wrapped" + name, "memory", lambda m, c, mask=mask: wrap(m, lambda p: PHRASE(m, kw(m, A, p, mask), kw(m, B, p + 1))),
                        "a list that ends on the lane slice's last slot, the first that goes to the spill area: GenAlloc::take, mrk_keval.h:33-45; tf 254..300: "
                        "the 8-bit escape in gen_open, mrk_keval.h:64-69, under a term node :95-99"))
        out.append(Case(7, "and a b c wrapped" + name, "memory", lambda m, c, mask=mask: wrap(m, lambda p: AND(m, kw(m, A, p, mask), kw(m, B, p + 1), kw(m, C, p + 2))),
                        "tf around 255 under a MULTIAND: total and the n < total guard, mrk_keval.h:152-160, 185"))
        # (a field-limited keyword INSIDE a quorum is declined by both planners, so the limit stands on the trailing c: the quorum
        # never sees the escape keyword with dropped hits)
        out.append(Case(7, "quorum 2 of a b c before c" + name.replace(", a limited", ", the trailing c limited"), "memory",
                        lambda m, c, mask=mask: BEFORE(m, QUORUM(m, 2, kw(m, A, 1), kw(m, B, 2), kw(m, C, 3)), kw(m, C, 4, mask)),
                        "tf around 255 under a quorum: gen_term per keyword, mrk_keval.h:624-625, 645"))
    return out


# ------------------------------------------------------------------ 8. the ring NEAR and its probe launch
RING_TOTAL = 2300  # rows; fewer than 2,000 of them hold hits


def ring_corpus():
    """A root NEAR over three and more operands (a, b, c; up to eight keywords).  Row 0 completes two chains (TWO_ORDERS: the inserting doc of
    everything behind it, with nothing in front of it); chains complete in every arrival order of three operands; head shift (a a b c), tail replace
    (a b b c); a complete chain directly followed by a new one; inserting docs at r - 1 and r of dependent docs, more than 64 and
    more than 2048 rowids apart."""
    c = Corpus("ring")
    c.total_docs = RING_TOTAL

    def at(row, cell, hits):
        assert row >= c.n
        c.n = row
        r = c.doc(cell, wrap_words=False)
        for t, ps in hits.items():
            c.put(r, t, ps)

    at(0, "row0", dict(TWO_ORDERS))                         # the first inserting doc: nothing in front of it, its own later insert must not count
    at(1, "bca", {B: [10], C: [11], A: [12]})
    for i, perm in enumerate(itertools.permutations((A, B, C))):
        at(2 + i, ("order", perm), {t: [10 + j] for j, t in enumerate(perm)})
    at(10, "head_shift", {A: [10, 11], B: [12], C: [13]})
    at(11, "tail_replace", {A: [10], B: [11, 12], C: [13]})
    at(12, "two_chains", {A: [10, 13], B: [11, 14], C: [12, 15]})
    at(13, "broken", {A: [10], B: [11], C: [20]})           # no chain: nothing inserted behind the first
    at(14, "dependent", {C: [10], B: [11], A: [12]})        # r - 1 and r
    at(15, "dependent_next", {A: [10], C: [11], B: [12]})
    at(16, "two_orders", dict(TWO_ORDERS))                  # MATCHANY's weight of this doc depends on the docs in front: see TWO_ORDERS
    at(17, "head_shift_far", {A: [10, 12], B: [11], C: [14]})    # under NEAR/2 only the head's shift onto the second a keeps c within reach
    at(18, "tail_replace_far", {A: [10], B: [12, 14], C: [16]})  # ... only the tail's move onto the second b keeps c within reach
    for i, perm in enumerate(itertools.permutations((A, B, C))):  # a complete chain, the next one directly behind it in every order
        at(20 + i, ("after_chain", perm), {t: [10 + (A, B, C).index(t), 13 + perm.index(t)] for t in (A, B, C)})
    at(100, "far_64", {C: [10], A: [11], B: [12]})          # > 64 rows behind the last inserting doc
    for r in range(101, 2250):                              # a, b and c far apart: candidates that complete nothing and insert nothing;
        if r % 4:                                           # they make the doclists long enough for item_bytes = 4096 to cut them
            at(r, ("filler", r), {A: [10], B: [200], C: [400]})
    at(2250, "far_2048", {B: [10], A: [11], C: [12]})       # > 2048
    at(2251, "eight", {t: [10 + i] for i, t in enumerate((A, B, C, E, F, G, P[0], P[1]))})
    at(2252, "eight_rev", {t: [30 - i] for i, t in enumerate((A, B, C, E, F, G, P[0], P[1]))})
    at(2253, "two_orders_far", dict(TWO_ORDERS))            # ... > 2048 rows behind the doc that inserted query position 1
    return c


# The doc whose weight depends on the docs in front of it.  Under 'a NEAR/2 b NEAR/2 c' (query positions 1, 2, 3) "a b c" folds into a
# hit with query position min(m_uFirstQpos, 3) and "c b a" into one with min(m_uFirstQpos, 1); a chain's first hit never enters
# m_uFirstQpos, so alone the doc emits the query positions 2 and 1 and MATCHANY counts two matched words, while behind any doc
# that inserted an `a` (row 0 of the ring corpus) both hits carry 1 and MATCHANY counts one: its weight is 19 instead of 20 (three fields of weight 1).
TWO_ORDERS = ((A, (10, 22)), (B, (11, 21)), (C, (12, 20)))


def part8_cases():
    abc = lambda m, p0: [kw(m, t, p0 + i) for i, t in enumerate((A, B, C))]
    edge = "the ring form: arrival orders, head shift, tail replace, last_p reset behind a complete chain, mrk_keval.h:488-546; first_qpos from the probe launch :449, 542"
    arrival = tuple(("order", perm) for perm in itertools.permutations((A, B, C)))
    out = [Case(8, "near/2 a b c", "ring", lambda m, c: NEAR(m, 2, *abc(m, 1)), edge, matches=arrival + ("row0", "head_shift_far", "tail_replace_far", "two_chains", "far_2048"), misses=("broken",)),
           Case(8, "near/3 c b a", "ring", lambda m, c: NEAR(m, 3, *reversed(abc(m, 1))), edge),
           Case(8, "near/2 a b c at query positions 61..63", "ring", lambda m, c: NEAR(m, 2, *abc(m, 61)), "query positions up to 63: the near_tab's 64 columns, mrk_keval.h:466-469"),
           Case(8, "near/2 a b c a", "ring", lambda m, c: NEAR(m, 2, *(abc(m, 1) + [kw(m, A, 4)])), "four operands, one repeated: the dupe branch, mrk_keval.h:474-487"),
           Case(8, "near/4 (a b) c a", "ring", lambda m, c: NEAR(m, 4, PHRASE(m, kw(m, A, 2), kw(m, B, 3)), kw(m, C, 4), kw(m, A, 5)), "a phrase operand, query positions from 2: "
                "matchlen > 1 in the ring, mrk_keval.h:488, 538"),
           Case(8, "near/3 of eight", "ring", lambda m, c: NEAR(m, 3, *[kw(m, t, i + 1) for i, t in enumerate((A, B, C, E, F, G, P[0], P[1]))]), "eight operands: the ring at k = 8, mrk_keval.h:451-453")]
    return out


# ------------------------------------------------------------------ 9. BEFORE spans
def before_corpus(layout):
    c = Corpus("before", layout)
    for d in (-1, 0, 1):          # "a c" << b: b at pos + spanlen - 1 (rejected), + 0, + 1 (accepted)
        row = c.doc(("pk", d))
        c.put(row, A, [10]), c.put(row, C, [11]), c.put(row, B, [12 + d])
    for d in (-1, 0, 1):          # a << "b c": b at a's own position (the first child takes it), the next, one further
        row = c.doc(("kp", d))
        c.put(row, A, [10]), c.put(row, B, [11 + d]), c.put(row, C, [12 + d])
    for name, at in BEFORE3_DOCS.items():
        row = c.doc(("k3", name))
        for t, ps in zip((A, B, C), at):
            c.put(row, t, ps)
    for d in (0, 1):              # "a c" << b << c: the second c directly behind b, and on b's position
        row = c.doc(("pk3", d))
        c.put(row, A, [10]), c.put(row, C, [11, 14 - d]), c.put(row, B, [13])
    row = c.doc("first_childs_doc")  # b also in fa, twice: the doc's tfidf and fields are a's
    c.put(row, A, [10]), c.put(row, B, [11]), c.put(row, B, [3, 4], c.fa)
    return c


BEFORE3_DOCS = {"in_order": ([10], [11], [12]), "c_on_b": ([10], [11], [11]), "catch_up": ([10, 12], [11, 13], [14]), "late_start": ([10, 13], [11], [12, 15]),
                "all_one": ([10], [10], [10]), "c_first": ([11], [12], [10])}


def part9_cases():
    out = [Case(9, "(a c) before b", "before", lambda m, c: BEFORE(m, PHRASE(m, kw(m, A, 1), kw(m, C, 2)), kw(m, B, 3)),
                "the next child at pos + spanlen (accepted) and pos + spanlen - 1 (rejected), spanlen 2: mrk_keval.h:695-700", matches=(("pk", 0), ("pk", 1)), misses=(("pk", -1),)),
           Case(9, "a before (b c)", "before", lambda m, c: BEFORE(m, kw(m, A, 1), PHRASE(m, kw(m, B, 2), kw(m, C, 3))),
                "two children with a hit on one position: the first child takes it, mrk_keval.h:682-687"),
           Case(9, "(a c) before b before c", "before", lambda m, c: BEFORE(m, PHRASE(m, kw(m, A, 1), kw(m, C, 2)), kw(m, B, 3), kw(m, C, 4)), "k = 3 with a span: mrk_keval.h:698-705")]
    out += both(9, "a before b", "before", lambda m, c, p: BEFORE(m, kw(m, A, p), kw(m, B, p + 1)), "k = 2 over keywords; the doc's tfidf and fields are the first child's, mrk_keval.h:726-727")
    out += both(9, "a before b before c", "before", lambda m, c, p: BEFORE(m, kw(m, A, p), kw(m, B, p + 1), kw(m, C, p + 2)),
                "k = 3: the catch-up of the second tracker (len_r == len_l), mrk_keval.h:714-721")
    return out


# ------------------------------------------------------------------ 10. units
UNIT_DOTS = (None, 10, 12, 14, 16)


def units_corpus():
    c = Corpus("units")
    for dot in UNIT_DOTS:          # a at 10, b at 14; a dot on the lower hit, between, on the higher, behind both; none
        row = c.doc(("dot", dot))
        c.put(row, A, [10]), c.put(row, B, [14])
        if dot is not None:
            c.put(row, DOT, [dot])
    row = c.doc("second_unit")      # a . b, then a b together
    c.put(row, A, [10, 20]), c.put(row, B, [14, 22]), c.put(row, DOT, [12])
    row = c.doc("second_unit_closed")  # ... and a dot behind them
    c.put(row, A, [10, 20]), c.put(row, B, [14, 22]), c.put(row, DOT, [12, 25])
    row = c.doc("b_first")          # b a . : the pair's lower hit is the right argument's
    c.put(row, B, [10]), c.put(row, A, [12]), c.put(row, DOT, [13])
    for dot in (13, 15):            # a b c with the dot in front of c and behind it
        row = c.doc(("abc", dot))
        c.put(row, A, [10]), c.put(row, B, [12]), c.put(row, C, [14]), c.put(row, DOT, [dot])
    return c


def part10_cases():
    out = []
    for op in ("SENTENCE", "PARAGRAPH"):
        for name, unit in (("the dot", DOT), ("a unit keyword in no doc", NODOC), ("a unit keyword absent from the dictionary", -1)):
            out.append(Case(10, f"{op.lower()} a b, {name}", "units", lambda m, c, op=op, unit=unit: UNIT(m, getattr(m, "SPH_QUERY_" + op), unit, kw(m, A, 1), kw(m, B, 2)),
                            "a dot on the lower hit, between the pair, on the higher hit, behind both, none; a second unit behind a separated pair; aux == 0xFF: mrk_keval.h:270-302"))
        out.append(Case(10, f"{op.lower()} a b c", "units", lambda m, c, op=op: UNIT(m, getattr(m, "SPH_QUERY_" + op), DOT, kw(m, A, 1), kw(m, B, 2), kw(m, C, 3)),
                        "a unit node over a unit node, the dot in front of the third argument and behind it: mrk_keval.h:267, 278-284"))
    return out


# ------------------------------------------------------------------ the tables
LAYERED = {"ladders": ladders, "fields": fields_corpus, "flags": flags_corpus, "shared": shared_corpus, "before": before_corpus, "merge": merge_corpus}
PLAIN = {"memory": memory_corpus, "ring": ring_corpus, "units": units_corpus}
WIDE_TOO = ("ladders", "fields", "flags", "shared", "before")  # parts 1-4 and 9


def corpus_ids():
    """every (corpus, layout) the table cases run on"""
    out = []
    for key in LAYERED:
        out += [(key, lay) for lay in (LAYOUTS if key in WIDE_TOO else ("narrow",))]
    return out + [("units", "narrow")]


_corpora = {}


def corpus(key, layout="narrow"):
    if (key, layout) not in _corpora:
        _corpora[(key, layout)] = LAYERED[key](layout) if key in LAYERED else PLAIN[key]()
    return _corpora[(key, layout)]


def ranker_names(m, case):
    return case if case.rankers is None else dataclasses.replace(case, rankers=tuple(getattr(m, "SPH_RANK_" + r) if isinstance(r, str) else r for r in case.rankers))


def cases(m, key=None):
    out = part1_cases() + part2_cases() + part3_cases() + part4_cases() + part5_cases() + part7_cases() + part8_cases() + part9_cases() + part10_cases()
    return [ranker_names(m, x) for x in out if key is None or x.corpus == key]
