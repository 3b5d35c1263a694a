"""CPU: the corpora, tables and witnesses of tests/gen_edges_common.py, which tests/test_gpu_gen_edges.py runs through the generic
per-doc evaluator (csrc/mrk_keval.h) and its specialised twins.  Conditions on the builders: every cell of every ladder exists and
stands where its name says, the sizes stay under the caps, a flagged hit is its keyword's last of the field.  The oracle gives the
hand-stated answers on the plain ladders of part 1.  route() -- which (tree, ranker) goes to the generic evaluator -- is held against
mrk::plan_query itself (tests/cpp/gen_route.cpp), so the GPU test's pure batches are pure by the planner's word."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import gen_edges_common as ge
from gen_edges_common import A, B, C, E, F, G, P
from test_gpu_batch_state import oracle_all
from test_gpu_parity import kw, orc_index_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def m():
    import manticoresearch_amd

    return manticoresearch_amd


def pos_of(c, row, term):
    """positions of a keyword in the chain's field fb"""
    return [p for f, p, _ in c.hits_of(row, term) if f == c.fb]


# ------------------------------------------------------------------ the builders
@pytest.mark.parametrize("layout", list(ge.LAYOUTS))
def test_ladder_cells_stand_where_the_table_says(layout):
    c = ge.corpus("ladders", layout)
    assert c.fb == {"narrow": 1, "wide17": 16, "wide32": 31}[layout] and c.fb == c.n_fields - (2 if layout == "narrow" else 1)
    n = 0
    for combo, span, D, behind, o in ge.ladder_cells():
        row = c.cells[("lad", combo, span, D, behind, o)]
        lt, rt = {"k": [A], "p": [A, C], "x": [E, F, G]}[combo[0]], {"k": [B], "p": [B, C], "x": [E, F, G]}[combo[1]]
        ls, rs = min(pos_of(c, row, lt[0])), min(pos_of(c, row, rt[0]))
        ll = max(pos_of(c, row, lt[-1])) - ls + 1 if combo[0] != "p" else 2
        lr = max(pos_of(c, row, rt[-1])) - rs + 1 if combo[1] != "p" else 2
        assert (ll, lr) == (ge.operand_len(combo[0], span), ge.operand_len(combo[1], span)), (combo, span)
        if behind:  # the second operand starts at first + matchlen + D - 2 .. + 1
            assert rs == ls + ll + D - 2 + o, (combo, span, D, o)
        else:       # ... and the first at second + matchlen + D - 2 .. + 1
            assert ls == rs + lr + D - 2 + o and rs > 0, (combo, span, D, o)
        n += 1
    assert n == (2 + 2 * len(ge.X_SPANS)) * 2 * 2 * 4 + 2 * 2 * 4  # 5 combos (two of them in three spans) x D x side x offset
    for g in (1, 2, 3, 4):
        row = c.cells[("abab", g)]
        assert pos_of(c, row, A) == [20, 20 + 2 * g] and pos_of(c, row, B) == [20 + g, 20 + 3 * g]
    for D in ge.DISTS:
        row = c.cells[("nn_same", D)]
        assert pos_of(c, row, A) == pos_of(c, row, B) == [20]
        for kept in (0, 1):  # qlen = 4: the last word arrives at hpf = 43
            row = c.cells[("px_drop", D, kept)]
            assert [pos_of(c, row, P[i]) for i in range(1, 5)] == [[40], [41], [42], [43]] and pos_of(c, row, P[0]) == [43 - 4 - D + kept]
    for n_keep, at in ge.PX_WEIGHT_DOCS.items():
        row = c.cells[("px_w", n_keep)]
        deltas = [pos_of(c, row, P[i])[0] - i for i in range(5)]
        runs = sum(k for k in (deltas.count(d) for d in set(deltas)) if k > 1)
        assert runs == n_keep and max(at) - min(at) < 4 + 3, (n_keep, deltas)  # all five inside qlen + dist of '~3'


@pytest.mark.parametrize("layout", list(ge.LAYOUTS))
def test_field_flag_shared_and_before_cells(layout):
    c = ge.corpus("fields", layout)
    fa, fb = c.fa, c.fb
    assert fb == fa + 1 < c.n_fields
    row = c.cells["end_next"]
    assert c.hits_of(row, A) == [(fa, 7, True)] and c.hits_of(row, B) == [(fb, 1, False)]
    row = c.cells["end_next_c"]
    assert c.hits_of(row, A) == [(fa, 6, False)] and c.hits_of(row, C) == [(fa, 7, True)] and c.hits_of(row, B) == [(fb, 1, False)]
    for d in (0, 1):
        row = c.cells[("same_pos", d)]
        assert c.hits_of(row, A) == [(fa, 5, False)] and c.hits_of(row, B) == [(fb, 5 + d, False)]
    row = c.cells["maxpos"]
    assert c.hits_of(row, B) == c.hits_of(row, C) == [(fb, (1 << 23) - 1, False)] and c.hits_of(row, A) == [(fb, (1 << 23) - 2, False)]
    assert c.hits_of(c.cells["maxpos_end"], B) == [(fb, (1 << 23) - 1, True)]
    row = c.cells["bf_split"]
    assert {f for f, _, _ in c.hits_of(row, A)} == {fa} and {f for f, _, _ in c.hits_of(row, B)} == {fb}
    row = c.cells["bf_started"]
    assert c.hits_of(row, A) == [(fa, 3, False), (fb, 2, False)] and c.hits_of(row, B) == [(fb, 4, False)]
    for name, f in (("fa", fa), ("fb", fb)):
        row = c.cells[("cut_mid", name)]
        assert [c.hits_of(row, t) for t in (A, C, B)] == [[(f, 5, False)], [(f, 6, False)], [(f, 7, False)]]
    assert c.hits_of(c.cells["both_fields"], A)[0][0] == fa

    c = ge.corpus("flags", layout)
    for which in (None, 0, 1, 2):
        row = c.cells[("flag", which)]
        assert [c.hits_of(row, t) for t in (A, C, B)] == [[(c.fb, 5 + i, which == i)] for i in range(3)]
    for flagged in (0, 1):
        row = c.cells[("unit_flag", flagged)]
        assert c.hits_of(row, A) == [(c.fb, 5, bool(flagged))] and c.hits_of(row, ge.DOT) == [(c.fb, 6, False)] and c.hits_of(row, B) == [(c.fb, 7, False)]
    assert c.hits_of(c.cells["sph04_exact"], B) == [(c.fb, 2, True)] and c.hits_of(c.cells["sph04_exact"], A) == [(c.fb, 1, False)]

    c = ge.corpus("shared", layout)
    for d in (0, 1, 2, 3):
        row = c.cells[("ab", d)]
        assert pos_of(c, row, A) == [10] and pos_of(c, row, B) == [10 + d]
    assert c.hits_of(c.cells["ab_end"], A) == [(c.fb, 10, True)] and c.hits_of(c.cells["ab_end"], B) == [(c.fb, 10, False)]
    for pre in (0, 1):
        row = c.cells[("rollback", pre)]
        assert pos_of(c, row, A) == ([8, 10] if pre else [10]) and pos_of(c, row, C) == [11]
    for at in ge.AA_DOCS:
        assert pos_of(c, c.cells[("aa", at)], A) == list(at)
    for name, at in ge.AND5_DOCS.items():
        assert [pos_of(c, c.cells[("and5", name)], P[i]) for i in range(5)] == [[p] for p in at]
    assert len(set(ge.AND5_DOCS["all_one"])) == 1
    row = c.cells["q_flag_first"]
    assert [c.hits_of(row, P[i]) for i in range(3)] == [[(c.fb, 10, True)], [(c.fb, 11, False)], [(c.fb, 12, False)]]
    row = c.cells["q_tie"]
    assert c.hits_of(row, P[0]) == [(c.fb, 10, True)] and c.hits_of(row, P[1]) == [(c.fb, 10, False)]

    c = ge.corpus("before", layout)
    for d in (-1, 0, 1):
        row = c.cells[("pk", d)]  # "a c" at 10, spanlen 2: b at pos + spanlen + d
        assert pos_of(c, row, A) == [10] and pos_of(c, row, C) == [11] and pos_of(c, row, B) == [10 + 2 + d]
        row = c.cells[("kp", d)]
        assert pos_of(c, row, A) == [10] and pos_of(c, row, B) == [10 + 1 + d] and pos_of(c, row, C) == [10 + 2 + d]
    for d in (0, 1):
        row = c.cells[("pk3", d)]
        assert pos_of(c, row, A) == [10] and pos_of(c, row, C) == [11, 14 - d] and pos_of(c, row, B) == [13]
    for name, at in ge.BEFORE3_DOCS.items():
        assert [pos_of(c, c.cells[("k3", name)], t) for t in (A, B, C)] == [list(x) for x in at]
    row = c.cells["first_childs_doc"]
    assert {f for f, _, _ in c.hits_of(row, A)} == {c.fb} and {f for f, _, _ in c.hits_of(row, B)} == {c.fa, c.fb}


def test_merge_quorum_memory_ring_and_unit_cells():
    for layout in ("narrow",):
        c = ge.corpus("merge", layout)
        fields = sorted((c.fa, c.fb, c.fz))
        for perm in itertools.permutations(range(3)):
            for tied in (0, 1):
                row = c.cells[("dry", perm, tied)]
                last = [max(c.hits_of(row, ge.MERGE_TERMS[s]))[0] for s in range(3)]  # the field of each stream's last hit
                assert [last[s] for s in perm] == fields, (perm, last)  # perm[0] runs dry first, perm[2] last
                assert all(len(c.hits_of(row, t)) == 1 for t in ge.MERGE_TERMS[3:])
    # part 6, read from the hits quorum_corpus() wrote: every keyword's list ends at its row, every event has docs on both of its
    # sides, and around every event the thresholds asked (1, 2, k - 1, k of the k longest lists) are met by some row
    H = ge.quorum_corpus()
    held = {}
    for t, r, _ in H.hits:
        if t - 1 < 8:
            held.setdefault(r, set()).add(t - 1)
    assert len(set(ge.Q_LAST)) == 8
    for j, last in enumerate(ge.Q_LAST):
        assert max(r for r in held if j in held[r]) == last and j not in held.get(last + 1, ())
        assert last - 1 in held and j in held[last] and last + 1 < ge.Q_DOCS, (j, last)  # docs at last - 1, last, last + 1
        assert any(j in held[r] for r in range(last)) and (j == 7 or held[last + 1])  # (behind the last list's end the docs hold y only)
    for k in (3, 5, 8):
        words = set(ge.Q8[8 - k:])
        for e, last in enumerate(ge.Q_LAST[:-1]):  # (behind the last keyword's end nothing is left)
            alive = len([j for j in words if ge.Q_LAST[j] > last])
            for thr in sorted({1, 2, k - 1, k}):
                near = [r for r in (last - 1, last, last + 1) if len(held[r] & words) >= thr]
                assert near or thr > alive + 1, (k, thr, last)  # met next to the event while enough lists are still running
        assert any(len(held[r] & words) == k for r in held)
    c = ge.corpus("memory")
    for tf in list(ge.TF_LADDER) + list(ge.TF_ESCAPE):
        row = c.cells[("tf", tf)]
        assert len(c.hits_of(row, A)) == tf
        if tf >= 254:
            assert sum(1 for f, _, _ in c.hits_of(row, A) if f == 0) == 100 and {f for f, _, _ in c.hits_of(row, B)} == {0, 1}
    assert {15, 16, 17, 7, 8} <= set(ge.TF_LADDER) and 2 * 7 + 2 == 16  # the first, second and third take on slot 16 and past it
    c = ge.corpus("ring")
    assert c.cells["row0"] == 0 and [c.hits_of(0, t) for t, _ in ge.TWO_ORDERS] == [[(c.fb, p, False) for p in ps] for _, ps in ge.TWO_ORDERS]
    assert c.cells["dependent_next"] == c.cells["dependent"] + 1
    assert c.cells["far_64"] - c.cells["dependent_next"] > 64 and c.cells["far_2048"] - c.cells["far_64"] > 2048 and c.total_docs > c.cells["eight_rev"]
    assert len({tuple(p) for k, p in ((k, k[1]) for k in c.cells if isinstance(k, tuple) and k[0] == "order")}) == 6
    assert pos_of(c, c.cells["head_shift"], A) == [10, 11] and pos_of(c, c.cells["tail_replace"], B) == [11, 12] and pos_of(c, c.cells["two_chains"], A) == [10, 13]
    assert pos_of(c, c.cells["head_shift_far"], A) == [10, 12] and pos_of(c, c.cells["head_shift_far"], B) == [11] and pos_of(c, c.cells["tail_replace_far"], B) == [12, 14]
    for perm in itertools.permutations((A, B, C)):
        row = c.cells[("after_chain", perm)]
        assert [pos_of(c, row, t)[0] for t in (A, B, C)] == [10, 11, 12] and [pos_of(c, row, t)[1] for t in perm] == [13, 14, 15]
    c = ge.corpus("units")
    for dot in ge.UNIT_DOTS:
        row = c.cells[("dot", dot)]
        assert pos_of(c, row, A) == [10] and pos_of(c, row, B) == [14] and pos_of(c, row, ge.DOT) == ([] if dot is None else [dot])
    assert pos_of(c, c.cells["second_unit"], ge.DOT) == [12] and pos_of(c, c.cells["second_unit"], A) == [10, 20]
    assert not any(t == ge.NODOC + 1 for cc in (ge.corpus("units"),) for t, _, _ in cc.H.hits)


def test_sizes_stay_under_the_caps(m):
    ids = ge.corpus_ids() + [("memory", "narrow"), ("ring", "narrow")]
    for key, layout in ids:
        c = ge.corpus(key, layout)
        assert len(c.cells) == c.n or key == "ring"
        assert len(c.cells) < ge.MAX_DOCS and len(c.H) < ge.MAX_HITS, (key, len(c.cells), len(c.H))
        for block, fmt in ge.FORMS:
            hi = c.index(m, block, fmt)
            assert hi.n_fields == c.n_fields and hi.total_docs == (c.total_docs or c.n)
        batches, n = ge.batches_of(m, ge.cases(m, key), c)
        assert n == sum(len(ge.queries_of(m, case, c)) for case in ge.cases(m, key)) and all(0 < len(qs) <= ge.MAX_BATCH for _, qs in batches)
    H = ge.quorum_corpus()
    assert ge.Q_DOCS < ge.MAX_DOCS and len(H) < ge.MAX_HITS and len(ge.quorum_queries(m)) > 0
    parts = {case.part for case in ge.cases(m)}
    assert parts == {1, 2, 3, 4, 5, 7, 8, 9, 10} and all(case.edge and "mrk_keval.h" in case.edge for case in ge.cases(m))  # (part 6: quorum_queries)


# ------------------------------------------------------------------ the oracle on the plain ladders
@pytest.mark.parametrize("layout", list(ge.LAYOUTS))
@pytest.mark.parametrize("D", ge.DISTS)
def test_oracle_gives_the_hand_stated_answers(orc, m, layout, D):
    """a NEAR/D b matches iff the operands are at most D apart, in both orders; "a c" NEAR/D b iff b starts at most D behind the
    phrase's end; a NOTNEAR/D b keeps the doc iff b comes before a or b - a > D; "a c" NOTNEAR/D b iff b is more than D behind c."""
    c = ge.corpus("ladders", layout)
    hi = c.index(m, 128, 1)   # (held while its oracle index is in use: the oracle borrows its memory)
    oi = orc_index_of(orc, hi)
    N = m.SPH_RANK_NONE
    qs = [m.Query(ge.pair_node(m, "near", D, "kk", 1), ranker=N), m.Query(ge.pair_node(m, "near", D, "pk", 1), ranker=N),
          m.Query(ge.pair_node(m, "notnear", D, "kk", 1), ranker=N), m.Query(ge.pair_node(m, "notnear", D, "pk", 1), ranker=N)]
    got = [set(r.rowid.tolist()) for r in oracle_all(orc, hi, qs, oi)]
    for combo, near, notnear in (("kk", got[0], got[2]), ("pk", got[1], got[3])):
        ll = ge.operand_len(combo[0], 0)
        for D2 in ge.DISTS:
            for behind in (True, False):
                for o in ge.OFFSETS:
                    row = c.cells[("lad", combo, 0, D2, behind, o)]
                    ls, rs = ge.ladder_starts(combo, 0, D2, behind, o)
                    gap = rs - (ls + ll - 1) if behind else ls - rs  # from the end of the one in front to the start of the one behind
                    if gap < 1:  # (the second operand ON the first one's last position: no hand-stated answer, the oracle's stands)
                        continue
                    assert (row in near) == (gap <= D), (combo, D, D2, behind, o, gap)
                    assert (row in notnear) == (not behind or gap > D), (combo, D, D2, behind, o, gap)
    del oi, hi


def test_every_case_matches_some_doc_and_not_every_doc(orc, m):
    """no row of the tables is vacuous: under SPH_RANK_NONE its tree matches at least one doc of its corpus"""
    for key, layout in ge.corpus_ids() + [("memory", "narrow"), ("ring", "narrow")]:
        c = ge.corpus(key, layout)
        hi = c.index(m, 128, 1)  # (held while its oracle index is in use)
        oi = orc_index_of(orc, hi)
        cases = ge.cases(m, key)
        res = oracle_all(orc, hi, [m.Query(case.make(m, c), ranker=m.SPH_RANK_NONE) for case in cases], oi)
        empty = [case.name for case, r in zip(cases, res) if r.total_found == 0]
        assert not empty, (key, layout, empty)
        assert key == "merge" or any(r.total_found < len(c.cells) for r in res)  # (merge: every cell is a match of every case, below)
        n_named = 0
        for case, r in zip(cases, res):  # the cells a row names: answered, or left out, as stated by hand
            rows = set(r.rowid.tolist())
            assert all(c.cells[cell] in rows for cell in case.matches), (key, layout, case.name, [cell for cell in case.matches if c.cells[cell] not in rows])
            assert not any(c.cells[cell] in rows for cell in case.misses), (key, layout, case.name, [cell for cell in case.misses if c.cells[cell] in rows])
            n_named += len(case.matches) + len(case.misses)
        assert n_named or key in ("ladders", "shared", "units", "memory")  # (ladders: test_oracle_gives_the_hand_stated_answers)
        if key == "merge":  # part 5: every order of running dry is answered by every case, so it reaches the merge
            assert all(len(case.matches) == 12 and r.total_found == 12 for case, r in zip(cases, res))
        del oi, hi


# ------------------------------------------------------------------ route() against the planner
def record(m, q, n_fields):
    from manticoresearch_amd.api import _CQueries

    cq = _CQueries([q])
    a = cq.arr[0]
    out = ["Q", n_fields, q.ranker, a.n_nodes]
    n_ch = 0
    for i in range(a.n_nodes):
        n = a.nodes[i]
        out += [n.op, n.term_id, n.atom_pos, n.field_mask, n.opt, n.term_pos, n.field_max_pos, n.n_children, n.first_child]
        n_ch = max(n_ch, n.first_child + n.n_children)
    return "Q " + " ".join(str(int(x)) for x in out[1:] + [n_ch] + [a.children[i] for i in range(n_ch)])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_route_is_the_planners(m, tmp_path):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1"]
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "gen_route.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "gen_route")
    subprocess.check_call([HIPCC] + objs + ["-o", exe])
    lines, want, names = [], [], []

    def dictionary(hi):
        d = hi.dict["docs"]
        lines.append("T %d %s" % (len(d), " ".join(str(int(x)) for x in d)))

    for key, layout in ge.corpus_ids() + [("memory", "narrow"), ("ring", "narrow")]:
        c = ge.corpus(key, layout)
        dictionary(c.index(m, 128, 1))
        for case in ge.cases(m, key):
            for rk in case.rankers or ge.all_rankers(m):
                q = m.Query(case.make(m, c), ranker=rk)
                lines.append(record(m, q, c.n_fields))
                want.append(ge.route(m, q.root, rk))
                names.append((key, layout, case.name, rk))
    dictionary(ge.quorum_corpus().index(m, ge.Q_TERMS, ge.Q_DOCS))
    seen = set()
    for name, q in ge.quorum_queries(m):
        if (name, q.ranker) not in seen:
            seen.add((name, q.ranker))
            lines.append(record(m, q, 2))
            want.append(ge.route(m, q.root, q.ranker))
            names.append(("quorum", "narrow", name, q.ranker))
    path = tmp_path / "queries.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    got = out.stdout.strip().split("\n")
    assert len(got) == len(want)
    declined = [(n, g) for n, g in zip(names, got) if g.startswith("D")]
    assert not declined, declined[:5]  # no query of the tables may come back declined
    wrong = [(n, g, w) for n, g, w in zip(names, got, want) if g[0] != w]
    assert not wrong, (len(wrong), wrong[:8])
    ring = [g for n, g in zip(names, got) if n[0] == "ring"]
    assert ring and all(g == "GN" for g in ring)  # part 8: every case takes the probe launch
    assert got.count("S") > 100 and sum(g[0] == "G" for g in got) > 300


# ------------------------------------------------------------------ part 8: a weight that depends on the docs in front
def test_a_ring_near_weight_depends_on_the_docs_in_front(orc, m):
    """ge.TWO_ORDERS alone, behind an inserting doc, and in the ring corpus (directly behind one, and > 2048 rows behind): MATCHANY's
    weight is 20 alone and 19 behind a doc that inserted query position 1.  The device gets that from the probe launch's near_tab
    and the strict tab[v] < rowid only, so test_gpu_gen_edges.py::test_ring_near fails if either is broken."""
    q = m.Query(ge.NEAR(m, 2, kw(m, A, 1), kw(m, B, 2), kw(m, C, 3)), ranker=m.SPH_RANK_MATCHANY)

    def weights(docs):
        H = ge.EndHits()
        for r, d in enumerate(docs):
            for t, ps in d.items():
                H.add(t, r, ps, 1)
        hi = H.index(m, ge.N_TERMS, len(docs), 3)  # (three fields, the chain in field 1, as in the ring corpus; held while its oracle index is in use)
        oi = orc_index_of(orc, hi)
        r = oracle_all(orc, hi, [q], oi)[0]
        return dict(zip(r.rowid.tolist(), r.weight.tolist()))

    dep, ins = dict(ge.TWO_ORDERS), {B: [10], C: [11], A: [12]}
    # (popcount of the matched query positions + (lcs - 1) * sum of the field weights * query words) * field weight: 2 + 2 * 3 * 3 alone
    assert weights([dep]) == {0: 20}
    assert weights([ins, dep])[1] == 19 and weights([dep, ins])[0] == 20  # only the docs IN FRONT count
    c = ge.corpus("ring")
    hi = c.index(m, 128, 1)
    oi = orc_index_of(orc, hi)
    r = oracle_all(orc, hi, [q], oi)[0]
    w = dict(zip(r.rowid.tolist(), r.weight.tolist()))
    assert w[c.cells["row0"]] == 20 and w[c.cells["two_orders"]] == 19 and w[c.cells["two_orders_far"]] == 19  # (row 0: strictly in front)
    assert c.cells["two_orders_far"] - c.cells["far_64"] > 2048
    del oi, hi


# ------------------------------------------------------------------ part 6: a report
def test_quorum_keyword_order_report(orc, m, capsys):
    """How many weights change when a quorum's keywords are listed in another order (a report, not a condition): the order of the
    tfidf sum shows in a weight only where the float sum rounds differently."""
    H = ge.quorum_corpus()
    hi = H.index(m, ge.Q_TERMS, ge.Q_DOCS)
    oi = orc_index_of(orc, hi)
    changed = total = 0
    for k in (3, 5, 8):
        words = ge.Q8[8 - k:]
        for thr in (2, k - 1):
            a = m.Query(ge.QUORUM(m, thr, *[kw(m, t, 1 + i) for i, t in enumerate(words)]), ranker=m.SPH_RANK_BM25)
            b = m.Query(ge.QUORUM(m, thr, *[kw(m, t, 1 + i) for i, t in enumerate(reversed(words))]), ranker=m.SPH_RANK_BM25)
            ra, rb = oracle_all(orc, hi, [a, b], oi)
            wa, wb = dict(zip(ra.rowid.tolist(), ra.weight.tolist())), dict(zip(rb.rowid.tolist(), rb.weight.tolist()))
            assert wa.keys() == wb.keys() and len(wa) > 0
            total += len(wa)
            changed += sum(wa[r] != wb[r] for r in wa)
    with capsys.disabled():
        print(f"\nquorum keyword order: {changed} of {total} weights change when the keywords are listed in reverse")
    del oi, hi
