"""CPU: the state rankers' edge suite (rank_edges_common.py).  The model of the six Update / Finalize pairs is pinned to the reference's
recorded weights first; then it judges the oracle on the hand-made corpora, every named cell holds its hand-stated figure, every cell's
structure is read back from the bytes index_from_hits wrote, and a restatement of prox_bounds (csrc/mrk_kprune.h) is held against the
model: by hits it brackets the true rank part of every doc, by keywords only where the END flag belongs to the position."""
import json
import os
import subprocess

import numpy as np
import pytest

import rank_edges_common as C
from helpers import make_hits
from rank_edges_common import A, B
from test_gpu_parity import orc_index_of, to_orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def m():
    import manticoresearch_amd

    return manticoresearch_amd


def golden(name):
    g = json.load(open(os.path.join(HERE, "golden", name), encoding="utf-8"))
    for c in g["corpora"].values():  # (as test_oracle_golden.py expands the corpora the reference builds in a loop)
        if "docs_spec" in c:
            c["docs"] = [[f if isinstance(f, str) else "".join(t * n for t, n in f["runs"]) for f in run["fields"]] for run in c["docs_spec"] for _ in range(run["count"])]
    return g


def text_corpus(orc, docs, min_word_len):
    """-> (oracle index, vocabulary, docs_hits, n_fields) of a text corpus"""
    W, R, Hh, vocab = make_hits(docs, min_word_len)
    nf = max(len(d) for d in docs)
    oi = orc.build_index(W, R, Hh, total_docs=len(docs), n_fields=nf, n_terms=len(vocab))
    hits = [{} for _ in docs]
    for w, r, hp in zip(W, R, Hh):
        hits[int(r)].setdefault(int(w) - 1, []).append(int(hp))
    return oi, vocab, hits, nf


def bm25_parts(orc, oi, oroot, docs_hits, kws, n_fields, field_weights):
    """the BM25 part of every match, as rank_edges_common's doc states it: the oracle under SPH_RANK_BM25 minus 1000 x the matched fields' weights"""
    r = orc.search(oi, oroot, ranker=orc.RANK_BM25, max_matches=max(len(docs_hits), 1), field_weights=field_weights)
    assert r.total_found == len(r.rowid)
    w = C.bound_weights(field_weights, n_fields)
    return {int(row): int(wt) - 1000 * C.stream_fields_weight(docs_hits[int(row)], kws, w) for row, wt in zip(r.rowid, r.weight)}


# --------------------------------------------------------------------------- 1. the model on the reference's recorded weights
def flat_golden_cases():
    out = []
    g = golden("reference_vectors.json")
    for c in g["cases"]:
        q = c["query"]
        if c["corpus"] in ("test_037", "test_037_test2", "test_019_fld", "test_322") and c["ranker"] in ("proximity_bm25", "sph04", "wordcount", "fieldmask", "matchany") and \
                q.get("op") in ("and", "or") and all("word" in k and not k.get("tp") for k in q["kids"]) and ("expect" in c or "expect_weights" in c):
            out.append((c, g["corpora"][c["corpus"]]))
    g = golden("sorted_vectors.json")
    for c in g["cases"]:
        if c["name"].startswith("016 any") and not c["filters"]:
            out.append((c, g["corpora"][c["corpus"]]))
    return out


def test_the_model_gives_the_recorded_weights_of_flat_queries(orc, m):
    seen = set()
    for case, corpus in flat_golden_cases():
        oi, vocab, hits, nf = text_corpus(orc, corpus["docs"], corpus["min_word_len"])
        q = case["query"]
        kws = [(vocab[k["word"]], k["pos"], k["mask"]) for k in q["kids"]]
        match_all = q["op"] == "and"  # ('"test it"/1' is the OR of its words)
        ranker = getattr(m, "SPH_RANK_" + case["ranker"].upper())
        fw = case.get("field_weights")
        oroot = orc.op(orc.OP_AND if match_all else orc.OP_OR, *[orc.term(t, p, field_mask=mk) for t, p, mk in kws])
        bm = bm25_parts(orc, oi, oroot, hits, kws, nf, fw) if C.uses_bm25(m, ranker) else None
        got, _ = C.model_flat(m, ranker, kws, match_all, hits, nf, fw, case.get("index_weight", 1), bm)
        ids = corpus["ids"]
        if "expect_weights" in case:
            assert {str(ids[r]): w for r, (_, w) in got.items()} == case["expect_weights"], case["name"]
        elif case.get("unordered"):
            assert sorted((ids[r], w) for r, (_, w) in got.items()) == sorted(map(tuple, case["expect"])), case["name"]
        else:
            rows, wts = C.top_k(got, 1000)
            assert [(ids[int(r)], int(w)) for r, w in zip(rows, wts)] == [tuple(x) for x in case["expect"]], case["name"]
        seen.add((case["corpus"], case["ranker"]))
    assert {("test_322", "proximity_bm25"), ("test_322", "wordcount"), ("test_037_test2", "sph04"), ("test_019_fld", "fieldmask"), ("test_016", "matchany")} <= seen, seen


def test_the_model_gives_the_recorded_weights_of_the_folded_phrase(orc, m):
    """test_037's phrase cases: the two occurrences of the two-word phrase in doc 1 reach the ranker as two hits of weight 2 and spanlen 2 on the first word's
    position (the folding is written out by hand here: the model knows none).  Recorded: proximity_bm25 2800, wordcount 2."""
    g = golden("reference_vectors.json")
    corpus = g["corpora"]["test_037"]
    oi, vocab, hits, nf = text_corpus(orc, corpus["docs"], corpus["min_word_len"])
    want = {c["ranker"]: c["expect"] for c in g["cases"] if c["name"].startswith("037 phrase")}
    first, second = (vocab[k["word"]] for k in next(c for c in g["cases"] if c["name"] == "037 phrase proximity_bm25")["query"]["kids"])
    starts = [hp for hp in hits[0][first] if (hp & ~C.END) + 1 in {x & ~C.END for x in hits[0][second]}]
    assert [C.pos_of(x) for x in starts] == [1, 7]
    bm25 = want["bm25"][0][1] - 1000 * 1  # (one matched field of weight 1)
    st, _ = C.state_of(m, m.SPH_RANK_PROXIMITY_BM25, nf, None, False, 2, 2)
    for hp in starts:
        st.update(hp, 1, weight=2, spanlen=2)
    assert st.finalize(bm25)[1] == want["proximity_bm25"][0][1] == 2800
    st, _ = C.state_of(m, m.SPH_RANK_WORDCOUNT, nf, None, False, 2, 2)
    for hp in starts:
        st.update(hp, 1, weight=2, spanlen=2)
    assert st.finalize()[1] == want["wordcount"][0][1] == 2


# --------------------------------------------------------------------------- 2. the model judges the oracle
_bm = {}


def bm25_of(orc, m, name, shape, wname):
    if (name, shape, wname) not in _bm:
        hi, docs, _ = C.segment(name)
        root = C.shapes(m, name)[shape][0]
        fw = C.weight_sets(name)[wname]
        q = m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=1000, field_weights=fw)
        r = to_orc(orc, q).run(orc_index_of(orc, hi))
        w = C.bound_weights(fw, hi.n_fields)
        kws = C.keywords_of(root)
        _bm[(name, shape, wname)] = {int(row): int(wt) - 1000 * C.stream_fields_weight(docs[int(row)], kws, w) for row, wt in zip(r.rowid, r.weight)}
    return _bm[(name, shape, wname)]


@pytest.mark.parametrize("name", C.SEGMENT_IDS)
def test_oracle_equals_model_on_every_flat_query(orc, m, name):
    hi, docs, names = C.segment(name)
    oi = orc_index_of(orc, hi)
    fam = C.ranker_family(m)
    n_checked, longest, stale = 0, 0, 0
    for route, qs in C.queries(m, name, index_weights=(1, 3)).items():
        for shape, wname, q in qs:
            if q.ranker not in fam or not C.is_flat(m, q.root):
                continue
            bm = bm25_of(orc, m, name, shape, wname) if C.uses_bm25(m, q.ranker) else None
            per_doc, st = C.model_run(m, q, docs, hi.n_fields, bm)
            rows, wts = C.top_k(per_doc, q.max_matches)
            got = to_orc(orc, q).run(oi)
            assert got.total_found == len(per_doc), (shape, q.ranker, got.total_found, len(per_doc))
            assert np.array_equal(got.rowid, rows) and np.array_equal(got.weight, wts), (shape, wname, q.ranker, q.max_matches, got.rowid[:6], rows[:6], got.weight[:6], wts[:6])
            if C.uses_bm25(m, q.ranker) and q.index_weight == 1:  # the rank part on its own
                for r, wt in zip(got.rowid, got.weight):
                    assert int(wt) - bm[int(r)] == 1000 * per_doc[int(r)][0]
            longest = max(longest, getattr(st, "longest", 0))
            stale += getattr(st, "stale_min_exp_decided", 0) if shape == "a b@10" else 0
            n_checked += 1
    assert n_checked > 1000
    # a byte-wide LCS cannot wrap: the longest run any stream of these corpora reaches, before the byte mask, is the eight query positions
    assert longest == 8
    # the doc `afresh` took SPH04's `if` branch on the state the doc in front left, and the oracle (and the device, which starts afresh) agree all the same
    assert stale > 0


@pytest.mark.parametrize("name", C.SEGMENT_IDS)
def test_every_cell_holds_its_hand_stated_figure(orc, m, name):
    hi, docs, names = C.segment(name)
    oi = orc_index_of(orc, hi)
    shapes = C.shapes(m, name)
    fam = C.ranker_family(m)
    n = 0
    for cell in C.CELLS:
        row = names[cell.name]
        for (shape, family), figures in cell.expect.items():
            root = shapes[shape][0]
            for rk in [r for r, f in fam.items() if f == family and r not in shapes[shape][3]]:
                for wname, fw in C.weight_sets(name).items():
                    kws = [k.word.term_id for k in _leaves(root)]
                    want = C.cell_rank(m, name, cell, shape, rk, fw, len(set(kws)))
                    q = m.Query(root, ranker=rk, max_matches=1000, field_weights=fw)
                    if C.is_flat(m, root):
                        bm = bm25_of(orc, m, name, shape, wname) if C.uses_bm25(m, rk) else None
                        per_doc, _ = C.model_run(m, q, docs, hi.n_fields, bm)
                        assert per_doc[row][0] == want, (cell.name, shape, rk, wname, per_doc[row][0], want)
                    got = to_orc(orc, q).run(oi)
                    w = {int(r): int(x) for r, x in zip(got.rowid, got.weight)}
                    assert row in w, (cell.name, shape, "the cell is no match of the shape it is made for")
                    if not C.uses_bm25(m, rk):  # (the oracle's weight IS the rank part)
                        assert w[row] == C.i32(want), (cell.name, shape, rk, wname, w.get(row), want)
                    else:  # ... minus the BM25 part, here through the row's own statement of the matched fields: the roles of its figures
                        b = to_orc(orc, m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=1000, field_weights=fw)).run(oi)
                        bw = {int(r): int(x) for r, x in zip(b.rowid, b.weight)}
                        wts = C.bound_weights(fw, hi.n_fields)
                        bm = bw[row] - 1000 * sum(wts[C.roles_of(name)[role]] for role in figures)
                        assert w[row] - bm == 1000 * want, (cell.name, shape, rk, wname, w[row], bm, want)
                    n += 1
    assert n > 400
    # the same doc with and without the field limit answers differently
    for cell, limited, free in (("run4", "a bX c d", "abcd"), ("lim_second", "a bX", "ab"), ("lim_between", "a bXZ", "ab")):
        e = C.CELL_BY_NAME[cell].expect
        assert e[(limited, C.PROX)] != e[(free, C.PROX)]


def _leaves(n):
    return [n] if n.word is not None else [x for c in n.children for x in _leaves(c)]


def test_every_row_names_its_edge_and_its_line():
    import re

    for c in C.CELLS:
        assert len(c.edge) > 10 and c.hits, c.name
        assert re.search(r"(sphinxsearch\.cpp|searchnode\.cpp|mrk_k\w+\.h|[ (;,]):\d+", c.edge), (c.name, "names no source line")
        assert c.expect, (c.name, "states no figure")
    assert len({c.name for c in C.CELLS}) == len(C.CELLS)


# --------------------------------------------------------------------------- 3. the cells' structure, from the written hits
@pytest.mark.parametrize("name", C.SEGMENT_IDS)
def test_cells_stand_where_the_table_says(orc, m, name):
    hi, docs, names = C.segment(name)
    oi = orc_index_of(orc, hi)
    roles = C.roles_of(name)
    assert roles["0"] < roles["x"] < roles["y"] < roles["z"] < roles["top"] == hi.n_fields - 1
    written = [{} for _ in docs]
    for t in range(C.N_TERMS):
        rowid, fields, nhits, hp = oi.decode_doclist(t)
        for r, fl, nh, p in zip(rowid, fields, nhits, hp):
            hs = [int(x) for x in oi.decode_hits(int(p))] if not int(p) >> 63 or not hi.hit_format else [int(p) & 0xFFFFFFFF]
            assert len(hs) == int(nh) and int(fl) == sum(1 << f for f in {C.field_of(x) for x in hs})
            written[int(r)][t] = hs
    assert written == docs
    for cell in C.CELLS:  # the bytes hold the row's hits: field by role, position, flag
        got = sorted((t, C.field_of(x), C.pos_of(x), C.is_end(x)) for t, hs in written[names[cell.name]].items() for x in hs)
        assert got == sorted((t, roles[role], p, fl) for t, role, p, fl in cell.hits), cell.name

    def at(cell, t):
        return written[names[cell]][t]

    # shared positions are shared, and the flag is where the row says
    for cell in ("shared_pos_flag", "shared_kw_flag"):
        assert {C.pos_with_field(x) for x in at(cell, A)} & {C.pos_with_field(x) for x in at(cell, B)} == {(roles["x"] << 24) | 2}
    assert [C.is_end(x) for x in at("shared_pos_flag", A)] == [False, False] and [C.is_end(x) for x in at("shared_kw_flag", A)] == [False, True]
    s = C.stream(written[names["shared_kw_flag"]], [(A, 1, C.U32), (B, 2, C.U32)])
    assert [(C.pos_of(x), qp) for x, qp in s] == [(1, 1), (2, 2), (2, 1), (3, 2)]  # b@2 in FRONT of a@2|END
    s = C.stream(written[names["shared_pos_flag"]], [(A, 1, C.U32), (B, 2, C.U32)])
    assert [(C.pos_of(x), qp) for x, qp in s] == [(1, 1), (2, 1), (2, 2), (3, 2)]
    assert at("head_shared", A) == at("head_shared", B) == [(roles["y"] << 24) | 1]
    assert at("min_exp", C.C)[0] & ~C.END == at("min_exp", B)[0] & ~C.END and C.is_end(at("min_exp", B)[0])
    assert at("head_top", B) == [(roles["top"] << 24) | 1] and at("head_0", A) == [1]
    assert names["afresh"] == names["afresh_front"] + 1 and max(at("afresh_front", A) + at("afresh_front", B)) + 1 <= min(at("afresh", B)) == 9
    assert len(at("tf300", A)) == 300 and len({C.field_of(x) for x in at("tf300", A)}) == 3 and len(at("tf255", A)) == 255
    if hi.n_fields == 32:
        assert roles["top"] == 31 and {roles["x"], roles["y"], roles["z"]} <= {7, 8, 16, 30}
    # neighbouring rowids hold different cells, and a lone hit travels inline or through .spp as the segment says
    lone = sum(1 for d in docs for hs in d.values() if len(hs) == 1)
    assert lone > 40


def test_the_wide_segments_reach_all_four_words_of_the_field_bytes():
    fields = set()
    for name in C.SEGMENT_IDS:
        if next(s for s in C.SEGMENTS if s[0] == name)[1] == 32:
            fields |= set(C.roles_of(name).values())
    assert {f >> 3 for f in fields} == {0, 1, 2, 3} and {7, 8, 16, 31} <= fields


# --------------------------------------------------------------------------- 4. routes: the generic evaluator by the planner's word
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_generic_route_is_the_planners(m, tmp_path):
    """tests/cpp/gen_route.cpp asks mrk::plan_query for tree_flags & TF_GEN: the shapes of route G, and only they, go to the generic evaluator under the hit
    rankers.  (P, L, F and B are told apart by the match queue a pass feeds: the GPU test asserts mrk_batch_stats.mq_chunks on every batch.)"""
    from test_gen_edges_cpu import record

    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1"]
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "gen_route.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "gen_route")
    subprocess.check_call([HIPCC] + objs + ["-o", exe])
    lines, want = [], []
    for name in ("N-inline-128", "W-inline-128"):
        hi, _, _ = C.segment(name)
        d = hi.dict["docs"]
        lines.append("T %d %s" % (len(d), " ".join(str(int(x)) for x in d)))
        for shape, row in C.shapes(m, name).items():
            for rk in C.all_rankers(m):
                if rk not in row[3]:
                    lines.append(record(m, m.Query(row[0], ranker=rk), hi.n_fields))
                    want.append((shape, rk, "G" if C.route_of(m, row, rk) == "G" else "S"))
    path = tmp_path / "queries.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    got = out.stdout.strip().split("\n")
    assert len(got) == len(want)
    wrong = [(w, g) for w, g in zip(want, got) if g != w[2]]
    assert not wrong, wrong[:8]
    assert got.count("G") == 2 * 4 * 6


# --------------------------------------------------------------------------- 5. the weight bounds
TINY_WEIGHTS = ([1, 1], [2, 3], [0, 5], [-1, 2], [-3, -2], [3, -1])


def true_lcs(m, hits, n_fields=2, qpos_b=2):
    """per-field LCS of one doc under a@1 b@qpos_b (an OR: the keywords present emit), by the model"""
    st = C.Proximity(n_fields, [1] * C.MAX_FIELDS, dupes=False, use_bm25=False)
    for hp, qp in C.stream(hits, [(A, 1, C.U32), (B, qpos_b, C.U32)]):
        st.update(hp, qp)
    lcs = st.lcs[:n_fields]
    st.finalize()
    return lcs


@pytest.mark.parametrize("by_position", [True, False], ids=["flag-on-position", "flag-on-keyword"])
def test_bounds_hold_exhaustively_on_tiny_docs(m, by_position):
    """All docs of 2 keywords x 2 fields x positions 1..3: lo <= true rank part <= hi by hits under both flag conventions; by keywords under the position flag
    only -- the keyword flag BREAKS it, which is why the default is the bound by hits."""
    n, broken, attained_lo, attained_hi = 0, 0, 0, 0
    for hits in C.tiny_docs(by_position):
        lcs = true_lcs(m, hits)
        kf, ktf, emit = C.doc_bound_inputs(hits, (A, B))
        for fw in TINY_WEIGHTS:
            rank = sum(l * w for l, w in zip(lcs, fw))
            lo, hi = C.prox_bounds(kf, ktf, emit, fw, by_keywords=False)
            assert lo <= rank <= hi, (hits, fw, lo, rank, hi)
            attained_lo += rank == lo
            attained_hi += rank == hi
            lo, hi = C.prox_bounds(kf, ktf, emit, fw, by_keywords=True)
            if by_position:
                assert lo <= rank <= hi, (hits, fw, lo, rank, hi)
            else:
                broken += not lo <= rank <= hi
        n += 1
    assert n == 64 * 64 - 1 and attained_lo > 0 and attained_hi > 0
    assert (broken > 0) == (not by_position)


@pytest.mark.parametrize("by_position", [False, True], ids=["flag-on-keyword", "flag-on-position"])
def test_bounds_on_the_bounds_corpus_and_the_attaining_docs(m, by_position):
    docs, kinds = C.bounds_corpus(by_position)
    lcs_of = {}
    for kind, rows in kinds.items():
        for r in (rows[0], rows[-1]):
            lcs_of[(kind, r)] = true_lcs(m, docs[r], 8)
    for (kind, r), lcs in lcs_of.items():
        kf, ktf, emit = C.doc_bound_inputs(docs[r], (A, B))
        for fw in C.BOUNDS_FW.values():
            rank = sum(l * w for l, w in zip(lcs, fw))
            lo, hi = C.prox_bounds(kf, ktf, emit, fw, by_keywords=False)
            assert lo <= rank <= hi, (kind, fw)
            klo, khi = C.prox_bounds(kf, ktf, emit, fw, by_keywords=True)
            if by_position:
                assert klo <= rank <= khi, (kind, fw)
            w = fw[C.BOUNDS_FIELD]
            # the named attaining docs hit each end exactly
            if kind == "filler":
                assert rank == (lo if w > 0 else hi) == w and rank == (klo if w > 0 else khi)
            if kind == "adjacent":
                assert rank == (hi if w > 0 else lo) == 2 * w and rank == (khi if w > 0 else klo)
            if kind == "low":
                assert (lo, rank, hi) == ((1, 1, 2) if fw[0] > 0 else (2 * fw[0], fw[0], fw[0]))
            # ... and under a@1 b@11 the two change places: the fillers run to 2, the adjacent pair to 1
            gap = sum(l * x for l, x in zip(true_lcs(m, docs[r], 8, C.BOUNDS_GAP_QPOS), fw))
            assert lo <= gap <= hi and (not by_position or klo <= gap <= khi), (kind, fw)
            if kind == "filler":
                assert gap == (hi if w > 0 else lo) == 2 * w
            if kind == "adjacent":
                assert gap == (lo if w > 0 else hi) == w
            if kind == "shared3":
                assert lcs[C.BOUNDS_FIELD] == (1 if by_position else 3)
                if not by_position:  # inside the bound by hits, one past the bound by keywords
                    assert (3 * w > khi) if w > 0 else (3 * w < klo)
                    assert abs(hi - lo) == 3 * abs(w)
    # tf 255 and the escape: what the doclist says is min(hits, 255); one field's run can take tf - |F| + 1 of them
    kf, ktf, emit = C.doc_bound_inputs(docs[kinds["tf300"][0]], (A, B))
    assert ktf == [255, 1] and C.popcount(kf[0]) == 3 and C.prox_bounds(kf, ktf, emit, C.BOUNDS_FW["pos"], False)[1] == 253 * 5 + 3
    assert true_lcs(m, docs[kinds["tf300"][0]], 8)[:4] == [0, 1, 1, 1]
    # the low class lies wholly below the field-2 docs under "pos" and wholly above them under "neg": what the scan may drop
    ends = {}
    for kind in ("low", "filler"):
        kf, ktf, emit = C.doc_bound_inputs(docs[kinds[kind][0]], (A, B))
        ends[kind] = {name: C.prox_bounds(kf, ktf, emit, fw, False) for name, fw in C.BOUNDS_FW.items()}
    assert ends["low"]["pos"][1] < ends["filler"]["pos"][0] and ends["filler"]["neg"][1] < ends["low"]["neg"][0] and ends["low"]["neglead"][1] < ends["filler"]["neglead"][0]


def test_bounds_fit_switches_at_4210():
    assert C.bounds_fit([4210], 1) and not C.bounds_fit([4211], 1)
    assert C.bounds_fit([1000, -3210], 1) and not C.bounds_fit([1000, -3211], 1) and not C.bounds_fit([2105, 1], 2)


def test_the_bounds_corpus_goes_to_the_tree_kernel(m):
    """every keyword stands in every doc, so each is dense whatever the size and an AND / OR / MAYBE over them is the tree kernel's (bt_edges_common restates
    tree_on_bitmaps; test_gpu_bt_edges.py holds that restatement against n_items_bt exactly).  What sizes the corpus is the histogram: a wave recomputes its
    threshold after 256 lower bounds, and a work item's four waves share three windows here."""
    import bt_edges_common as bt

    hi, docs, kinds = C.bounds_segment(False)
    ndocs = [int(x) for x in hi.dict["docs"]]
    assert ndocs[A] == ndocs[B] == hi.total_docs == C.BOUNDS_DOCS > 2 * 2048 + 256
    kw = m.XQNode.keyword
    for root in (m.XQNode.AND(kw(A, 1), kw(B, 2)), m.XQNode(m.SPH_QUERY_OR, [kw(A, 1), kw(B, 2)]), m.XQNode(m.SPH_QUERY_MAYBE, [kw(A, 1), kw(B, 2)])):
        for rk in (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_PROXIMITY):
            assert bt.on_tree_kernel(m, m.Query(root, ranker=rk), ndocs, hi.total_docs)
    assert not bt.on_tree_kernel(m, m.Query(m.XQNode.AND(kw(A, 1), kw(B, 2, 4)), ranker=m.SPH_RANK_PROXIMITY), ndocs, hi.total_docs)  # a field limit: the block scan
