"""CPU: the sorted top-K selection's edge cases (csrc/mrk_sortsel.hip) before they reach a GPU.  Every case of
tests/test_gpu_sortsel_edges.py is shown to have the structure it names, read off the oracle's full match list and the attribute
columns: class sizes and their order, the class that holds rank K for each listed K, the exact doc counts of the list-length corpus.
The bin geometry the cases rest on is printed by a host-only program under AddressSanitizer + UBSan (tests/cpp/sortsel_geom.cpp: the
planner over a stand-in segment that holds these very rows, the probe keys through cand_bin) and asserted here."""
import os
import re
import subprocess

import numpy as np
import pytest

import manticoresearch_amd as m
import sortsel_edges_common as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def corpora(orc):
    return sc.Corpora(m, orc)


def classes(values):
    """[(value, rows)] ascending by value"""
    v, n = np.unique(values, return_counts=True)
    return [(int(a), int(b)) for a, b in zip(v, n)]


def rank_class(sizes, K):
    """(index, rows above it) of the class that holds rank K, the classes best first"""
    above = 0
    for i, n in enumerate(sizes):
        if above + n >= K:
            return i, above
        above += n
    raise AssertionError((sizes, K))


def col(rows, full, name):
    off, cnt, _ = sc.COLS[name]
    return sc.raw_of(rows, full.rowid, off, cnt)


def test_constants_are_the_headers():
    src = open(os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_dev.h")).read()
    assert "constexpr int WAVES = 4;" in src and "constexpr int WG = 64 * WAVES;" in src and sc.WG == 256
    assert "constexpr int KCAP = MRK_MAX_K;" in src and "constexpr int CAND = 2 * KCAP;" in src and "constexpr int NBINS = 1024;" in src
    assert re.search(r"#define MRK_MAX_K 1024\b", open(os.path.join(ROOT, "include", "mrk.h")).read())
    assert (sc.KCAP, sc.CAND, sc.NBINS) == (1024, 2048, 1024)
    assert sc.S_MATCHES == 4 * sc.CAND and sc.LADDER[2] > 3 * sc.CAND + sc.WG  # the buffer overfills several times; so does the largest class alone
    trigger = sc.CAND - sc.WG
    assert {trigger - 1, trigger, trigger + 1, sc.CAND - 1, sc.CAND, sc.CAND + 1, sc.WG - 1, sc.WG, sc.WG + 1, 1, 2 * sc.CAND + 1} == set(sc.LIST_COUNTS)


# ------------------------------------------------------------------ corpus S: the weight ladder
@pytest.mark.parametrize("placement", ["even", "high"])
@pytest.mark.parametrize("ranker", ["bm25", "proximity_bm25"])
def test_weight_ladder_has_its_classes(corpora, placement, ranker):
    name = ("S", placement)
    hi, oi, rows = corpora.get(*name)
    assert hi.total_docs == sc.S_DOCS and [int(d["docs"]) for d in hi.dict] == [sc.S_MATCHES] * 2
    rk = m.SPH_RANK_BM25 if ranker == "bm25" else m.SPH_RANK_PROXIMITY_BM25
    full = corpora.full(name, m.Query(sc.root_ab(m), ranker=rk))
    assert full.total_found == sc.S_MATCHES and np.array_equal(np.sort(full.rowid), np.arange(sc.S_MATCHES) * 4)
    cls = classes(full.weight)[::-1]  # best first: b's tf 3, 2, 1
    assert [n for _, n in cls] == list(sc.LADDER)
    by_row = np.zeros(sc.S_DOCS, np.int64)
    by_row[full.rowid] = full.weight
    w = by_row[::4]
    assert np.array_equal(np.searchsorted([c for c, _ in cls[::-1]], w) + 1, sc.ladder(placement))  # the heavier the class the larger b's tf
    if placement == "high":
        assert (w[-sc.LADDER[0]:] == cls[0][0]).all() and (w[:sc.LADDER[2]] == cls[2][0]).all()


def test_key_ladders_are_independent_of_the_weight_and_rank_k_lies_where_named(corpora):
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    full = corpora.full(name, m.Query(sc.root_ab(m), ranker=m.SPH_RANK_BM25))
    wcls = np.searchsorted(np.unique(full.weight), full.weight) + 1
    for p in sc.PLACEMENTS:
        key = col(rows, full, "lad_" + p)
        assert classes(key) == [(1, sc.LADDER[2]), (2, sc.LADDER[1]), (3, sc.LADDER[0])]
        order = np.argsort(full.rowid)
        k = key[order]
        if p == "low":
            assert (k[:300] == 3).all() and (k[300:800] == 2).all()
        if p == "high":
            assert (k[-300:] == 3).all() and (k[-800:-300] == 2).all()
        # every weight class inside the key class of 7392 rows, and inside the other two where the key is placed low or high
        tab = np.array([[int(((key == a) & (wcls == b)).sum()) for b in (1, 2, 3)] for a in (1, 2, 3)])
        assert (tab[0] > 0).all() and (p == "even" or (tab > 0).all()), (p, tab)
        assert not np.array_equal(key, wcls)
    # the class that holds rank K: descending 300 / 500 / 7392, ascending the class of 7392 leads
    want_desc = {1: (0, 0), 299: (0, 0), 300: (0, 0), 301: (1, 300), 799: (1, 300), 800: (1, 300), 801: (2, 800), 1000: (2, 800), 1024: (2, 800)}
    assert set(want_desc) == set(sc.LADDER_KS)
    for K in sc.LADDER_KS:
        assert rank_class(sc.LADDER, K) == want_desc[K] and rank_class(sc.LADDER[::-1], K) == (0, 0)
    assert sc.LADDER[2] > 4 * (sc.CAND - sc.WG)  # ascending, rank K lies inside a class more than four buffers long
    assert (col(rows, full, "const") == 42).all() and (rows[:, sc.CONST] == 42).all()


def test_case_queries_are_the_ones_named():
    q1 = sc.case1(m, m.SPH_RANK_BM25)
    assert len(q1) == 3 * 2 * 3 * len(sc.LADDER_KS) and {q.max_matches for q in q1} == set(sc.LADDER_KS) and {q.sort.then_weight for q in q1} == {0, 1, 2}
    q2 = sc.case2(m, m.SPH_RANK_BM25)
    assert {q.max_matches for q in q2} == {1, 2, 300, 301, 1024} and {q.sort.then_weight for q in q2} == {0, 1, 2}
    q3 = sc.case3(m)
    assert len(q3) == 5 * 2 * 3 and {(q.sort.bit_offset, q.sort.desc, q.max_matches) for q in q3} == {(sc.COLS[c][0], d, K) for c in sc.GEOMETRY_COLS for d in (True, False) for K in (1, 10, 1024)}
    assert {(q.sort.bit_offset, q.sort.bit_count) for q in sc.case4(m)} == {(sc.BITS_B * 32 + 31, 1), (sc.BITS_A * 32, 1), (sc.BITS_A * 32 + 1, 31), (sc.BITS_B * 32 + 27, 5)}
    q6 = sc.case6(m)
    i64 = [q for q in q6 if q.order.parts[0].kind == m.SORTKEY_INT64]
    assert {(q.order.parts[0].desc, q.order.then_weight, q.max_matches) for q in i64} == {(d, t, K) for d in (True, False) for t in (0, 1, 2) for K in (1, 911, 1024)}
    two = [q for q in q6 if len(q.order.parts) == 2]
    assert len(two) == 4 * len(sc.TWO_PARTS) and {(q.order.parts[0].desc, q.order.parts[1].desc) for q in two[:4]} == {(True, True), (False, False), (True, False), (False, True)}
    q7 = sc.case7(m)
    assert len(q7) == (3 + 4) * len(sc.WF_KS) and {q.order.weight_first for q in q7} == {1, 2} and all(q.order.then_weight == 0 for q in q7)
    seq, q10 = sc.case10(m)
    pairs = {(a, b) for a, b in zip(seq, seq[1:]) if a != b}
    assert pairs == {(a, b) for a in range(7) for b in range(7) if a != b} and len(q10) == len(seq)
    assert sc.S_BASES[0] + sc.S_DOCS == 2**32 and sc.S_BASES[1] < 2**31 - 4 * sc.CAND and sc.S_BASES[1] + sc.S_DOCS > 2**31 + 4 * sc.CAND


# ------------------------------------------------------------------ corpus S: the columns
def test_geometry_columns_hold_what_they_name(corpora):
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    full = corpora.full(name, m.Query(sc.root_ab(m), ranker=m.SPH_RANK_BM25))
    f32 = classes(col(rows, full, "full32"))
    assert [v for v, _ in f32] == sorted(int(v) for v in sc.full32_values()) and {n for _, n in f32} == {4}
    vals = {v for v, _ in f32}
    assert {0, 0xFFFFFFFF} <= vals and all((c << 22) - 1 in vals and (c << 22) in vals for c in range(1, 1024))
    assert int(rows[:, sc.FULL32].min()) == 0 and int(rows[:, sc.FULL32].max()) == 0xFFFFFFFF
    for c, span in (("span1023", 1023), ("span1024", 1024), ("span1025", 1025)):
        got = classes(col(rows, full, c))
        assert [v for v, _ in got] == list(range(sc.SPAN_LO, sc.SPAN_LO + span + 1))
        column = rows[:, sc.COLS[c][0] // 32]
        assert int(column.max()) - int(column.min()) == span
    band = classes(col(rows, full, "band"))
    assert [v for v, _ in band] == list(range(sc.BAND_LO, sc.BAND_LO + 1025)) and {n for _, n in band} == {7, 8}
    dead = rows[np.arange(sc.S_DOCS) % 4 != 0, sc.BAND]
    assert set(np.unique(dead).tolist()) == {0, 0xFFFFFFFF}
    # the class of rank K: 8 rows from the low end (every K), 7 rows for the eight highest values and 8 below them
    sizes_asc = [n for _, n in band]
    for K in (1, 10, 1024):
        assert sizes_asc[rank_class(sizes_asc, K)[0]] == 8
        assert sizes_asc[::-1][rank_class(sizes_asc[::-1], K)[0]] == (8 if K == 1024 else 7)
    # bit-fields: both one-bit columns split the matches into two classes longer than the buffer; the wide ones take many values
    for c in ("bit31", "bit0"):
        got = classes(col(rows, full, c))
        assert [v for v, _ in got] == [0, 1] and min(n for _, n in got) > sc.CAND
    assert len(classes(col(rows, full, "bits31at1"))) > 8000 and int(col(rows, full, "bits31at1").max()) >= 2**30
    five = classes(col(rows, full, "bits5at27"))
    assert [v for v, _ in five] == list(range(32)) and min(n for _, n in five) > 100
    assert [n for _, n in classes(col(rows, full, "cat4"))] == [sc.S_MATCHES // 4] * 4
    for c, span in (("r255", 255), ("r256", 256)):
        column = rows[:, sc.COLS[c][0] // 32]
        assert int(column.max()) - int(column.min()) == span and len(classes(col(rows, full, c))) == span + 1


def test_float_columns_put_rank_k_into_the_merged_zero_class(corpora):
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    full = corpora.full(name, m.Query(sc.root_ab(m), ranker=m.SPH_RANK_BM25))
    order = np.argsort(full.rowid)
    d = col(rows, full, "fltd")[order]
    a = col(rows, full, "flta")[order]
    assert np.array_equal(a, d ^ np.uint32(0x80000000))
    assert int((d == 0x80000000).sum()) == sc.ZEROS and int((d == 0).sum()) == sc.ZEROS
    zeros = d[(d << np.uint32(1)) == 0]
    assert (zeros[0::2] == 0x80000000).all() and (zeros[1::2] == 0).all()  # interleaved by rowid
    f = d.view(np.float32)
    assert not np.isnan(f).any() and int((f > 0).sum()) == sc.FLT_ABOVE and int((f < 0).sum()) == sc.S_MATCHES - sc.FLT_ABOVE - 2 * sc.ZEROS
    for e in sc.FLT_EDGES:
        assert int((d == e).sum()) == 2 and int((d == (e | 0x80000000)).sum()) == 2
    # rank K of FLTD descending and of FLTA ascending: 500 is the last row above the zeros, 501 .. 1024 lie in the zero class
    for q in sc.case5(m):
        off = q.sort.bit_offset
        if (off == sc.FLTD * 32) == q.sort.desc:
            r, w, key, total = corpora.want(name, q)
            in_zero = (int(key[-1]) << 1) & 0xFFFFFFFF == 0
            assert in_zero == (q.max_matches > sc.FLT_ABOVE) and len(r) == q.max_matches, (q.sort, q.max_matches)
            if q.max_matches == 1024:
                assert {0, 0x80000000} <= set(key.tolist())  # both zeros leave with their own bits
    assert set(sc.FLT_KS) == {1, sc.FLT_ABOVE, sc.FLT_ABOVE + 1, 1000, 1024}


def test_int64_column_cycles_its_nine_values(corpora):
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    full = corpora.full(name, m.Query(sc.root_ab(m), ranker=m.SPH_RANK_BM25))
    v = np.ascontiguousarray(rows[full.rowid, sc.I64:sc.I64 + 2]).view(np.int64).reshape(-1)
    got = dict(classes(v))
    assert set(got) == set(sc.I64_VALUES) and len(sc.I64_VALUES) == 9
    assert got[-2**63] == got[2**63 - 1] == 911 and all(got[x] == 910 for x in sc.I64_VALUES[2:])
    # K = 911: the last row of the best class in either direction; 1024 lies in the class behind it
    desc, asc = sorted(sc.I64_VALUES, reverse=True), sorted(sc.I64_VALUES)
    for order_ in (desc, asc):
        sizes = [got[x] for x in order_]
        assert rank_class(sizes, 911) == (0, 0) and rank_class(sizes, 1024) == (1, 911)
    # the low dword must compare unsigned under a signed high dword: pairs of one high dword whose low dwords differ in bit 31
    for x, y in ((0x7FFFFFFF, 0x80000000), (-0x80000001, -0x80000000)):
        assert x < y and (x >> 32) == (y >> 32) and (x & 0xFFFFFFFF) < 2**31 <= (y & 0xFFFFFFFF)
    assert desc[1] == 0x80000000 and asc[1] == -0x80000001  # and they are the classes behind the best one, where K = 1024 lies


def test_weight_first_classes(corpora):
    name = ("S", "high")
    plain = corpora.full(name, m.Query(sc.root_ab(m), ranker=m.SPH_RANK_BM25))
    fb = corpora.full(name, m.Query(sc.root_ab(m), ranker=m.SPH_RANK_BM25, field_weights=list(sc.FALLBACK_FIELD_WEIGHTS)))
    neg = corpora.full(name, m.Query(sc.root_ab(m), ranker=m.SPH_RANK_BM25, field_weights=list(sc.NEGATIVE_FIELD_WEIGHTS)))
    for full in (plain, fb, neg):
        assert [n for _, n in classes(full.weight)] == list(sc.LADDER[::-1])
    assert sc.FALLBACK_FIELD_WEIGHTS[0] * 1000 > 2**31 - 1 and 0 < int(fb.weight.min()) and int(fb.weight.max()) < 2**20
    assert int(neg.weight.max()) < 0 < int(plain.weight.min())
    want = {1: 0, 300: 0, 301: 1, 800: 1, 801: 2, 1024: 2}
    assert set(want) == set(sc.WF_KS)
    for K in sc.WF_KS:
        assert rank_class(sc.LADDER, K)[0] == want[K] and rank_class(sc.LADDER[::-1], K) == (0, 0)  # weight ASC: the class of 7392 leads


# ------------------------------------------------------------------ corpus L
def test_list_corpus_has_its_lengths(corpora):
    hi, oi, rows = corpora.get("L")
    assert hi.total_docs == sc.L_DOCS and [int(d["docs"]) for d in hi.dict] == list(sc.LIST_COUNTS) + [sc.L_DOCS // 8] * 2
    assert np.unique(rows[:, sc.L_DIST]).size == sc.L_DOCS and (rows[:, sc.L_CONST] == 42).all()
    qs = sc.case8(m)
    assert len(qs) == 4 * len(sc.LIST_COUNTS) + 2 and {q.max_matches for q in qs} == {1, 1024} and all(q.sort.then_weight == 0 for q in qs)
    for i, q in enumerate(qs):
        full = corpora.full(("L",), q)
        assert full.total_found == (sc.LIST_COUNTS[i // 4] if i // 4 < len(sc.LIST_COUNTS) else 0)
        if full.total_found:
            assert np.array_equal(np.sort(full.rowid), sc.list_rows_of(i // 4)) and np.unique(full.weight).size == 1
    offsets = np.cumsum([corpora.full(("L",), q).total_found for q in qs])
    assert any(o % sc.WG for o in offsets[:-2])  # back to back: the lists start at no multiple of anything


# ------------------------------------------------------------------ the planner's geometry, under sanitizers
def spec(name, kind, parts, then_weight, fw=(0, 0), probes=()):
    """one QUERY argument of sortsel_geom"""
    p = [sc.COLS[c] + (int(d),) for c, d in parts] + [(0, 0, 0, 0)] * (2 - len(parts))
    words = [name, kind, len(parts)] + [x for (off, cnt, k, d) in p for x in (k, off, cnt, d)] + [then_weight, fw[0], fw[1], ",".join("%x" % x for x in probes)]
    return ":".join(str(x) for x in words)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_planner_geometry_under_sanitizers(tmp_path):
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "sortsel_geom.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + FLAGS + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "sortsel_geom")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    rows = sc.s_rows()
    path = str(tmp_path / "rows.bin")
    with open(path, "wb") as f:
        f.write(np.array(rows.shape, np.uint32).tobytes())
        f.write(rows.tobytes())
    edges = [x for c in range(1, 1024) for x in ((c << 22) - 1, c << 22)]
    i64p = [v & (2**64 - 1) for v in sorted(sc.I64_VALUES)]
    args = []
    for d in (1, 0):
        args += [spec(f"full32.{d}", "s", [("full32", d)], 1, probes=[0] + edges + [0xFFFFFFFF]),
                 spec(f"span1023.{d}", "s", [("span1023", d)], 0, probes=[sc.SPAN_LO, sc.SPAN_LO + 1023]),
                 spec(f"span1024.{d}", "s", [("span1024", d)], 2, probes=[sc.SPAN_LO, sc.SPAN_LO + 1024]),
                 spec(f"span1025.{d}", "s", [("span1025", d)], 1, probes=[sc.SPAN_LO, sc.SPAN_LO + 1025]),
                 spec(f"band.{d}", "s", [("band", d)], 1, probes=[sc.BAND_LO, sc.BAND_LO + 1024]),
                 spec(f"const.{d}", "s", [("const", d)], 1, probes=[42]),
                 spec(f"i64.{d}", "o", [("i64", d)], 1, probes=i64p),
                 spec(f"r255.{d}", "o", [("cat4", 1), ("r255", d)], 1, probes=[(c << 32) | (sc.R_LO + x) for c in (0, 3) for x in (0, 255)]),
                 spec(f"r256.{d}", "o", [("cat4", d), ("r256", 1)], 0, probes=[(c << 32) | (sc.R_LO + x) for c in (0, 3) for x in (0, 256)]),
                 spec(f"const_span.{d}", "o", [("const", 1), ("span1024", d)], 2, probes=[(42 << 32) | (sc.SPAN_LO + x) for x in (0, 1024)])]
    for wf in (1, 2):
        args += [spec(f"wf_fallback.{wf}", "o", [("lad_low", 0)], 0x100 | wf, fw=sc.FALLBACK_FIELD_WEIGHTS, probes=[1, 1524, 1530, 2**31 - 1]),
                 spec(f"wf_plain.{wf}", "o", [("lad_low", 0)], 0x100 | wf, probes=[1524, 1528, 1530]),
                 spec(f"wf_negative.{wf}", "o", [("lad_low", 0)], 0x100 | wf, fw=sc.NEGATIVE_FIELD_WEIGHTS, probes=[(-2476) & 0xFFFFFFFF, (-2470) & 0xFFFFFFFF])]
    out = subprocess.run([exe, path] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("ok %d queries" % len(args)), out.stdout[-500:]
    G = {}
    for line in out.stdout.splitlines():
        mt = re.fullmatch(r"q (\S+) sort_on (\d+) tie (\d+) bin_lo (-?\d+) bin_shift (\d+) geom (\d+) (\d+) (\d+) (\d+) bins ([\d,]*)", line)
        if mt:
            G[mt.group(1)] = dict(sort_on=int(mt.group(2)), tie=int(mt.group(3)), bin_lo=int(mt.group(4)), shift=int(mt.group(5)), nb=int(mt.group(8)),
                                  gshift=int(mt.group(9)), bins=[int(x) for x in mt.group(10).split(",") if x])
    assert len(G) == len(args)
    for d in (1, 0):
        g = G[f"full32.{d}"]
        assert g["sort_on"] == 1 and g["shift"] == 22 and len(g["bins"]) == 2 * 1023 + 2
        b = g["bins"] if d else g["bins"][::-1]  # walked upwards in the mapped key
        assert b == sorted(b) and b[0] == 0 and b[-1] == 1023
        inner = g["bins"][1:-1]
        assert all(inner[2 * i] != inner[2 * i + 1] for i in range(1023))  # c 2^22 - 1 and c 2^22 lie in different bins
        assert G[f"span1023.{d}"]["shift"] == 0 and G[f"span1023.{d}"]["bins"] == ([0, 1023] if d else [1023, 0])
        assert G[f"span1024.{d}"]["shift"] == 1 and G[f"span1024.{d}"]["bins"] == ([0, 512] if d else [512, 0])
        assert G[f"span1025.{d}"]["shift"] == 1 and G[f"span1025.{d}"]["bins"] == ([0, 512] if d else [512, 0])
        g = G[f"band.{d}"]
        assert g["shift"] == 22 and g["bins"][0] == g["bins"][1] and 0 < g["bins"][0] < 1023  # all of BAND's matches lie in one bin, no edge bin
        assert G[f"const.{d}"]["shift"] == 0 and G[f"const.{d}"]["bins"] == [0]
        g = G[f"i64.{d}"]
        assert g["sort_on"] == 2 and g["nb"] == 32 and g["gshift"] == 54 and g["bins"] == (sorted(g["bins"]) if d else sorted(g["bins"], reverse=True))
        assert g["bins"][0 if d else -1] == 0 and g["bins"][-1 if d else 0] == 1023
        assert G[f"r255.{d}"]["nb"] == 8 and G[f"r256.{d}"]["nb"] == 9  # the second part's range of exactly 255 / 256
        assert G[f"r255.{d}"]["gshift"] == 0 and G[f"r256.{d}"]["gshift"] == 1 and len(set(G[f"r255.{d}"]["bins"])) == 4
        g = G[f"const_span.{d}"]
        assert g["nb"] == 11 and g["gshift"] == 1 and sorted(g["bins"]) == [0, 512]  # the first part spans nothing: the second part's bins alone
    for wf in (1, 2):
        g = G[f"wf_fallback.{wf}"]
        assert g["sort_on"] == 3 and g["tie"] == wf and g["bin_lo"] == -2**31 and g["shift"] == 31
        assert g["bins"] == ([1, 1, 1, 1] if wf == 1 else [1022, 1022, 1022, 1022])  # every positive weight in one bin
        g = G[f"wf_plain.{wf}"]
        assert g["sort_on"] == 3 and g["shift"] < 31 and g["bins"] == sorted(g["bins"], reverse=wf == 2)
        g = G[f"wf_negative.{wf}"]
        assert g["sort_on"] == 3 and g["shift"] < 31 and g["bins"] == sorted(g["bins"], reverse=wf == 2)
