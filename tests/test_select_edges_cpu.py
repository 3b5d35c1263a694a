"""CPU: the relevance top-K selection's edge cases (csrc/mrk_select.hip) before they reach a GPU.  The arithmetic a
CPU can call -- weight_bin, rowid_bin, SubKey::sub and sub_guard of csrc/mrk_sortkey.h -- and the planner's bin geometry are held
against the definition of the sorter's order by a host-only program under AddressSanitizer + UBSan (tests/cpp/select_subkey.cpp);
and every corpus of tests/test_gpu_select_edges.py is shown to have the structure its case names, read off the oracle's full match
list: class sizes, their order, the class that holds rank K.  The oracle's own K-sized queue must equal the definition's cut of
that list, which pins its tie order where the GPU tests cannot."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import manticoresearch_amd as m
import select_edges_common as se
from test_gpu_parity import to_orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def corpora(orc):
    return se.Corpora(m, orc)


def oracle_equals_cut(orc, oi, q, full):
    """the oracle's K-sized queue against the definition's cut of its own full list"""
    got = to_orc(orc, q).run(oi)
    rid, w, total = se.cut(full, q.max_matches)
    assert got.total_found == total
    assert np.array_equal(got.rowid, rid) and np.array_equal(got.weight, w), (q.max_matches, got.rowid[:5], rid[:5])


def same_bytes(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("spd", "spp", "spe")) and a.dict.tobytes() == b.dict.tobytes() and a.total_docs == b.total_docs


def rows_of_class(full, weight):
    return np.sort(full.rowid[full.weight == weight])


# ------------------------------------------------------------------ cases A, B: the ladders
# the class that holds rank K and the matches above it, as the issue names them
LADDER_RANKS = {"L1": {1: (0, 0), 299: (0, 0), 300: (0, 0), 301: (1, 300), 799: (1, 300), 800: (1, 300), 801: (2, 800), 1000: (2, 800), 1024: (2, 800)},
                "L2": {301: (1, 300), 1000: (1, 300), 1024: (1, 300)},
                "ONE": {1: (0, 0), 2: (0, 0), 1000: (0, 0), 1024: (0, 0)}}


@pytest.mark.parametrize("ladder,placement", [(l, p) for l in ("L1", "L2") for p in se.PLACEMENTS] + [("ONE", "low")])
def test_ladder_corpus_has_its_classes(orc, corpora, ladder, placement):
    name = ("shared", ladder, placement)
    hi, oi = corpora.get(*name)
    assert hi.total_docs == se.SHARED_DOCS and [int(d["docs"]) for d in hi.dict] == [se.SHARED_MATCHES] * 2  # a quarter of the rowids: idf > 0
    full = corpora.full(name, "bm25", se.q_and(m, 1000))
    cls = se.classes(full)
    assert [n for _, n in cls] == [n for n in se.LADDERS[ladder] if n]  # best class first: b's tf 3, 2, 1
    assert [w for w, _ in cls] == sorted({w for w, _ in cls}, reverse=True) and len({w for w, _ in cls}) == len(cls)
    assert full.total_found == se.SHARED_MATCHES
    if len(cls) == 3:  # where the better classes lie
        r = [rows_of_class(full, w) for w, _ in cls]
        if placement == "low":
            assert r[0][-1] < r[1][0] and r[1][-1] < r[2][0] and r[0][0] == 0
        elif placement == "high":
            assert r[0][0] > r[1][-1] and r[1][0] > r[2][-1] and r[0][-1] == se.SHARED_DOCS - 4
        else:
            for rows, n in zip(r[:2], se.LADDERS[ladder][:2]):
                per = np.bincount(rows // (se.SHARED_DOCS // 10), minlength=10)
                assert per.min() >= n // 10 - 1 and per.max() <= n // 10 + 1
    assert set(LADDER_RANKS[ladder]) == set(se.LADDER_KS[ladder])
    for K in se.LADDER_KS[ladder]:
        assert se.rank_class(cls, K) == LADDER_RANKS[ladder][K], K
        oracle_equals_cut(orc, oi, se.q_and(m, K), full)
    assert same_bytes(hi, se.shared_index(m, ladder, placement))


# ------------------------------------------------------------------ cases D, E: the same corpus under rowid bins and the fallback geometry
def test_rank_none_is_one_class_and_field_weights_stay_in_int32(orc, corpora):
    name = ("shared", "L2", "even")
    hi, oi = corpora.get(*name)
    none = corpora.full(name, "none", se.q_and(m, 1000, ranker=m.SPH_RANK_NONE))
    assert se.classes(none) == [(1, se.SHARED_MATCHES)]
    for K in (1, 1000, 1024):
        oracle_equals_cut(orc, oi, se.q_and(m, K, ranker=m.SPH_RANK_NONE), none)
    assert (se.cut(none, 1024)[0] == np.arange(1024) * 4).all()  # all weights equal: the lowest rowids
    fw = list(se.FALLBACK_FIELD_WEIGHTS)
    assert fw[0] * 1000 > 2**31 - 1 and se.FIELD == 1  # field 0's weight alone leaves int32 once it is scaled; no hit lies there
    fb = corpora.full(name, "fallback", se.q_and(m, 1000, field_weights=fw))
    plain = corpora.full(name, "bm25", se.q_and(m, 1000))
    assert int(fb.weight.max()) < 2**20 and int(fb.weight.min()) > 0  # inside int32 by far, and all in the fallback's sub-bin 0
    assert se.classes(fb) == se.classes(plain) and [n for _, n in se.classes(fb)] == list(se.LADDERS["L2"])
    for K in (1000, 1024):
        assert se.rank_class(se.classes(fb), K) == (1, 300)
        oracle_equals_cut(orc, oi, se.q_and(m, K, field_weights=fw), fb)
    assert se.BASES[2] + se.SHARED_DOCS == 2**32 and se.BASES[1] == 1 << 24


# ------------------------------------------------------------------ cases C, G: lists of 2048 j +- 1 keys
def test_slice_corpus_has_its_lists(orc, corpora):
    name = ("slices",)
    hi, oi = corpora.get(*name)
    assert [int(d["docs"]) for d in hi.dict] == list(se.SLICE_COUNTS) + [se.SLICE_DOCS // 4]
    assert {n % 2048 for n in se.SLICE_COUNTS} == {0, 1, 2047} and max(se.SLICE_COUNTS) > 3 * 2048
    for t, n in enumerate(se.SLICE_COUNTS):
        full = corpora.full(name, ("one", t), se.q_one(m, t, 1000))
        cls = se.classes(full)
        assert full.total_found == n
        if n > se.SLICE_TOP:
            assert [c for _, c in cls] == [se.SLICE_TOP, n - se.SLICE_TOP] and cls[0][0] > cls[1][0]
            assert np.array_equal(rows_of_class(full, cls[0][0]), se.slice_rows(t)[-se.SLICE_TOP:])  # the class on top is found last
            for K in (1000, 1024):
                assert se.rank_class(cls, K) == (1, se.SLICE_TOP)  # rank K lies in the tf-1 class, ten above it
        else:
            assert cls == [(cls[0][0], 1)]
        for K in (1, 1000, 1024):
            oracle_equals_cut(orc, oi, se.q_one(m, t, K), full)
        both = corpora.full(name, ("and", t), se.q_with_dense(m, t))
        assert both.total_found == np.intersect1d(se.slice_rows(t), se.slice_rows(se.SLICE_DENSE)).size
        oracle_equals_cut(orc, oi, se.q_with_dense(m, t), both)
    assert any(corpora.full(name, ("and", t), None).total_found > 1024 for t in range(len(se.SLICE_COUNTS)))
    assert same_bytes(hi, se.slice_index(m))
    batch = se.slice_batch(m)
    assert len(batch) == 27 and [q.max_matches for q in batch] == [1000] * 9 + [1024] * 9 + [1000] * 9
    group = se.group_batch(m)
    assert len(group) == se.GROUP_QUERIES > 4096 and len(set(group)) <= 27
    assert [se.SLICE_COUNTS[t] for t, _ in group[4093:]] == [4097, 6143, 6145, 4097, 6143, 6145, 4097]
    assert {k for _, k in group} == {1, 1000, 1024} and {t for t, _ in group} == set(range(9))


# ------------------------------------------------------------------ case F: two chunks of slices
def test_chunk_corpus_has_its_classes(orc, corpora):
    name = ("chunks",)
    hi, oi = corpora.get(*name)
    assert int(hi.dict[0]["docs"]) == se.CHUNK_DOCS > 2**21 and hi.total_docs == 4 * se.CHUNK_DOCS
    full = corpora.full(name, "one", se.q_one(m, 0, 1000))
    cls = se.classes(full)
    assert [n for _, n in cls] == [se.CHUNK_TOP, se.CHUNK_DOCS - se.CHUNK_TOP] and cls[0][0] > cls[1][0]
    assert se.rank_class(cls, 1000) == (1, se.CHUNK_TOP)
    rid, w, total = se.cut(full, 1000)
    assert rid.tolist() == list(range(se.CHUNK_DOCS - se.CHUNK_TOP, se.CHUNK_DOCS)) + list(range(1000 - se.CHUNK_TOP)) and total == se.CHUNK_DOCS
    oracle_equals_cut(orc, oi, se.q_one(m, 0, 1000), full)


# ------------------------------------------------------------------ the arithmetic and the planner, under sanitizers
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_subkey_bins_and_planner_under_sanitizers(tmp_path, corpora):
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "select_subkey.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + FLAGS + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "select_subkey")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    # the rank-K classes' weights of cases A-C, F (and G, which reuses C's): DOCS:DF0[:DF1]:weights
    args, n_w = [], 0

    def spec(docs, dfs, full):
        nonlocal n_w
        ws = [w for w, _ in se.classes(full)]
        n_w += len(ws)
        args.append(":".join(str(x) for x in [docs] + dfs) + ":" + ",".join(str(w) for w in ws))

    for ladder in ("L1", "L2", "ONE"):
        spec(se.SHARED_DOCS, [se.SHARED_MATCHES] * 2, corpora.full(("shared", ladder, "low"), "bm25", se.q_and(m, 1000)))
    for t, n in enumerate(se.SLICE_COUNTS):
        spec(se.SLICE_DOCS, [n], corpora.full(("slices",), ("one", t), se.q_one(m, t, 1000)))
        if corpora.full(("slices",), ("and", t), se.q_with_dense(m, t)).total_found:
            spec(se.SLICE_DOCS, [n, se.SLICE_DOCS // 4], corpora.full(("slices",), ("and", t), None))
    spec(4 * se.CHUNK_DOCS, [se.CHUNK_DOCS], corpora.full(("chunks",), "one", se.q_one(m, 0, 1000)))
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.startswith("ok bins "), out.stdout
    # three bases of case D + case E's fallback + one plan per argument; every weight handed over was checked
    assert re.search(r"plans %d interior %d$" % (4 + len(args), n_w), out.stdout.strip()), (out.stdout, len(args), n_w)
    got = {k: int(v) for v, k in re.findall(r"(\d+) (bin0|top|nobits|wide|empty|accepted|geometries)", out.stdout)}
    assert got["accepted"] > 1000 and min(got["bin0"], got["top"], got["nobits"], got["wide"]) > 0, out.stdout
