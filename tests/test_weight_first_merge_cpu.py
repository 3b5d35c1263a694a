"""CPU: weight-first orders (Order.weight_first) across segments and shards without a device.  (1) the order spec word with
OSPEC_WFIRST: the C builder (tests/cpp/weight_first_spec.cpp, under ASan + UBSan) against dist.order_spec_word(..., weight_first=),
unmap under it, attribute-first specs unchanged; (2) dist.merge_orows_np against the order's definition, a lexsort written in
weight_first_merge_common.py; (3) the loud cases; (4) the reference's recorded weight-first results cut into every 2- and 3-shard
split and merged.  Every comparison is exact."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import sorted_golden_common as sg
import weight_first_merge_common as wmc
from weight_first_expect import expected_weight_first

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
K1 = 1024


def _m():
    import manticoresearch_amd as m

    return m


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_c_builder_equals_the_python_builder_under_sanitizers(tmp_path):
    m = _m()
    from manticoresearch_amd import dist

    exe = str(tmp_path / "weight_first_spec")
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(HERE, "cpp", "weight_first_spec.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert lines[-1].startswith("ok weight-first spec "), lines[-1]
    seen = {}
    for ln in lines[:-1]:
        tag, wf, tw, n_parts, i64, f0, b0, d0, f1, b1, d1, spec = ln.split()
        assert tag == "S"
        wf, tw, n_parts, i64, f0, b0, d0, f1, b1, d1 = (int(x) for x in (wf, tw, n_parts, i64, f0, b0, d0, f1, b1, d1))
        if i64:
            parts = [m.OrderPart(0, 64, desc=bool(d0), kind=m.SORTKEY_INT64)]
        else:
            parts = [m.OrderPart(0, b, desc=bool(d), kind=m.SORTKEY_FLOAT if f else m.SORTKEY_INT) for f, b, d in ((f0, b0, d0), (f1, b1, d1))[:n_parts]]
        py = dist.order_spec_word(parts, tw, weight_first=wf)
        assert py == int(spec, 16), (ln, hex(py))
        assert bool(py & dist.OSPEC_WFIRST) == bool(wf), ln  # bit 3 exactly for weight-first
        if wf:
            assert (py >> 4) & 3 == wf
        else:
            assert py == dist.order_spec_word(parts, tw), ln  # the keyword left alone: the spec as it was
        seen[(wf, n_parts, i64)] = seen.get((wf, n_parts, i64), 0) + 1
    # 5 kinds x 2 directions, x the same for a second part, 2 INT64 directions, no parts under weight ASC only; attribute-first under 3 tie rules
    assert seen == {(0, 1, 0): 30, (0, 2, 0): 300, (0, 1, 1): 6, (1, 1, 0): 10, (1, 2, 0): 100, (1, 1, 1): 2, (2, 1, 0): 10, (2, 2, 0): 100, (2, 1, 1): 2, (2, 0, 0): 1}


def test_python_spec_and_unmap():
    """dist.order_spec_word's refusals, attribute-first specs bit for bit what they were (assembled here from the documented fields),
    dist.unmap_order_keys and mrk_order_unmap_key under a weight-first spec: the parts as without bit 3, 0 without parts."""
    m = _m()
    from manticoresearch_amd import _lib, dist

    P = m.OrderPart
    assert dist.OSPEC_WFIRST == 8
    a, b, f, big = P(0, 5, desc=True), P(32, 32, desc=False), P(64, 32, desc=True, kind=m.SORTKEY_FLOAT), P(96, 64, desc=False, kind=m.SORTKEY_INT64)
    assert dist.order_spec_word([a], 2) == 1 | (2 << 4) | ((2 | (5 << 4)) << 8)
    assert dist.order_spec_word([a, b], 0) == 1 | 2 | ((2 | (5 << 4)) << 8) | ((32 << 4) << 24)
    assert dist.order_spec_word([f, a], 1) == 1 | 2 | (1 << 4) | ((1 | 2 | (32 << 4)) << 8) | ((2 | (5 << 4)) << 24)
    assert dist.order_spec_word([big], 1) == 1 | 2 | 4 | (1 << 4) | ((4 | (32 << 4)) << 8) | ((32 << 4) << 24)
    assert dist.order_spec_word([], 0, weight_first=2) == 1 | 8 | (2 << 4)
    for bad in (lambda: dist.order_spec_word([], 1), lambda: dist.order_spec_word([], 0, weight_first=1), lambda: dist.order_spec_word([a], 0, weight_first=3),
                lambda: dist.order_spec_word([a, b, a], 0, weight_first=1)):
        with pytest.raises(AssertionError):
            bad()
    unmap_c = _lib.lib().mrk_order_unmap_key
    rng = np.random.default_rng(3)
    mapped = rng.integers(0, 2 ** 64, 300, dtype=np.uint64)
    for parts in ([a], [a, b], [f, a], [big]):
        for wf in (1, 2):
            spec, plain = dist.order_spec_word(parts, 0, weight_first=wf), dist.order_spec_word(parts, wf)
            assert spec == plain | dist.OSPEC_WFIRST
            got = dist.unmap_order_keys(spec, mapped)
            assert np.array_equal(got, dist.unmap_order_keys(plain, mapped))
            assert got.tolist() == [unmap_c(spec, int(x)) for x in mapped] == [unmap_c(plain, int(x)) for x in mapped]
    none = dist.order_spec_word([], 0, weight_first=2)
    assert not dist.unmap_order_keys(none, mapped).any() and all(unmap_c(none, int(x)) == 0 for x in mapped[:20])
    hdr = open(os.path.join(ROOT, "include", "mrk.h")).read()
    assert "mrk_batch_orows_weight_first" in hdr and hasattr(_lib.lib(), "mrk_batch_orows_weight_first") and hasattr(m.Batch, "orows_weight_first")


@pytest.mark.parametrize("flavor,wf", wmc.FLAVORS)
def test_merge_orows_np_equals_the_definition(flavor, wf):
    """5 distinct weights and 3 distinct mapped keys per list: ties reach the mapped key and the docid.  List counts 1, 2, 3, 5, 8, k in
    1, 7, 1024, per-list counts 0, 1, partial, 1024."""
    from manticoresearch_amd import dist

    levels = set()
    for (f, w, n, k), (rows, want) in wmc.size_references().items():
        if (f, w) != (flavor, wf):
            continue
        got = dist.merge_orows_np(rows, k)
        assert np.array_equal(got, want), (flavor, wf, n, k)
        if n > 1:
            levels |= wmc.levels_decided(rows, k)
    assert levels == ({1, 3} if flavor == "none" else {1, 2, 3})  # (without parts every mapped key is 0: it decides nothing)


def test_merge_orows_np_is_loud():
    from manticoresearch_amd import dist

    for name, rows in wmc.loud_cases():
        for k in (7, 1024):
            got = dist.merge_orows_np(rows, k)
            wmc.assert_loud(dist, rows, got, name)
        # the same merged row whichever list was the odd one: queries 0 / 1 / 2 differ in its place only where the lists' contents do
        if name.startswith("declined-spec0"):
            assert len({int(got[q, -1]) for q in range(rows.shape[1])}) == 1 and int(got[0, -1]) == wmc.spec_of("int64", 2)
            perm = rows[::-1].copy()
            assert np.array_equal(dist.merge_orows_np(perm, 1024), got), name
    # MRK_ROW_RERUN is OR-ed through, next to a decline and on its own
    rng = np.random.default_rng(5)
    rows = np.stack([np.stack([wmc.make_list(rng, "two", 1, 30, 1 + l * 2048, flags=dist.ROW_RERUN if l == 1 else 0) for _ in range(1)]) for l in range(3)])
    got = dist.merge_orows_np(rows, 1024)
    assert int(got[0, K1 + 1]) & dist.ROW_RERUN and not int(got[0, K1 + 1]) & dist.ROW_DECLINED and int(got[0, K1]) == 90
    rows[2, 0, -1] = wmc.spec_of("two", 2)
    wmc.assert_loud(dist, rows, dist.merge_orows_np(rows, 1024), "rerun next to a mismatch")


def _oracle_index(orc, m, corpus, lo=0, hi=None):
    from test_gpu_parity import orc_index_of

    host = corpus.index(m, lo, hi)
    oi = orc_index_of(orc, host)
    oi.host = host  # (the oracle's arrays are views into the host index: it must outlive them)
    oi.attrs = np.ascontiguousarray(corpus.rows[lo:hi])
    return oi


def _recorded_cases(m):
    """(case, corpus, query) of the fixture's two weight-first sorters, in the Order translation tests/test_weight_first_cpu.py pins"""
    out = []
    case = next(c for c in sg.CASES if c["source"] == "test/test_016/test.xml:38")
    corpus = sg.Corpus(case["corpus"])
    out.append((case, corpus, dataclasses.replace(sg.base_query(m, corpus, case), order=m.Order(parts=[], weight_first=2))))
    case = next(c for c in sg.CASES if c["source"] == "test/test_106/test.xml:59")
    corpus = sg.Corpus(case["corpus"])
    off, bits, kind = corpus.loc["date_added"]
    out.append((case, corpus, dataclasses.replace(sg.base_query(m, corpus, case), order=m.Order([m.OrderPart(off, bits, desc=True, kind=kind)], weight_first=1))))
    return out


def test_recorded_corpora_sharded_equal_unsharded_at_every_cut_and_k(orc):
    """test_016:38 and test_106:59 cut into every 2- and 3-shard split: each shard ranked by the oracle with the corpus-wide statistics,
    packed into order rows, merged by merge_orows_np -> the unsharded weight_first_expect list (which test_weight_first_cpu.py holds
    against the recorded one; nothing more is said here about the inner order of test_106's three fully tied pairs), at every K."""
    m = _m()
    from manticoresearch_amd import dist

    for case, corpus, q0 in _recorded_cases(m):
        q = corpus.globalize(q0)
        whole = _oracle_index(orc, m, corpus)
        rid, w, okey, total = expected_weight_first(orc, whole, q, corpus.rows, corpus.n)
        assert total == case["total_found"] == len(rid)
        n_cuts = 0
        for shards in (2, 3):
            for cuts in corpus.cuts(shards):
                orows = np.zeros((shards, 1, dist.OROW_WORDS), np.uint64)
                for s in range(shards):
                    oi = _oracle_index(orc, m, corpus, cuts[s], cuts[s + 1])
                    ans = wmc.wf_answer(orc, oi, q, oi.attrs, cuts[s + 1] - cuts[s], expected_weight_first)
                    orows[s, 0] = wmc.pack_wf_orow(ans[0], ans[1], ans[2], ans[4], cuts[s], q)
                for K in sorted(set(range(1, total + 1)) | {1024}):
                    row = dist.merge_orows_np(orows, K)[0]
                    n = min(K, total)
                    assert int(row[K1]) == n and int(row[K1 + 1]) == total and int(row[-1]) == wmc.query_spec(q), (case["name"], cuts, K)
                    weight, mapped, docid = wmc.decode(row)
                    assert docid.tolist() == rid[:n].tolist() and weight.tolist() == w[:n].tolist(), (case["name"], cuts, K)
                    vals = dist.unmap_order_keys(int(row[-1]), mapped)
                    assert not vals.any() if okey is None else np.array_equal(vals, okey[:n]), (case["name"], cuts, K)
                n_cuts += 1
        assert n_cuts == len(corpus.cuts(2)) + len(corpus.cuts(3)) > 0
