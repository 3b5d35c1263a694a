"""CPU: the attribute, float, MVA and weight filters at their edges (filter_edges_common.py).

  - the oracle (oracle/cpu_ref.c::filters_pass, a near copy of the kernel's function) against the plain Python model of the
    reference, on every case, on the 8-field corpus and its 32-field twin, with dead rows and under a cutoff;
  - the corpus holds what it claims, asserted from the built bytes; no case is trivially "all rows" / "no rows" but the listed ones;
  - mrk::row_passes_filters / weight_passes_filters themselves (csrc/mrk_dev.h, compiled for the host) and the load-time blob-row walk
    (csrc/mrk_blobrow.h) in a stand-alone program under AddressSanitizer + UBSan over exact-size allocations (tests/cpp/filter_edges.cpp).

What the stand-alone program catches -- mutants of row_passes_filters, each built once from a scratch copy of mrk_dev.h and run on the
CPU only; the program exits 1 and its `MISMATCH case` lines name the cases:

    32-bit attribute sign-extended                  40 cases: every u32_* but u32_values_8 and the four closed ranges with a strict maximum, pair0_*, w_next_to_u32
    (T) casts of MvaEval_RangeAll dropped           m32_rall_min_minus1, m32_rall_max_2p32_plus_5, pair3_ab, pair3_ba
    MvaEval_RangeAny tests the next value           m32_rany_min_found_strict, m32_rany_at_2p31, m64_rany_min_found_strict, m64_rany_inner, pair3_*
    a two-byte blob length read as one byte         AddressSanitizer stops the program: a read outside the pool
    l0 = 0 for blob attributes behind the first     all 17 m64_* cases, pair2_*, pair3_*, w_next_to_m64
    bit-field mask one bit short                    all 11 bf* cases, pair2_*, pair4_*   (one bit wide: bfa1_is_1, bfb31_ends, bfb31_range_strict)
    float compare on the bit patterns               flt_zeros, flt_denormal_bounds[_strict], flt_nan_max, flt_inf_*, flt_max_exclude,
                                                    flt_strict_below_minus_flt_max, flt_negative, pair1_*"""
import os
import struct
import subprocess

import numpy as np
import pytest

import filter_edges_common as C

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"
CUTOFF = 40


def oracle_index(orc, n_fields):
    W, R, H = C.hits(n_fields)
    oi = orc.build_index(W, R, H, total_docs=C.N_DOCS, n_fields=n_fields, n_terms=C.N_TERMS)
    oi.attrs, oi.blobs = C.attr_rows()
    return oi


@pytest.fixture(scope="module", params=[8, 32])
def world(orc, request):
    """(oracle index, the unfiltered answer's weight per rowid) of one twin"""
    oi = oracle_index(orc, request.param)
    full = orc.search(oi, orc.term(C.T_A, 1), ranker=orc.RANK_BM25, max_matches=C.N_DOCS, field_weights=C.field_weights(request.param))
    assert full.total_found == C.N_DOCS == len(full.rowid)  # keyword A: every row reaches the filter
    return oi, dict(zip(full.rowid.tolist(), full.weight.tolist())), request.param


def run(orc, oi, n_fields, **kw):
    return orc.search(oi, orc.term(C.T_A, 1), ranker=orc.RANK_BM25, max_matches=C.N_DOCS, field_weights=C.field_weights(n_fields), **kw)


def same(r, want_rows, weight_of, what):
    assert r.total_found == len(want_rows), (what, r.total_found, len(want_rows))
    assert sorted(r.rowid.tolist()) == want_rows, what
    assert all(weight_of[d] == w for d, w in zip(r.rowid.tolist(), r.weight.tolist())), what


def test_oracle_against_the_model(orc, world):
    oi, weight_of, n_fields = world
    rows, pool = C.attr_rows()
    every = list(range(C.N_DOCS))
    dead = C.dead_map()
    for case in C.cases():
        same(run(orc, oi, n_fields, filters=case.filters), C.model_rows(case, every, rows, pool), weight_of, case.name)
        same(run(orc, oi, n_fields, filters=case.filters, cutoff=CUTOFF), C.model_rows(case, every, rows, pool, cutoff=CUTOFF), weight_of, (case.name, "cutoff"))
    try:
        oi.dead_rows = dead
        for case in C.cases():
            same(run(orc, oi, n_fields, filters=case.filters), C.model_rows(case, every, rows, pool, dead=dead), weight_of, (case.name, "dead rows"))
    finally:
        oi.dead_rows = None


def test_oracle_weight_filters_against_the_model(orc, world):
    oi, weight_of, n_fields = world
    rows, pool = C.attr_rows()
    for name, fl, wf in C.weight_cases(weight_of.values()):
        want = [r for r in range(C.N_DOCS) if C.row_passes(fl, r, rows, pool) and C.weight_passes(wf, weight_of[r])]
        assert 0 < len(want) < C.N_DOCS, name
        same(run(orc, oi, n_fields, filters=fl or None, weight_filters=wf), want, weight_of, name)


def test_model_on_hand_made_values():
    """the odd corners of the reference, on values small enough to check by eye"""
    assert C.mva_range_any([3, 10, 20, 30], 20, 25, False, True) is True      # minimum found, strict, a next value: true though 30 > 25
    assert C.mva_range_any([10, 20], 20, 25, False, True) is False            # ... found at the last position: no next value
    assert C.mva_range_any([10, 20], 20, 25, True, True) is True
    assert C.mva_range_any([3, 10], 4, 10, True, False) is False and C.mva_range_any([3, 10], 4, 10, True, True) is True
    assert C.mva_range_all([C.U32_MAX], -1, C.U32_MAX, True, True, 32) is True and C.mva_range_all([5], -1, C.U32_MAX, True, True, 32) is False
    assert C.mva_range_all([1, 5], 0, (1 << 32) + 5, True, True, 32) is True and C.mva_range_all([1, 6], 0, (1 << 32) + 5, True, True, 32) is False
    assert C.mva_range_all([-3], -1, 5, True, True, 64) is False
    assert C.mva_any([3, 10, 20, 30], [2, 10, 25]) and not C.mva_any([3, 10, 20, 30], [2, 11, 25]) and not C.mva_any([], [1])
    assert C.mva_all([1, 2], [1, 2, 3]) and not C.mva_all([1, 4], [1, 2, 3]) and not C.mva_all([], [1])
    assert C.eval_values(5, [5]) and C.eval_values(3, [1, 3, 9]) and not C.eval_values(4, [1, 3, 9]) and not C.eval_values(-1, [0, C.U32_MAX])
    row = np.array([0xFFFFFFFF, 0x80000000, 0xF8000001], np.uint32)
    assert C.get_row_attr(row, 0, 32) == C.U32_MAX and C.get_row_attr(row, 32, 32) == 1 << 31
    assert C.get_row_attr(row, 0, 64) == -(1 << 63) + C.U32_MAX and C.get_row_attr(row, 64 + 27, 5) == 31 and C.get_row_attr(row, 64 + 1, 31) == 0x7C000000
    assert C.weight_passes([dict(min=-5, max=5)], -5) and not C.weight_passes([dict(min=-5, max=5, has_equal_min=False)], -5)
    assert C.weight_passes([dict(values=[-7, 2], exclude=True)], 0) and not C.weight_passes([dict(values=[-7, 2], exclude=True)], -7)


def test_corpus_holds_what_it_claims():
    rows, pool = C.attr_rows()
    N = C.N_DOCS
    assert N == 3 * 128 + 36 and rows.shape == (N, C.STRIDE) and C.D_I64 + 2 == C.STRIDE  # the 64-bit attribute ends the row
    offs = [int(rows[r, C.D_BLOB]) | (int(rows[r, C.D_BLOB + 1]) << 32) for r in range(N)]
    # every size class in the headers, at the reference's thresholds, and the blob rows end exactly at the pool's end
    by_total = {}
    for r in range(N):
        total = sum(len(b) for b in C.blob_bytes(r))
        assert int(pool[offs[r]]) == C.blob_size_class(total), (r, total)
        by_total.setdefault(total, []).append(r)
        for attr, bits in (("m32", 32), ("m64", 64)):  # the bytes hold the crafted values
            assert C.row_mva(r, rows, pool, C.BLOB_ID[attr], C.N_BLOB, bits) == C.blob_values(r)[0 if attr == "m32" else 2], (r, attr)
    assert [C.blob_size_class(t) for t in (0, 254, 255, 256, 65534, 65535, 65536)] == [0, 0, 1, 1, 1, 2, 2]
    assert all(t in by_total for t in (0, 254, 255, 256, 65534, 65535, 65536))
    assert {int(pool[o]) for o in offs} == {0, 1, 2}
    last = offs[N - 1]
    assert last + 1 + 4 * C.N_BLOB + 65536 == pool.size and C.blob_values(N - 1)[2] == []  # the last blob row ends on the pool's last byte
    assert {r: t for r, (t, _) in C.SIZED_ROWS.items()} == {0: 0, 63: 254, 64: 255, 127: 65534, 128: 65535, 256: 0, 383: 256, N - 1: 65536}
    # MVA data unaligned: an MVA64 behind a string of odd length, at every alignment of its absolute start
    starts = set()
    for r in range(N):
        m32, slen, m64 = C.blob_values(r)
        if m64:
            sz = (1, 2, 4)[int(pool[offs[r]])]
            starts.add((offs[r] + 1 + C.N_BLOB * sz + 4 * len(m32) + slen) & 7)
    assert starts == set(range(8))
    assert any(slen % 2 == 1 and m64 for _, slen, m64 in map(C.blob_values, range(N)))
    assert any(m32 and slen == 0 and m64 for m32, slen, m64 in map(C.blob_values, range(N)))  # an MVA64 whose neighbour is empty (l0 == l1)
    # every pattern of every attribute in both rows of a lane (doc slot < 64 / >= 64) of every full block, and in the partial block
    sizes = {"u32": len(C.U32_VALUES), "bfa": len(C.BF_PAIRS), "bfb": len(C.BF_PAIRS), "bfc": len(C.BFC_PAIRS), "i64": len(C.I64_VALUES), "flt": len(C.FLOAT_BITS),
             "m32": len(C.M32_LISTS), "m64": len(C.M64_LISTS)}
    for attr, n in sizes.items():
        assert n == C.ATTR_PERIODS[attr] and np.gcd(n, 64) == 1
        for block in range(3):
            for slot in (0, 1):
                rs = [r for r in range(block * 128 + slot * 64, block * 128 + slot * 64 + 64) if attr not in ("m32", "m64") or r not in C.SIZED_ROWS]
                assert {C.pattern_index(attr, r) for r in rs} == set(range(n)), (attr, block, slot)
        assert {C.pattern_index(attr, r) for r in range(384, N)} == set(range(n)), attr
    # the block edges and the last rowid hold the size-class rows; the first rowid an empty blob row
    assert all(r in C.SIZED_ROWS for r in (0, 127, 128, 383, N - 1))
    # the crafted values are in the rows
    assert set(rows[:, C.D_U32].tolist()) == set(C.U32_VALUES)
    assert set(rows[:, C.D_FLT].tolist()) == set(C.FLOAT_BITS)
    assert {C.get_row_attr(rows[r], *C.LOC["i64"]) for r in range(N)} == set(C.I64_VALUES)
    assert {(C.get_row_attr(rows[r], *C.LOC["bfa1"]), C.get_row_attr(rows[r], *C.LOC["bfa31"])) for r in range(N)} == set(C.BF_PAIRS)
    assert {(C.get_row_attr(rows[r], *C.LOC["bfb1"]), C.get_row_attr(rows[r], *C.LOC["bfb31"])) for r in range(N)} == set(C.BF_PAIRS)
    assert {(C.get_row_attr(rows[r], *C.LOC["bfc5"]), int(rows[r, C.D_BFC]) & 0x7FFFFFF) for r in range(N)} == set(C.BFC_PAIRS)
    f = np.array(C.FLOAT_BITS, np.uint32).view(np.float32)
    assert np.isnan(f).sum() == 3 and np.isinf(f).sum() == 2 and sum(1 for b in C.FLOAT_BITS if b & 0x7F800000 == 0 and b & 0x7FFFFF) == 4


def test_no_case_is_trivial_but_the_listed_ones():
    rows, pool = C.attr_rows()
    cases = C.cases()
    assert 110 <= len(cases) <= 140
    for case in cases:
        assert all("values" not in f or (list(f["values"]) == sorted(set(f["values"])) and 1 <= len(f["values"]) <= 8) for f in case.filters), case.name
        n = len(C.model_rows(case, range(C.N_DOCS), rows, pool))
        kind = "none" if n == 0 else "all" if n == C.N_DOCS else None
        assert kind == case.trivial == C.TRIVIAL.get(case.name), (case.name, n)
    assert sum(1 for c in cases if c.trivial) == len(C.TRIVIAL) == 8


def write_input(path, weight_of):
    """rows, pool, the cases as DevFilters and the model's bit per (case, row) for tests/cpp/filter_edges.cpp"""
    rows, pool = C.attr_rows()
    todo = [(c.name, c.filters, []) for c in C.cases()] + list(C.weight_cases(weight_of.values()))
    weights = np.array([weight_of[r] for r in range(C.N_DOCS)], np.int32)
    with open(path, "wb") as fp:
        fp.write(struct.pack("<6Q", 0x47444546, C.STRIDE, C.N_DOCS, pool.size, C.N_BLOB, len(todo)))
        fp.write(np.ascontiguousarray(rows).tobytes())
        fp.write(np.ascontiguousarray(pool).tobytes())
        for name, fl, wf in todo:
            fp.write(struct.pack("<2I", len(fl), len(wf)))
            for lst, on_weight in ((fl, False), (wf, True)):
                img = np.zeros(2, C.DEV_FILTER)
                for i, f in enumerate(lst):
                    img[i] = C.dev_filter(f, on_weight)
                fp.write(img.tobytes())
            fp.write(weights.tobytes())
            fp.write(bytes(int(C.row_passes(fl, r, rows, pool) and C.weight_passes(wf, weight_of[r])) for r in range(C.N_DOCS)))
    return [t[0] for t in todo]


def build_program(tmp_path):
    """hipcc, host side only, AddressSanitizer + UBSan"""
    src = os.path.join(HERE, "cpp", "filter_edges.cpp")
    exe = str(tmp_path / "filter_edges")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-sanitize-recover=undefined", src, "-o", exe])
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_device_functions_on_the_host(orc, tmp_path):
    oi = oracle_index(orc, 8)
    full = run(orc, oi, 8)
    weight_of = dict(zip(full.rowid.tolist(), full.weight.tolist()))
    names = write_input(str(tmp_path / "cases.bin"), weight_of)
    exe = build_program(tmp_path)
    out = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    caught = [names[int(ln.split()[2])] for ln in out.stdout.split("\n") if ln.startswith("MISMATCH case")]
    assert out.returncode == 0, (caught, out.stdout[-1500:], out.stderr[-3000:])
    lines = out.stdout.strip().split("\n")
    assert lines[-2] == f"checked {len(names) * C.N_DOCS}" and lines[-1] == "ok", out.stdout
