"""CPU: grouped queries with aggregates across segments and shards without a device.  (1) the new symbols, the row's layout, the
aggregate spec word in C and in Python; (2) dist.merge_arows_np -- the numpy mirror of merge_arows_kernel -- against
group_aggr_expect's model over the WHOLE match set, with every shard's aggregate row built by the test from the oracle's matches inside
the shard's rowid range: all three funcs x {INT, a 7-bit bit-field, widened, signed INT64}, with and without an ordering aggregate, at
1 / 2 / 3 / 8 lists, staged merges; (3) the reference's recorded aggregates cut into every split of 1..3 lists; (4) flags, mismatches
and hostile rows in the mirror; (5) the merge restated over GroupSeqOps, the kernels' row reader and the spec pack / unpack in a
stand-alone program under ASan + UBSan (tests/cpp/aggr_merge.cpp), which also holds the fifth decline bit's truth table.  Every
comparison is exact."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import aggr_merge_common as amc
import group_aggr_expect as gae
import group_expect as ge
import group_merge_common as gmc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"

N_DOCS, PROBS = 6000, [1.0, 0.6, 0.4, 0.3, 0.2]
CUTS = {1: [0, N_DOCS], 2: [0, 2501, N_DOCS], 3: [0, 1500, 4001, N_DOCS], 8: [0, 700, 1500, 2200, 3000, 3800, 4500, 5300, N_DOCS]}


class A:  # an aggregate as the model and the spec word read it (api.Aggr's fields)
    def __init__(self, func, kind=gae.KIND_INT, widen=False):
        self.func, self.kind, self.widen = func, kind, widen


def test_symbols_layout_and_spec_word():
    import manticoresearch_amd as m
    from manticoresearch_amd import _lib, dist

    G = gmc.G
    assert m.AROW_WORDS == _lib.AROW_WORDS == dist.AROW_WORDS == amc.WORDS == 6 * m.GROW_GROUPS + 4 == 24580 and hasattr(m.Batch, "export_arows")
    assert (dist.AROW_AGGR, dist.AROW_GSPEC, dist.AROW_ASPEC) == (amc.AGGR, amc.GSPEC, amc.ASPEC) == (2 * G + 2, 6 * G + 2, 6 * G + 3)
    assert m.GROW_WORDS == 2 * G + 3, "the group row keeps its layout"
    hdr = open(os.path.join(ROOT, "include", "mrk.h")).read()
    assert re.search(r"#define\s+MRK_AROW_WORDS\s+\(6 \* MRK_GROW_GROUPS \+ 4\)", hdr)
    for name in ("mrk_batch_export_arows", "mrk_topk_merge_arows", "mrk_topk_merge_arows_async", "mrk_topk_merge_arows_part", "mrk_shard_exchange_arows", "mrk_aggr_spec_word"):
        assert hasattr(_lib.lib(), name) and name in hdr, name
    lib = _lib.lib()
    assert lib.mrk_topk_merge_arows.argtypes == lib.mrk_topk_merge_grows.argtypes and lib.mrk_topk_merge_arows_part.argtypes == lib.mrk_topk_merge_grows_part.argtypes
    assert lib.mrk_topk_merge_arows_async.argtypes == lib.mrk_topk_merge_grows_async.argtypes and lib.mrk_shard_exchange_arows.argtypes == lib.mrk_shard_exchange_grows.argtypes
    assert lib.mrk_aggr_spec_word.argtypes[0] == C.POINTER(_lib.Aggrs) and lib.mrk_aggr_spec_word.restype == C.c_uint64
    assert C.sizeof(_lib.Aggr) == 20 and C.sizeof(_lib.Aggrs) == 88, "the structs the spec word is made from keep their sizes"

    def c_word(aggrs, order_by, sort_by=ge.GROUPSORT_KEY):
        ca = _lib.Aggrs()
        ca.n, ca.order_by = len(aggrs), order_by
        for i, a in enumerate(aggrs[:4]):
            ca.a[i] = _lib.Aggr(a.func, a.kind, 64 * i, 64 if a.kind == gae.KIND_INT64 else 32, a.widen if isinstance(a.widen, int) and not isinstance(a.widen, bool) else (1 if a.widen else 0))
        return lib.mrk_aggr_spec_word(C.byref(ca), sort_by)

    kinds = [(gae.KIND_INT, False), (gae.KIND_INT, True), (gae.KIND_INT64, False)]
    n_words = 0
    for n in (1, 2, 3, 4):
        for combo in itertools.product(range(9), repeat=min(n, 2)):
            aggrs = [A(1 + combo[i % len(combo)] // 3, *kinds[(combo[i % len(combo)] + i // 2) % 3]) for i in range(n)]
            for order_by in range(-1, n):
                w = dist.aggr_spec_word(aggrs, order_by)
                want = 1 | (n << 1) | ((order_by + 1) << 4)
                for i, a in enumerate(aggrs):
                    want |= (a.func | (4 if a.kind == gae.KIND_INT64 else 0) | (8 if a.widen else 0)) << (8 + 4 * i)
                assert w == want
                ok = order_by < 0 or (aggrs[order_by].kind == gae.KIND_INT and not aggrs[order_by].widen)
                assert c_word(aggrs, order_by) == (w if ok else 0), (n, combo, order_by)
                un = dist.aggr_spec_unpack(w, ge.GROUPSORT_KEY)
                assert (un is not None) == ok
                if ok:
                    assert un == (n, order_by, [(a.func, a.kind == gae.KIND_INT64, bool(a.widen)) for a in aggrs])
                    for by in (ge.GROUPSORT_COUNT, ge.GROUPSORT_WEIGHT):  # an order stands next to GROUPSORT_KEY only
                        assert c_word(aggrs, order_by, by) == (w if order_by < 0 else 0) and (dist.aggr_spec_unpack(w, by) is not None) == (order_by < 0)
                n_words += 1
    assert n_words == 9 * 2 + 81 * (3 + 4 + 5)
    # each invalid one is 0 in C and None in Python
    ok = A(gae.AGGR_SUM)
    assert lib.mrk_aggr_spec_word(None, 0) == 0 and dist.aggr_spec_word([], -1) == 0 and dist.aggr_spec_word(None) == 0
    for aggrs, order_by in (([], -1), ([ok] * 5, -1), ([A(0)], -1), ([A(4)], -1), ([A(1, kind=gae.KIND_FLOAT)], -1), ([A(1, kind=3)], -1), ([A(1, widen=2)], -1),
                            ([A(1, gae.KIND_INT64, widen=True)], -1), ([ok], 1), ([ok], -2), ([A(1, widen=True)], 0), ([A(3, gae.KIND_INT64)], 0)):
        assert c_word(aggrs, order_by) == 0, (len(aggrs), order_by)
    assert c_word([ok], -1, 3) == 0
    good = dist.aggr_spec_word([ok, A(gae.AGGR_MAX, gae.KIND_INT64)], 0)
    for bad in (0, good & ~1, good | 0x80, good | (1 << 24), good | (1 << 63), good | (1 << 16), (good & ~0xE) | (5 << 1), good & ~0xE, good & ~(3 << 8), good | (8 << 12),
                dist.aggr_spec_word([ok, A(gae.AGGR_MAX, gae.KIND_INT64)], 1), dist.aggr_spec_word([ok], 1), dist.aggr_spec_word([A(1, widen=True)], 0)):
        assert dist.aggr_spec_unpack(bad, 0) is None, hex(bad)


class _Corpus:
    def __init__(self, orc):
        import manticoresearch_amd as m
        from test_gpu_group_aggr import make_rows
        from test_gpu_parity import orc_index_of

        self.m = m
        self.hi = m.synth_index(N_DOCS, PROBS, seed=61, n_fields=4, max_pos=6)
        self.rows = make_rows(N_DOCS)
        self.oi = orc_index_of(orc, self.hi)
        self.oi.attrs = self.rows
        self.cache = {}

    def matches(self, orc, q):
        key = (repr(q.root), q.ranker, q.group.bit_offset, q.group.bit_count, repr(q.aggrs))
        if key not in self.cache:
            self.cache[key] = amc.whole_matches(orc, self.oi, q, self.rows, N_DOCS)
        return self.cache[key]


@pytest.fixture(scope="module")
def corpus(orc):
    return _Corpus(orc)


def _cases(m):
    """(query, must the model answer): every func over every source kind, four at once; each 32-bit result ordering, both directions"""
    from test_gpu_group import BITS, C17, C64
    from test_gpu_group_aggr import BIG, I64, Q

    Ag, I6 = m.Aggr, m.SORTKEY_INT64
    out = []
    for fi, func in enumerate((m.AGGR_SUM, m.AGGR_MIN, m.AGGR_MAX)):
        four = [Ag(func, BIG * 32, 32), Ag(func, BITS * 32 + 9, 7), Ag(func, BIG * 32, 32, widen=True), Ag(func, I64 * 32, 64, kind=I6)]
        for sh, (by, desc) in zip(("one", "and2"), ((ge.GROUPSORT_COUNT, True), (ge.GROUPSORT_WEIGHT, False))):
            out.append((Q(m, sh, C64, four, K=20, by=by, desc=desc), True))
        for order in (0, 1):
            for desc in (True, False):
                out.append((Q(m, ("and2", "one", "tree")[fi], C64, four, K=16 + order, desc=desc, order=order), True))
        out.append((Q(m, "one", C17, four[:1 + fi], K=4), False))
    return out


def test_merge_np_equals_the_model_over_the_whole_match_set(orc, corpus):
    from manticoresearch_amd import dist

    cases = _cases(corpus.m)
    n_decl = 0
    for i, (q, must) in enumerate(cases):
        mt = corpus.matches(orc, q)
        one = amc.shard_arows_np(q, mt, CUTS[1])[:, None, :]
        for S in (1, 2, 3, 8):
            rows = amc.shard_arows_np(q, mt, CUTS[S])[:, None, :]
            merged = dist.merge_arows_np(rows, 1024)
            n_decl += amc.check_merged(dist, q, mt, merged[0], ("lists", S, i), must)
            if must:
                assert np.array_equal(merged[0], one[0, 0]), ("the row of the whole match set", S, i)
            assert np.array_equal(amc.staged(dist.merge_arows_np, rows, 1024), merged), ("staged", S, i)
            assert np.array_equal(dist.merge_arows_np(rows[::-1], 1024), merged), ("the lists' order", S, i)
            assert np.array_equal(dist.merge_arows_np(rows, q.max_matches), merged), ("k = the query's own", S, i)
    assert n_decl == 4 * sum(not must for _, must in cases) == 12


def test_the_reference_recorded_aggregates_in_every_split():
    """tests/golden/group_aggr_vectors.json: each case's three rows dealt to 1..3 lists in every way; the merged row gives the recorded groups"""
    from manticoresearch_amd import dist

    with open(os.path.join(HERE, "golden", "group_aggr_vectors.json")) as fp:
        v = json.load(fp)
    funcs = {"sum": gae.AGGR_SUM, "min": gae.AGGR_MIN, "max": gae.AGGR_MAX}
    by = {"key": ge.GROUPSORT_KEY, "count": ge.GROUPSORT_COUNT, "weight": ge.GROUPSORT_WEIGHT}
    assert len(v["cases"]) == 4
    n_splits = 0
    for c in v["cases"]:
        rows = np.array(c["rows"], np.int64)
        assert len(rows) == 3
        q = type("Q", (), {})()
        q.group = type("G", (), dict(sort_by=by[c["sort_by"]], desc=c["desc"], bit_count=32))()
        q.max_matches, q.aggrs, q.aggr_order = v["max_matches"], [A(funcs[c["func"]])], -1
        for L in (1, 2, 3):
            for deal in itertools.product(range(L), repeat=3):
                lists = []
                for l in range(L):
                    mine = rows[np.array(deal) == l]
                    lists.append(amc.arow_of_matches(q, mine[:, 0].astype(np.uint32), mine[:, 1], mine[:, 2].astype(np.uint32), [mine[:, 3].astype(np.uint64)]))
                merged = dist.merge_arows_np(np.stack(lists)[:, None, :], 1024)[0]
                r, w, k, cnt, total, ag = dist.arow_groups(merged)
                assert total == len(c["groups"]) and ag.shape == (total, 1), (c["source"], deal)
                for i, (hid, key, count, value) in enumerate(c["groups"]):
                    assert int(k[i]) == key and int(ag[i, 0]) == value, (c["source"], deal, i)
                    assert hid is None or int(r[i]) == hid
                    assert count is None or int(cnt[i]) == count
                n_splits += 1
    assert n_splits == 4 * (1 + 8 + 27)


def test_flags_mismatches_and_hostile_rows_in_the_mirror(orc, corpus):
    from manticoresearch_amd import dist
    from test_gpu_group import C16
    from test_gpu_group_aggr import BIG, I64, Q

    m = corpus.m
    aggrs = [m.Aggr(m.AGGR_SUM, BIG * 32, 32), m.Aggr(m.AGGR_MIN, I64 * 32, 64, kind=m.SORTKEY_INT64)]
    q = Q(m, "and2", C16, aggrs, K=10, order=0)
    mt = corpus.matches(orc, q)
    base = amc.shard_arows_np(q, mt, CUTS[3])[:, None, :]
    spec, aspec, R, D = amc.spec_of(q), amc.aspec_of(q), amc.RERUN, amc.DECLINED
    assert not amc.check_merged(dist, q, mt, dist.merge_arows_np(base, 1024)[0], "base", True)

    def with_list(l, f):
        rows = base.copy()
        f(rows[l, 0])
        return dist.merge_arows_np(rows, 1024)[0]

    def rerun(row):
        row[:amc.GSPEC], row[amc.TOTAL] = 0, R

    def planner_declined(row):
        row[:], row[amc.TOTAL] = 0, D

    def own_declined(row):
        row[:amc.GSPEC], row[amc.TOTAL] = 0, D

    def setw(at, value):
        def f(row):
            row[at] = value
        return f

    g2 = dist.aggr_spec_word
    hostile = [setw(amc.CNT, amc.G + 1), setw(amc.CNT, 0xFFFFFFFFFFFFFFFF), setw(amc.GSPEC, spec | (1 << 40)), setw(amc.GSPEC, 0), setw(amc.GSPEC, dist.group_spec_word(1, 1, 32, 10)),
               setw(amc.ASPEC, aspec | 0x80), setw(amc.ASPEC, aspec | (1 << 24)), setw(amc.ASPEC, aspec & ~0xE), setw(amc.ASPEC, (aspec & ~0xE) | (5 << 1)), setw(amc.ASPEC, aspec & ~(3 << 8)),
               setw(amc.ASPEC, aspec | (1 << 16)), setw(amc.ASPEC, aspec | (8 << 12)), setw(amc.ASPEC, g2(aggrs, 1)), setw(amc.ASPEC, (aspec & ~0x70) | (3 << 4))]
    for fault, flags in [(rerun, R), (planner_declined, D), (own_declined, D)] + [(h, D) for h in hostile]:
        got = [with_list(l, fault) for l in range(3)]
        assert amc.is_empty(got[0], flags, spec, aspec) and np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), fault
    both = base.copy()
    rerun(both[0, 0]), planner_declined(both[2, 0])
    assert amc.is_empty(dist.merge_arows_np(both, 1024)[0], R | D, spec, aspec)
    # the aggregate spec words of the answering lists must be equal in every bit: the first answering list's two words stay
    for other in (aspec ^ (2 << 8), aspec ^ (1 << 4), g2(aggrs[:1], 0), g2(aggrs + aggrs[:1], 0), 0):
        for l in range(3):
            rows = base.copy()
            rows[l, 0, amc.ASPEC] = other
            assert amc.is_empty(dist.merge_arows_np(rows, 1024)[0], D, spec, other if l == 0 else aspec), (hex(other), l)
    rows = base.copy()
    rows[1, 0, amc.GSPEC] = dist.group_spec_word(0, 0, 32, 10)
    assert amc.is_empty(dist.merge_arows_np(rows, 1024)[0], D, spec, aspec)
    assert amc.is_empty(dist.merge_arows_np(base, 9)[0], D, spec, aspec), "max_matches above the call's k"
    rel = base.copy()
    rel[2, 0] = amc.arow_of_relevance(np.array([5, 9]), np.array([7, 7]), 2)
    assert amc.is_empty(dist.merge_arows_np(rel, 1024)[0], D, spec, aspec)
    got = dist.merge_arows_np(rel[::-1], 1024)[0]  # the relevance row first: spec words 0 and the narrow merge's sum of totals under the flag
    assert int(got[amc.TOTAL]) == D | int(rel[:, 0, amc.TOTAL].sum()) and int(got[amc.CNT]) == 0 and not got[:amc.G].any() and not got[amc.PLANE:].any()


def test_no_aggregates_and_relevance_rows_merge_as_group_rows_do(orc, corpus):
    """spec-0 rows and grouped rows without aggregates: words [0, 2G+2) and the group spec word equal merge_grows_np's, the planes and
    the aggregate spec word are zero"""
    from manticoresearch_amd import dist
    from test_gpu_group import C64, Q

    m = corpus.m
    q = Q(m, "and2", C64, K=20, by=ge.GROUPSORT_COUNT)
    q.aggrs, q.aggr_order = None, -1
    mt = corpus.matches(orc, q)
    arows = amc.shard_arows_np(q, mt, CUTS[3])
    grows = gmc.shard_rows_np(q, mt[:3], CUTS[3])
    rng = np.random.default_rng(8)
    rel_a, rel_g = [], []
    for s, n in enumerate((3, 1024, 700)):
        rowid, weight = rng.choice(100000, n, replace=False) + s * 100000, rng.integers(1, 50, n)
        o = np.argsort(gmc.make_keys(weight, rowid))[::-1]
        rel_a.append(amc.arow_of_relevance(rowid[o], weight[o], n + 17)), rel_g.append(gmc.grow_of_relevance(rowid[o], weight[o], n + 17))
    A2, G2 = np.stack([arows, np.stack(rel_a)], axis=1), np.stack([grows, np.stack(rel_g)], axis=1)
    for k in (20, 1024):
        ma, mg = dist.merge_arows_np(A2, k), dist.merge_grows_np(G2, k)
        assert np.array_equal(ma[:, :amc.AGGR], mg[:, :gmc.SPEC]) and np.array_equal(ma[:, amc.GSPEC], mg[:, gmc.SPEC])
        assert not ma[:, amc.AGGR:amc.GSPEC].any() and not ma[:, amc.ASPEC].any()
    assert not amc.check_merged(dist, q, mt, dist.merge_arows_np(A2, 1024)[0], "no aggregates", True)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_merge_restated_over_the_shared_functions_under_sanitizers(tmp_path):
    exe = str(tmp_path / "aggr_merge")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "cpp", "aggr_merge.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.startswith("ok aggr merge specs 1134 merges "), out.stdout
