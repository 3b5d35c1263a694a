"""CPU: sorted queries (mrk_query.sort) on the host.  The order-preserving key map and the planner's answers are checked by a
host-only program under AddressSanitizer + UBSan (tests/cpp/sort_plan.cpp, built like the planner's fuzz target); the Python
marshalling of Query.sort is checked on the flattened C structs."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_sort_map_and_planner_under_sanitizers(tmp_path):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "sort_plan.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "sort_plan")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.startswith("ok accepted 80 "), out.stdout


def test_query_sort_round_trips_through_cqueries():
    import manticoresearch_amd as m
    from manticoresearch_amd import _lib
    from manticoresearch_amd.api import _CQueries

    kw = m.XQNode.keyword
    qs = [m.Query(kw(0, 1), ranker=m.SPH_RANK_BM25),
          m.Query(kw(1, 1), ranker=m.SPH_RANK_BM25, sort=m.Sort(0, 32)),
          m.Query(m.XQNode.AND(kw(0, 1), kw(1, 2)), sort=m.Sort(35, 5, desc=False, then_weight=2)),
          m.Query(kw(2, 1), sort=m.Sort(64, 32, desc=True, then_weight=0, kind=m.SORTKEY_FLOAT))]
    cq = _CQueries(qs)
    assert not cq.arr[0].sort  # NULL = by relevance, today's behaviour
    want = [(0, 0, 32, 1, 1), (0, 35, 5, 0, 2), (1, 64, 32, 1, 0)]
    for c, w in zip(list(cq.arr)[1:], want):
        s = c.sort.contents
        assert (s.kind, s.bit_offset, s.bit_count, s.desc, s.then_weight) == w
    # the struct is mrk_sort of include/mrk.h: five int32, appended to mrk_query behind the weight filters; sort_key behind status
    assert C.sizeof(_lib.Sort) == 20
    assert _lib.Query.sort.offset > _lib.Query.n_weight_filters.offset
    assert _lib.Result.sort_key.offset > _lib.Result.status.offset
    assert m.Matches(None, None, 0).sort_key is None
