"""CPU: aggregates of a grouped query (SUM / MIN / MAX of an integer attribute) on the host.

  - the numpy model every GPU test of aggregates compares against (group_aggr_expect) on what the REFERENCE recorded for its own
    grouping sorter (tests/golden/group_aggr_vectors.json: test_153's `select gr, sum(tag) ... group by gr` and test_171's MIN / MAX /
    SUM statements over the index dist_no), and on the typing rules the recorded cases do not reach (a 32-bit sum that wraps, its
    widened twin, signed 64-bit sources at their extremes, the order by an aggregate with ties);
  - the table's accumulators -- csrc/mrk_kgroup.h, the functions the kernels call, under a sequential policy -- in a stand-alone
    program under AddressSanitizer + UBSan (tests/cpp/group_aggr.cpp);
  - the planner's aggregate stage in another (tests/cpp/group_aggr_plan.cpp, linked with csrc/mrk_plan.cpp);
  - the ctypes mirrors and the marshalling of Query.aggrs into the third parallel pointer array of mrk_batch_submit_aggr."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import group_aggr_expect as gae
import group_expect as ge
from test_group_cpu import HIPCC, build

HERE = os.path.dirname(os.path.abspath(__file__))


class A:  # an aggregate as the model reads it (api.Aggr's fields)
    def __init__(self, func, kind=gae.KIND_INT, widen=False):
        self.func, self.kind, self.widen = func, kind, widen


def test_model_on_the_reference_recorded_aggregates():
    with open(os.path.join(HERE, "golden", "group_aggr_vectors.json")) as fp:
        v = json.load(fp)
    funcs = {"sum": gae.AGGR_SUM, "min": gae.AGGR_MIN, "max": gae.AGGR_MAX}
    by = {"key": ge.GROUPSORT_KEY, "count": ge.GROUPSORT_COUNT, "weight": ge.GROUPSORT_WEIGHT}
    assert len(v["cases"]) == 4 and sorted(c["func"] for c in v["cases"]) == ["max", "min", "sum", "sum"]
    for c in v["cases"]:
        rows = np.array(c["rows"], np.int64)
        out = gae.expected_group_aggrs(rows[:, 0], rows[:, 1], rows[:, 2], [rows[:, 3].astype(np.uint64)], [A(funcs[c["func"]])], -1, by[c["sort_by"]], c["desc"], v["max_matches"])
        r, w, k, cnt, total, ag = out
        assert total == len(c["groups"]) and ag.shape == (len(c["groups"]), 1) and ag.dtype == np.uint64
        for i, (hid, key, count, value) in enumerate(c["groups"]):
            assert int(k[i]) == key and int(ag[i, 0]) == value, (c["statement"], i)
            assert hid is None or int(r[i]) == hid
            assert count is None or int(cnt[i]) == count


def test_model_typing_rules_and_order():
    rowid = np.arange(12, dtype=np.uint32)
    weight = np.ones(12, np.int32)
    value = (rowid % 3).astype(np.uint32)  # three groups of four
    big = np.full(12, 0xF0000000, np.uint64)
    i64 = np.array([-5, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 7, 0, -1, 9, 1, 2, -9, 3, 4], np.int64)
    aggrs = [A(gae.AGGR_SUM), A(gae.AGGR_SUM, widen=True), A(gae.AGGR_SUM, gae.KIND_INT64), A(gae.AGGR_MIN, gae.KIND_INT64)]
    r, w, k, cnt, total, ag = gae.expected_group_aggrs(rowid, weight, value, [big, big, i64, i64], aggrs, -1, ge.GROUPSORT_KEY, False, 10)
    assert k.tolist() == [0, 1, 2] and cnt.tolist() == [4, 4, 4]
    assert ag[:, 0].tolist() == [(4 * 0xF0000000) & 0xFFFFFFFF] * 3 == [0xC0000000] * 3  # wraps modulo 2^32
    assert ag[:, 1].tolist() == [4 * 0xF0000000] * 3 and 4 * 0xF0000000 > 1 << 32         # the widened sum passes 2^32
    assert ag[0, 2] == (-5 + 7 + 9 - 9) & gae.M64 and ag[1, 2] == (np.iinfo(np.int64).min + 0 + 1 + 3) & gae.M64  # two's complement
    assert ag[1, 3] == 1 << 63 and ag[2, 3] == (-1) & gae.M64 and ag[0, 3] == (-9) & gae.M64  # signed MIN, the integer's bits
    mx = gae.expected_group_aggrs(rowid, weight, value, [i64], [A(gae.AGGR_MAX, gae.KIND_INT64)], -1, ge.GROUPSORT_KEY, False, 10)[5]
    assert mx[:, 0].tolist() == [9, 3, (1 << 63) - 1]
    # unsigned MIN / MAX of a 32-bit source: 0xFFFFFFFF is the largest value, not -1
    u = np.array([0xFFFFFFFF, 0, 5] * 4, np.uint64)
    mm = gae.expected_group_aggrs(rowid, weight, np.zeros(12, np.uint32), [u, u], [A(gae.AGGR_MIN), A(gae.AGGR_MAX)], -1, ge.GROUPSORT_KEY, True, 10)[5]
    assert mm.tolist() == [[0, 0xFFFFFFFF]]
    # the order by an aggregate: its value in Group.desc's direction, ties to the head's rowid ascending whatever the direction; the cut at K
    src = np.array([5, 7, 5, 1] * 3, np.uint64)
    val4 = (rowid % 4).astype(np.uint32)  # sums 15, 21, 15, 3; heads 0, 1, 2, 3
    for desc, keys in ((True, [1, 0, 2, 3]), (False, [3, 0, 2, 1])):
        r, w, k, cnt, total, ag = gae.expected_group_aggrs(rowid, weight, val4, [src], [A(gae.AGGR_SUM)], 0, ge.GROUPSORT_KEY, desc, 10)
        assert k.tolist() == keys and ag[:, 0].tolist() == [[15, 21, 15, 3][x] for x in keys] and total == 4
        r2 = gae.expected_group_aggrs(rowid, weight, val4, [src], [A(gae.AGGR_SUM)], 0, ge.GROUPSORT_KEY, desc, 2)
        assert r2[2].tolist() == keys[:2] and r2[4] == 4
    # the limit is the group's: 4 K distinct keys answer, one more declines
    assert gae.expected_group_aggrs(rowid, weight, rowid % 5, [src], [A(gae.AGGR_SUM)], -1, ge.GROUPSORT_KEY, True, 1) is ge.DECLINED
    assert gae.expected_group_aggrs(rowid, weight, val4, [src], [A(gae.AGGR_SUM)], 0, ge.GROUPSORT_KEY, True, 1) is not ge.DECLINED


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_accumulators_under_sanitizers(tmp_path):
    out = subprocess.run([build(tmp_path, "group_aggr", False)], capture_output=True, text=True, timeout=600)
    # 6 aggregate lists x 4 value classes x 3 ways of combining x 4 table shapes
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok runs %d" % (6 * 4 * 3 * 4)), (out.stdout[-3000:], out.stderr[-3000:])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_planner_aggregate_stage_under_sanitizers(tmp_path):
    out = subprocess.run([build(tmp_path, "group_aggr_plan", True)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    # 6 query shapes x 3 K x 18 accepted specs; every MRK_E_INVAL and MRK_E_UNSUPPORTED of include/mrk.h
    assert out.stdout.startswith("ok accepted %d inval 26 unsupported 9" % (6 * 3 * 18)), out.stdout


def test_ctypes_mirrors_and_marshalling():
    import manticoresearch_amd as m
    from manticoresearch_amd import _lib
    from manticoresearch_amd.api import _CQueries

    # the structs beside the query keep their sizes: the aggregates travel in a third parallel array
    P = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.Group) == 16
    assert C.sizeof(_lib.Result) == _lib.Result.group_count.offset + P and _lib.Result.group_count.offset == _lib.Result.order_key.offset + 2 * P
    assert not hasattr(_lib.Query, "aggrs") and not hasattr(_lib.Group, "aggrs")
    assert C.sizeof(_lib.Aggr) == 20 and [f.offset for f in (_lib.Aggr.func, _lib.Aggr.kind, _lib.Aggr.bit_offset, _lib.Aggr.bit_count, _lib.Aggr.flags)] == [0, 4, 8, 12, 16]
    assert C.sizeof(_lib.Aggrs) == 8 + 4 * 20 and (_lib.Aggrs.n.offset, _lib.Aggrs.order_by.offset, _lib.Aggrs.a.offset) == (0, 4, 8)
    assert (m.AGGR_SUM, m.AGGR_MIN, m.AGGR_MAX, m.MAX_AGGRS, _lib.AGGR_WIDEN) == (1, 2, 3, 4, 1)

    kw = m.XQNode.keyword
    G = m.Group(64, 32)
    none = [m.Query(kw(0, 1)), m.Query(kw(1, 1), group=G), m.Query(kw(2, 1), sort=m.Sort(0, 32))]
    some = none + [m.Query(kw(0, 1), group=m.Group(35, 5), aggrs=[m.Aggr(m.AGGR_SUM, 96, 32), m.Aggr(m.AGGR_MIN, 128, 64, kind=m.SORTKEY_INT64), m.Aggr(m.AGGR_MAX, 41, 7, widen=True)], aggr_order=0)]
    every = [m.Query(kw(0, 1), group=G, aggrs=[m.Aggr(m.AGGR_MAX, 0, 32)]), m.Query(kw(1, 1), group=G, aggrs=[m.Aggr(m.AGGR_SUM, 32, 1, widen=True)] * 4)]
    cq = _CQueries(none)
    assert cq.aggrs is None and cq.groups is not None  # no aggregates: mrk_batch_submit_grouped as before
    assert _CQueries(none[:1]).aggrs is None and _CQueries(none[:1]).groups is None
    cq = _CQueries(some)
    assert cq.aggrs is not None and len(cq.aggrs) == 4 and len(cq.groups) == 4
    assert not cq.aggrs[0] and not cq.aggrs[1] and not cq.aggrs[2] and cq.groups[1] and cq.groups[3] and not cq.groups[0]
    a = cq.aggrs[3].contents
    assert (a.n, a.order_by) == (3, 0)
    assert [(x.func, x.kind, x.bit_offset, x.bit_count, x.flags) for x in a.a[:3]] == [(1, 0, 96, 32, 0), (2, 2, 128, 64, 0), (3, 0, 41, 7, 1)]
    assert (a.a[3].func, a.a[3].bit_count) == (0, 0)
    cq = _CQueries(every)
    assert cq.aggrs[0] and cq.aggrs[1] and cq.aggrs[0].contents.order_by == -1 and cq.aggrs[1].contents.n == 4
    assert [x.flags for x in cq.aggrs[1].contents.a] == [1] * 4
    # aggregates without a group reach the library (which refuses them): the group array stands, all NULL
    cq = _CQueries([m.Query(kw(0, 1), aggrs=[m.Aggr(m.AGGR_SUM, 0, 32)])])
    assert cq.aggrs[0] and cq.groups is not None and not cq.groups[0]
    # more than MAX_AGGRS: n says so
    assert _CQueries([m.Query(kw(0, 1), group=G, aggrs=[m.Aggr(m.AGGR_SUM, 0, 32)] * 5)]).aggrs[0].contents.n == 5
    assert m.Matches(np.zeros(0, np.uint32), np.zeros(0, np.int32), 0).aggr is None
    lib = _lib.lib()
    assert lib.mrk_batch_submit_aggr.argtypes[4] == C.POINTER(C.POINTER(_lib.Aggrs)) and lib.mrk_batch_submit_aggr.argtypes[3] == C.POINTER(C.POINTER(_lib.Group))
    assert lib.mrk_batch_result_aggrs.argtypes[2] == C.POINTER(C.POINTER(C.c_uint64))
