"""CPU: GROUP BY a multi-value attribute on the host.

  - the numpy model every GPU test of MVA groups compares against (group_mva_expect) on what the REFERENCE recorded for its own
    MVAGroupSorter_T (tests/golden/group_mva_vectors.json: test_020's `groupattr = mva` queries), and on what the recorded cases do
    not reach: duplicates, empty MVAs, the limit, the tie rule and the cut under it;
  - blob_mva_span, the expansion into the group table and the tie order as a comparator -- csrc/mrk_kgroup.h, the functions the kernels
    call -- in a stand-alone program under AddressSanitizer + UBSan (tests/cpp/group_mva.cpp), whose GROUP / ORDER lines the model is
    checked against;
  - the planner's stage in another (tests/cpp/group_mva_plan.cpp, linked with csrc/mrk_plan.cpp);
  - the ctypes mirror and the marshalling of Group's MVA fields into the fourth parallel pointer array of mrk_batch_submit_mva."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import group_expect as ge
import group_mva_expect as gme
from test_group_cpu import HIPCC, build

HERE = os.path.dirname(os.path.abspath(__file__))
BY = {"key": ge.GROUPSORT_KEY, "count": ge.GROUPSORT_COUNT, "weight": ge.GROUPSORT_WEIGHT}


def test_model_on_the_reference_recorded_mva_groups():
    with open(os.path.join(HERE, "golden", "group_mva_vectors.json")) as fp:
        v = json.load(fp)
    rows = v["corpus"]["rows"]
    ids = np.array([r[0] for r in rows], np.uint32)
    weight = np.full(len(ids), v["weight"], np.int64)  # 'test*' matched all ten rows at the one recorded weight
    mva = {r[0]: r[1] for r in rows}
    assert len(v["cases"]) == 2 and {c["groupsort"] for c in v["cases"]} == {"@group desc", "@group asc"}
    # (group 5 with @count 7 and group 6 with @count 2, as the reference recorded them)
    assert [5, 7] in [m[2:] for m in v["cases"][0]["matches"]] and [6, 2] in [m[2:] for m in v["cases"][0]["matches"]]
    for c in v["cases"]:
        assert all(m[1] == v["weight"] for m in c["matches"])  # one weight: the recorded heads are the groups' smallest ids
        # rowids ascend with the ids (the indexer numbers rows in document order), so the id stands for the rowid
        push = gme.expand(ids, weight, lambda r: mva[r])
        assert not gme.has_tie(*push, BY[c["sort_by"]], c["desc"])  # ordered by the key: no two groups tie
        r, w, k, cnt, total = gme.expected_groups_mva(*push, BY[c["sort_by"]], c["desc"], v["max_matches"])
        got = [[int(a), int(b), int(x), int(y)] for a, b, x, y in zip(r, w, k, cnt)]
        assert got == c["matches"] and total == c["total_found"], (c["groupsort"], got)


def test_model_pushes_limit_ties_and_cut():
    # doc 0: {7, 7, 3} (a value stored twice counts twice, stored order kept), doc 1: {}, doc 2: {3}, doc 3: {9, 3}
    mva = {0: [7, 7, 3], 1: [], 2: [3], 3: [9, 3]}
    rowid, weight = np.arange(4, dtype=np.uint32), np.array([10, 99, 30, 20], np.int64)
    push = gme.expand(rowid, weight, lambda r: mva[r])
    assert push[0].tolist() == [0, 0, 0, 2, 3, 3] and push[2].tolist() == [7, 7, 3, 3, 9, 3]  # the doc without values joins no group
    r, w, k, cnt, total = gme.expected_groups_mva(*push, ge.GROUPSORT_KEY, False, 10)
    assert (k.tolist(), cnt.tolist(), r.tolist(), w.tolist(), total) == ([3, 7, 9], [3, 2, 1], [2, 0, 3], [30, 10, 20], 3)
    # the limit counts distinct values over all pushes -- also when one doc alone carries them
    one = gme.expand([5], [1], lambda r: [1, 2, 3, 4, 5])
    assert gme.expected_groups_mva(*one, ge.GROUPSORT_KEY, True, 1) is ge.DECLINED
    assert gme.expected_groups_mva(*gme.expand([5], [1], lambda r: [1, 2, 3, 4, 4]), ge.GROUPSORT_KEY, True, 1) is not ge.DECLINED
    assert gme.expected_groups_mva(*gme.expand([], [], lambda r: []), ge.GROUPSORT_COUNT, True, 5)[4] == 0
    # ties: values 8 and 2 are carried by exactly the same docs -- equal under @count and under the head's weight in both directions;
    # the smaller value comes first whatever desc says, and it is the one that stays when K cuts between the two
    mva = {0: [8, 2], 1: [8, 2, 5], 2: [5]}
    push = gme.expand([0, 1, 2], [40, 50, 60], lambda r: mva[r])
    for by in (ge.GROUPSORT_COUNT, ge.GROUPSORT_WEIGHT):
        for desc in (True, False):
            assert gme.has_tie(*push, by, desc)
            k = gme.expected_groups_mva(*push, by, desc, 10)[2].tolist()
            assert k.index(2) + 1 == k.index(8), (by, desc, k)
    assert gme.expected_groups_mva(*push, ge.GROUPSORT_WEIGHT, False, 1)[2].tolist() == [2]  # heads: 5 -> 60, 2 and 8 -> 50
    assert gme.expected_groups_mva(*push, ge.GROUPSORT_WEIGHT, False, 2)[2].tolist() == [2, 8]
    assert gme.expected_groups_mva(*push, ge.GROUPSORT_COUNT, True, 2)[2].tolist() == [2, 8]  # counts 2, 2, 2; heads: rowid 1 twice, then 2
    assert not gme.has_tie(*push, ge.GROUPSORT_KEY, True)
    # a blob row read from the format's definition: attribute 1 of 2 behind a string, 2-byte lengths
    from helpers import build_blob_pool

    pool, offs = build_blob_pool([[b"x" * 300, np.array([9, 1, 9], "<u4").tobytes()], [b"", b""]])
    assert gme.mva_values(pool, offs[0], 1, 2).tolist() == [9, 1, 9] and gme.mva_values(pool, offs[1], 1, 2).tolist() == [] and pool[offs[0]] == 1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_span_expansion_and_tie_order_under_sanitizers(tmp_path):
    out = subprocess.run([build(tmp_path, "group_mva", False)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok spans 38 expansions 9"), (out.stdout[-3000:], out.stderr[-3000:])
    # the comparator's order of its groups == the model's order of pushes that form those groups (count pushes of the head's own doc)
    groups = [tuple(int(x) for x in g) for g in re.findall(r"GROUP (\d+) (\d+) (-?\d+) (\d+)", out.stdout)]
    orders = {(int(by), int(desc)): [int(x) for x in vals.split()] for by, desc, vals in re.findall(r"ORDER (\d) (\d)((?: \d+)+)", out.stdout)}
    assert len(groups) == 8 and len(orders) == 6
    rowid = np.concatenate([np.full(c, r, np.uint32) for v, c, w, r in groups])
    weight = np.concatenate([np.full(c, w, np.int64) for v, c, w, r in groups])
    value = np.concatenate([np.full(c, v, np.uint32) for v, c, w, r in groups])
    tied = 0
    for (by, desc), want in orders.items():
        r, w, k, cnt, total = gme.expected_groups_mva(rowid, weight, value, by, bool(desc), 100)
        assert k.tolist() == want and total == 8, (by, desc, k.tolist(), want)
        tied += gme.has_tie(rowid, weight, value, by, bool(desc))
    assert tied == 4  # @count and the weight tie in both directions, the key never does


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_planner_mva_stage_under_sanitizers(tmp_path):
    out = subprocess.run([build(tmp_path, "group_mva_plan", True)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    # 5 query shapes x 3 K x 3 group specs x 3 blob attributes; every MRK_E_INVAL and MRK_E_UNSUPPORTED of include/mrk.h
    assert out.stdout.startswith("ok accepted %d inval 15 unsupported 8" % (5 * 3 * 3 * 3)), out.stdout


def test_ctypes_mirror_and_marshalling():
    import manticoresearch_amd as m
    from manticoresearch_amd import _lib
    from manticoresearch_amd.api import _CQueries

    # the structs beside the query keep their sizes: the MVA travels in a fourth parallel array
    assert C.sizeof(_lib.Group) == 16 and not hasattr(_lib.Group, "mva_bits")
    assert C.sizeof(_lib.GroupMva) == 12 and [f.offset for f in (_lib.GroupMva.mva_bits, _lib.GroupMva.blob_attr_id, _lib.GroupMva.n_blob_attrs)] == [0, 4, 8]
    g = m.Group(64, 32)
    assert (g.mva_bits, g.blob_attr_id, g.n_blob_attrs) == (0, 0, 0) and (g.sort_by, g.desc) == (m.GROUPSORT_KEY, True)

    kw = m.XQNode.keyword
    M = m.Group(0, 0, sort_by=m.GROUPSORT_COUNT, desc=False, mva_bits=32, blob_attr_id=2, n_blob_attrs=3)
    plain = [m.Query(kw(0, 1)), m.Query(kw(1, 1), group=g), m.Query(kw(2, 1), group=g, aggrs=[m.Aggr(m.AGGR_SUM, 0, 32)])]
    # no MVA group: the arrays and the call every existing query is submitted by
    assert _CQueries(plain).mvas is None and _CQueries(plain[:1]).mvas is None and _CQueries(plain[:1]).groups is None and _CQueries(plain[:2]).aggrs is None
    cq = _CQueries(plain + [m.Query(kw(3, 1), group=M)])
    assert cq.mvas is not None and len(cq.mvas) == 4 and not cq.mvas[0] and not cq.mvas[1] and not cq.mvas[2] and cq.mvas[3]
    mv, cg = cq.mvas[3].contents, cq.groups[3].contents
    assert (mv.mva_bits, mv.blob_attr_id, mv.n_blob_attrs) == (32, 2, 3) and (cg.sort_by, cg.desc) == (m.GROUPSORT_COUNT, 0)
    assert cq.aggrs is not None and cq.aggrs[2] and not cq.aggrs[3] and cq.groups[1] and not cq.groups[0]
    alone = _CQueries([m.Query(kw(3, 1), group=M)])
    assert alone.mvas[0] and alone.aggrs is None and alone.groups[0]
    # a hostile width reaches the library (which refuses it)
    assert _CQueries([m.Query(kw(0, 1), group=m.Group(0, 0, mva_bits=16, n_blob_attrs=1))]).mvas[0].contents.mva_bits == 16
    lib = _lib.lib()
    at = lib.mrk_batch_submit_mva.argtypes
    assert len(at) == 7 and at[3] == C.POINTER(C.POINTER(_lib.Group)) and at[4] == C.POINTER(C.POINTER(_lib.Aggrs)) and at[5] == C.POINTER(C.POINTER(_lib.GroupMva)) and at[6] == C.c_uint32
