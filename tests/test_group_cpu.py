"""CPU: GROUP BY an integer attribute on the host.

  - the numpy model every grouped GPU test compares against (group_expect.expected_groups) on what the REFERENCE recorded for its own
    grouping sorter (tests/golden/group_vectors.json: test_020's full-scan GROUP BY tag under five groupsort clauses), and on its
    limit (4 * max_matches distinct keys answer, one more declines), ties and cuts;
  - the group table's hash, probe and claim -- csrc/mrk_kgroup.h, the functions the kernels call, under a sequential policy -- in a
    stand-alone program under AddressSanitizer + UBSan (tests/cpp/group_table.cpp), and the seeds it finds for the GPU test;
  - the planner's group stage in another (tests/cpp/group_plan.cpp, linked with csrc/mrk_plan.cpp);
  - the ctypes mirrors and the marshalling of Query.group into the parallel pointer array of mrk_batch_submit_grouped."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import group_expect as ge

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-gpu-sanitize"]
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g"] + SAN + ["-fno-sanitize-recover=undefined"]


def test_model_on_the_reference_recorded_groups():
    with open(os.path.join(HERE, "golden", "group_vectors.json")) as fp:
        v = json.load(fp)
    ids = np.array([r[0] for r in v["corpus"]["rows"]], np.uint32)
    tag = np.array([r[1] for r in v["corpus"]["rows"]], np.uint32)
    weight = np.ones(len(ids), np.int32)  # a full scan: every row matches with weight 1
    by = {"key": ge.GROUPSORT_KEY, "count": ge.GROUPSORT_COUNT, "weight": ge.GROUPSORT_WEIGHT}
    assert len(v["cases"]) == 5 and {c["groupsort"] for c in v["cases"]} == {"@group desc", "@group asc", "@count desc", "@count asc", "tag desc"}
    for c in v["cases"]:
        # rowids ascend with the ids (the indexer numbers rows in document order), so the id stands for the rowid
        r, w, k, cnt, total = ge.expected_groups(ids, weight, tag, by[c["sort_by"]], c["desc"], v["max_matches"])
        got = [[int(a), int(b), int(x), int(y)] for a, b, x, y in zip(r, w, k, cnt)]
        assert got == c["matches"] and total == c["total_found"], (c["groupsort"], got)


def test_model_limit_ties_and_cut():
    rng = np.random.default_rng(4)
    n = 5000
    rowid = rng.permutation(n).astype(np.uint32)
    weight = rng.integers(-3, 4, n).astype(np.int32)
    for K, card, declined in ((4, 16, False), (4, 17, True), (1, 4, False), (1, 5, True), (1024, 4096, False), (1024, 4097, True)):
        value = (rowid % card).astype(np.uint32) * np.uint32(0x9E3779B1)
        out = ge.expected_groups(rowid, weight, value, ge.GROUPSORT_COUNT, True, K)
        assert (out is ge.DECLINED) == declined, (K, card)
        if declined:
            continue
        r, w, k, cnt, total = out
        assert total == card and len(r) == min(K, card) and int(cnt.sum()) <= n
        for hr, hw, kv, c in zip(r, w, k, cnt):  # head = weight DESC, rowid ASC inside the group; count = its matches
            mine = value == kv
            best = weight[mine].max()
            assert c == mine.sum() and hw == best and hr == rowid[mine & (weight == best)].min()
    # ties in the part fall to the head's rowid ascending, whatever the direction
    value = np.array([5, 5, 9, 9, 1, 1], np.uint32)
    rowid = np.array([10, 11, 3, 4, 20, 21], np.uint32)
    weight = np.array([7, 7, 7, 7, 7, 7], np.int32)
    for by in (ge.GROUPSORT_COUNT, ge.GROUPSORT_WEIGHT):
        for desc in (True, False):
            r, w, k, cnt, total = ge.expected_groups(rowid, weight, value, by, desc, 2)
            assert r.tolist() == [3, 10] and k.tolist() == [9, 5] and cnt.tolist() == [2, 2] and total == 3
    r, w, k, cnt, total = ge.expected_groups(rowid, weight, value, ge.GROUPSORT_KEY, False, 10)
    assert k.tolist() == [1, 5, 9] and r.tolist() == [20, 10, 3]
    assert ge.expected_groups(rowid[:0], weight[:0], value[:0], ge.GROUPSORT_KEY, True, 3)[4] == 0


def build(tmp_path, name, with_planner):
    srcs = [os.path.join(HERE, "cpp", name + ".cpp")] + ([os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp")] if with_planner else [])
    objs = []
    for src in srcs:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + FLAGS + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / name)
    subprocess.check_call([HIPCC] + SAN + objs + ["-o", exe])
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_group_table_under_sanitizers_and_the_gpu_tests_seeds(tmp_path):
    out = subprocess.run([build(tmp_path, "group_table", False)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), (out.stdout[-3000:], out.stderr[-3000:])
    found = {int(k): (int(c), int(w)) for k, c, w in re.findall(r"SEED k=(\d+) collide=(\d+) wrap=(\d+)", out.stdout)}
    import test_gpu_group as tg

    named = {}
    for k, seed, what in tg.SEEDS.values():
        named.setdefault(k, {})[what] = seed
    assert found == {k: (d["collide"], d["wrap"]) for k, d in named.items()}, (found, named)
    # and the Python restatement of the generator agrees with the program's
    assert [ge.seeded_value(8, j) for j in range(3)] == [tg.make_rows(16)[j, tg.S1W] for j in range(3)]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_planner_group_stage_under_sanitizers(tmp_path):
    out = subprocess.run([build(tmp_path, "group_plan", True)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    # 6 query shapes x 6 K x 4 specs; 20 declines
    assert out.stdout.startswith("ok accepted %d declines 20" % (6 * 6 * 4)), out.stdout


def test_ctypes_mirrors_and_marshalling():
    import manticoresearch_amd as m
    from manticoresearch_amd import _lib
    from manticoresearch_amd.api import _CQueries

    assert C.sizeof(_lib.Group) == 16 and [(_lib.Group.bit_offset.offset, _lib.Group.bit_count.offset, _lib.Group.sort_by.offset, _lib.Group.desc.offset)] == [(0, 4, 8, 12)]
    P = C.sizeof(C.c_void_p)
    assert _lib.Result.group_key.offset == _lib.Result.order_key.offset + P and _lib.Result.group_count.offset == _lib.Result.group_key.offset + P
    assert C.sizeof(_lib.Result) == _lib.Result.group_count.offset + P
    assert (m.GROUPSORT_KEY, m.GROUPSORT_COUNT, m.GROUPSORT_WEIGHT) == (0, 1, 2)
    assert not hasattr(_lib.Query, "group"), "mrk_query does not grow: the group travels beside it"

    kw = m.XQNode.keyword
    qs = [m.Query(kw(0, 1)), m.Query(kw(1, 1), group=m.Group(35, 5, sort_by=m.GROUPSORT_COUNT, desc=False)), m.Query(kw(2, 1), sort=m.Sort(0, 32)),
          m.Query(kw(0, 1), group=m.Group(64, 32))]
    cq = _CQueries(qs)
    assert cq.groups is not None and len(cq.groups) == 4
    assert not cq.groups[0] and not cq.groups[2]
    g = cq.groups[1].contents
    assert (g.bit_offset, g.bit_count, g.sort_by, g.desc) == (35, 5, 1, 0)
    g = cq.groups[3].contents
    assert (g.bit_offset, g.bit_count, g.sort_by, g.desc) == (64, 32, 0, 1)
    assert _CQueries(qs[:1] + qs[2:3]).groups is None  # no grouped query: plain mrk_batch_submit
    assert m.Matches(np.zeros(0, np.uint32), np.zeros(0, np.int32), 0).group_key is None
    lib = _lib.lib()
    assert lib.mrk_batch_submit_grouped.argtypes[3] == C.POINTER(C.POINTER(_lib.Group))
