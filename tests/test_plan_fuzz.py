"""CPU: the query planner (csrc/mrk_plan.cpp -- host code, no kernel in it) under AddressSanitizer + UBSan, fed flattened trees a
caller could hand to mrk_batch_submit: half of them well-formed (every operator, shared subtrees, filters, cutoffs), half hostile
(child indices out of range, cycles, unknown operators, keywords outside the dictionary, INT_MIN / INT_MAX arguments, NaN boosts,
impossible filter locators).  Every call must come back MRK_OK / MRK_E_UNSUPPORTED / MRK_E_INVAL, the passes and work items of an
accepted query must stay inside what the launch code indexes (tests/cpp/fuzz_plan.cpp), and neither sanitizer may fire.

The same generator also draws mrk_query.sort / mrk_query.order specs (well-formed and hostile), cutoff bounds and a share of
"typical" queries (1-4 keyword trees over the dense keywords with the common rankers: what reaches the bitmap-driven kernels).  In
digest mode the harness prints one FNV-1a digest per 1000 iterations over everything plan_query answered -- return code, message,
head pass, further passes, work items, evaluator programs, the BatchPlan's counters -- plus the accepted plans per class and the
digest of the segments' sort_ranges caches.  tests/golden/plan_digests.json holds those lines as recorded from plan_query while it
was one function of 770 lines, before it was split into stages: an -O2 build and this test's -O1 ASan + UBSan build printed the
same lines (nothing hashed is uninitialised; DevQuery, which has padding, is hashed member by member).  A plan that changes by one
byte, a message that changes by one letter or a check that moves in front of another fails the comparison."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_planner_under_sanitizers(tmp_path):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "fuzz_plan.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "fuzz_plan")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    for seed in ("11", "12"):
        out = subprocess.run([exe, "250000", seed], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
        ok, uns, inval = (int(x) for x in out.stdout.split()[1::2])
        assert ok + uns + inval == 250000 and ok > 10000 and uns > 10000 and inval > 10000, out.stdout

    with open(os.path.join(HERE, "golden", "plan_digests.json")) as f:
        want = json.load(f)
    assert len(want["digests"]) >= 500 and want["iters"] == 1000 * len(want["digests"])
    out = subprocess.run([exe, str(want["iters"]), str(want["seed"]), "digest"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    lines = out.stdout.split("\n")
    got = [ln.split()[1:] for ln in lines if ln.startswith("chunk ")]
    assert [int(i) for i, _ in got] == list(range(len(want["digests"])))
    differ = [int(i) for (i, d), w in zip(got, want["digests"]) if d != w]
    assert not differ, f"chunks planned differently than recorded: {differ[:20]} ({len(differ)} in all)"
    words = next(ln for ln in lines if ln.startswith("classes ")).split()[1:]
    classes = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    print(classes)
    assert len(classes) == 18 and all(n >= 200 for n in classes.values()), classes
    assert classes == want["classes"]
    assert next(ln for ln in lines if ln.startswith("sort_ranges ")).split()[1] == want["sort_ranges"]
    ok, uns, inval = (int(x) for x in lines[-2].split()[1::2])
    assert ok + uns + inval == want["iters"] and min(ok, uns, inval) > 10000 * (want["iters"] // 250000), lines[-2]
