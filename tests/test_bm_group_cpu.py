"""CPU: the planner's grouping of a batch's scan_bm queries for the grouped bitmap kernel (mrk::plan_bm_groups in
csrc/mrk_plan.cpp, host code) under AddressSanitizer + UBSan: every query in exactly one group, at most four per group, one
class and one shared keyword per group, lone queries on the ungrouped layout, deterministic (tests/cpp/bm_group.cpp)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_bm_grouping(tmp_path):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "bm_group.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "bm_group")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    out = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    groups, members, singles, full = (int(x) for x in out.stdout.split()[1::2])
    assert members > groups > 0 and singles > 0 and full > 0, out.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_bm_grouping_cost(tmp_path):
    """The grouping runs on every submit: a bench-sized batch (256 queries, 145 keywords) must plan in well under the submit's
    own time (about 0.1 ms per call was the quadratic first version; the holder lists take a few microseconds)."""
    exe = str(tmp_path / "bm_group_o2")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"),
                           os.path.join(HERE, "cpp", "bm_group.cpp"), "-o", exe])
    out = subprocess.run([exe, "time"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    f = out.stdout.split()
    us = float(f[1])
    print(out.stdout)
    assert int(f[9]) > 0  # groups of four formed
    assert us < 200.0, out.stdout  # (loose: shared build machines; the quadratic version took ~110 us at -O3)
