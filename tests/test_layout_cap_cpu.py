"""CPU: the cap on a block-scan work item's length (LayoutKnobs::p2_max_blocks, set by mrk_batch_submit for launches on the lean
block-scan instance; mrk::layout_batch in csrc/mrk_plan.cpp) under AddressSanitizer + UBSan.  tests/cpp/layout_cap.cpp lays the
seeded batches of the layout test out with the cap at 0, 4, 8 and 16 and checks the piece lengths, the cover of every pass's
block range, the piece counts written back to the passes and that the window-range sections do not move."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_capped_block_items(tmp_path):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "layout_cap.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "layout_cap")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    n = 60
    out = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    last = out.stdout.strip().split("\n")[-1].split()
    assert last[0] == "ok", out.stdout[-500:]
    layouts, pieces, cut_finer = (int(x) for x in last[2::2])
    # (every batch under 2 orders x 2 groupings x 3 pk_min_items x 3 caps; the cap adds items wherever the batch has block items
    # and pk_min_items has not already cut them to one block per wave: well over a quarter of the layouts)
    assert layouts == n * 36 and pieces > 100 * layouts and cut_finer > layouts // 4, last
