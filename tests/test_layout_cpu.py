"""CPU: the launch layout of a planned batch (mrk::layout_batch in csrc/mrk_plan.cpp, host code: how block ranges and window
ranges are cut and ordered, the scan_bm groups, the match queues' sizes) under AddressSanitizer + UBSan.  tests/cpp/layout.cpp
lays seeded random batches out under every item_order, bm_group and pk_min_items setting and checks what holds by construction;
its per-batch digests must equal tests/golden/layout_digests.json, recorded from the code as mrk_batch_submit held it before the
cutting loops were unified: the item array is element for element the same."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_layout_properties_and_digests(tmp_path):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "layout.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "layout")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    with open(os.path.join(HERE, "golden", "layout_digests.json")) as f:
        want = json.load(f)["digests"]
    out = subprocess.run([exe, str(len(want))], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    lines = out.stdout.split("\n")
    got = [ln.split() for ln in lines if ln and not ln.startswith("ok")]
    assert [int(i) for i, _ in got] == list(range(len(want)))
    differ = [int(i) for (i, d), w in zip(got, want) if d != w]
    assert not differ, f"batches laid out differently than recorded: {differ}"
    layouts, items, groups = (int(x) for x in lines[-2].split()[2::2])
    assert layouts == len(want) * 192 and items > 1000 * layouts and groups > layouts, lines[-2]
