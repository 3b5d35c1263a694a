"""CPU: the host half of segments with 9-32 fields under AddressSanitizer + UBSan (tests/cpp/wide_fields.cpp): the wide packed
layout gives back every doclist entry's field mask, tf and rowid in both hit formats (and the narrow layout still declines such a
doclist), the planner's closed-form weight bounds equal a walk over every mask for up to 16 fields, and planning on a 32-field
segment accepts and declines what it does on an 8-field twin, without the bitmap kernels, and trips no sanitizer."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_wide_fields_host_side_under_sanitizers(tmp_path):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    csrc = os.path.join(ROOT, "manticoresearch_amd", "csrc")
    objs = []
    for src in (os.path.join(csrc, "mrk_plan.cpp"), os.path.join(csrc, "mrk_pack.cpp"), os.path.join(HERE, "cpp", "wide_fields.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "wide_fields")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    for seed in ("21", "22"):
        out = subprocess.run([exe, "3000", seed], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
        ok, uns, fails = (int(x) for x in out.stdout.split()[1::2])
        assert fails == 0 and ok > 5000, out.stdout
