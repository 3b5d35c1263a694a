"""CPU: one doc of a packed block read on its own (mrk::pk_doc_off / mrk::pk_lower_bound in csrc/mrk_kpk.h, the host-and-device
helpers behind the lean block scan's per-lane probe of a sparse second keyword) under AddressSanitizer + UBSan.
tests/cpp/pk_probe.cpp packs doclists with mrk::pack_term for every width 0 .. 16 and PK_WIDE and block sizes 1 .. 128 and checks
every doc's offset and the lower bound for every rowid around the block against the plain decode."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_doc_offset_and_lower_bound_of_every_width(tmp_path):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_pack.cpp"), os.path.join(HERE, "cpp", "pk_probe.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "pk_probe")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    last = out.stdout.strip().split("\n")[-1].split()
    assert last[0] == "ok", out.stdout[-500:]
    widths, cases, blocks, probes = (int(x) for x in last[1::2])
    # (widths 8 .. 16 and PK_WIDE hold every block size: 7 sizes x 2 last offsets x alone / behind a full block)
    assert widths == 18 and cases >= 10 * 28 and blocks > cases and probes > 8 * blocks, last
