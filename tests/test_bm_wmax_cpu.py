"""CPU: the per-word tf-class plane behind the two-bitmap AND kernel's weight bound (ctx key bm_wmax), host code under
AddressSanitizer + UBSan (tests/cpp/bm_wmax.cpp, a stand-alone program).  The plane mrk::pack_term builds equals the per-word
maximum recomputed from the postings -- single postings of tf 14, 15, 254, 255 and 300, an empty word, the last partial window,
groups of four windows that end early, both hit formats -- and the per-class bound the kernel calls (mrk::bm_wmax_bound) is never
below mrk::term_tfidf for any tf in 1..300 of that class or a lower one, for positive, zero and negative idf."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "manticoresearch_amd", "csrc")
SRCS = (os.path.join(HERE, "cpp", "bm_wmax.cpp"), os.path.join(CSRC, "mrk_pack.cpp"), os.path.join(CSRC, "mrk_writer.cpp"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_plane_and_bound(tmp_path):
    # (the library's own arithmetic flags: no contraction; the host's fp32 divide is IEEE already)
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
             "-fno-sanitize-recover=undefined"]
    objs = []
    for src in SRCS:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "bm_wmax")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-lpthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    lines = out.stdout.split("\n")
    assert lines[0].startswith("bounds ") and int(lines[0].split()[1]) > 100_000 and lines[1] == "ok", out.stdout
