"""CPU: the dispatch order of a batch's scan_bm work items (mrk::place_bm_items in csrc/mrk_plan.cpp, host code; ctx key
bm_place) under AddressSanitizer + UBSan.  tests/cpp/bm_place.cpp lays batches out with mrk::layout_batch, places them under
every mode and both bm_group settings and checks: a permutation; the identity for mode 0 and for fewer than two owners; the same
output twice; ascending windows inside a class; every item in a slot of its owner's class except where that class has run out;
the keyword figures against a count of its own; the classes' bytes never above the owners'.  Its inputs are seeded random
batches and the benchmark's own dense x dense query sets (bench.make_queries, a keyword's docs = its probability x 100 M), on
which at most 8 % of the items may sit outside their class's slots and the classes must hold at most 0.75 of the owners' bytes."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
DOCS = 100_000_000
SRCS = (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "bm_place.cpp"))


def write_bench_sets(path):
    """The cc stratum of the benchmark's query file, set by set: keyword ids and doc counts."""
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    c = bench.zipf_c()
    n_sets = (bench.QUERY_FILE // 3) // 256
    ranks, strata = bench.make_queries(c, n_sets * 256)
    docs = [int(min(0.5, c / r) * DOCS) for r in ranks]
    with open(path, "w") as f:
        f.write(f"nwin {(DOCS + 2047) // 2048}\n")
        for s in range(n_sets):
            f.write("set 256\n")
            for a, b in strata["cc"][s * 256:(s + 1) * 256]:
                f.write(f"{a} {docs[a]} {b} {docs[b]}\n")
    return n_sets


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_bm_placement(tmp_path):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    objs = []
    for src in SRCS:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "bm_place")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    sets = str(tmp_path / "sets.txt")
    n_sets = write_bench_sets(sets)
    assert n_sets == 13
    out = subprocess.run([exe, sets, "200"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    print(out.stdout)
    lines = out.stdout.strip().split("\n")
    assert sum(ln.startswith("set") for ln in lines) == 2 * n_sets  # 256 and 128 windows per item (each passed its two bounds inside the program)
    placements, items, tail, saved = (int(x) for x in lines[-1].split()[2::2])
    assert placements > 1000 and items > 100 * placements and saved > placements // 2 and tail < items // 10, lines[-1]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_bm_placement_cost_report(tmp_path):
    """The placement runs on every submit of a large launch.  Prints what a call costs on the benchmark's sets (about 50 000 work
    items, 90 owners, 150 keywords) next to layout_batch's own time; a figure to read, not a bound: build machines are shared."""
    exe = str(tmp_path / "bm_place_o2")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2"] + list(SRCS) + ["-o", exe])
    sets = str(tmp_path / "sets.txt")
    write_bench_sets(sets)
    out = subprocess.run([exe, sets, "time"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    assert out.stdout.startswith("us_per_call") and int(out.stdout.split()[-1]) > 40_000  # the launch is the benchmark's size
