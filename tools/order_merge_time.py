#!/usr/bin/env python3
"""tools/order_merge_time.py [--root DIR] [--lists L] [--queries N] [--k K] [--reps R] [--out FILE] -- tools/sort_merge_time.py with
the ORDER rows' legs: synthetic sorted rows of L shards x N queries (every list full, K entries), merged by mrk_topk_merge_rows
(narrow rows), mrk_topk_merge_srows (wide rows: all-relevance, all-sorted) and mrk_topk_merge_orows (order rows: all-relevance,
all-ordered by a two-part 64-bit key whose both dwords decide, all weight-first -- the weight descending in front of the same
two-part key, OSPEC_WFIRST: the "all ordered" leg's lists in the other order, one more dword compare per exchange).  Per leg: warm-up launches, then R synchronous calls timed one by
one (wall clock around the call, which launches the kernel and waits for it) -> median, min, max in ms, the ratio to the narrow
merge and the ratio of bytes read.  The wide and order legs' results are checked against dist.merge_srows_np / merge_orows_np in
the same run.  --root DIR imports the package from another checkout (the commit before, built side by side): the legs that
checkout lacks are left out.  --parent FILE (that run's --out) adds the guard of tools/timing_guard.py for the legs both runs hold:
the change's median inside the parent's [min - spread .. max + spread]."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manticoresearch_amd as m  # noqa: E402
from manticoresearch_amd import _lib, dist  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=ROOT)
ap.add_argument("--lists", type=int, default=8)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--k", type=int, default=1000)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
ap.add_argument("--parent", default="", help="this script's result file of the commit before: the guard of tools/timing_guard.py over the shared legs")
args = ap.parse_args()
Lh, N, K, K1 = args.lists, args.queries, args.k, 1024
has_wide, has_order, has_wfirst = hasattr(dist, "SROW_WORDS"), hasattr(dist, "OROW_WORDS"), hasattr(dist, "OSPEC_WFIRST")
hip = C.CDLL("libamdhip64.so")
ctx = m.Context(0)
lib = _lib.lib()
rng = np.random.default_rng(7)


def dmalloc(n):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
    return p


def rows_of(words, kind=None):
    """[Lh][N][words] rows: K entries per list, in the merge's order; docids are distinct over the lists of a query.  kind: None =
    relevance rows (any width); "sorted" = wide rows over a 4-valued 32-bit key; "ordered" = order rows over a two-part 64-bit key, a
    4-valued high dword | a 16-valued low one, so that both dwords decide; "wfirst" = the same keys behind the weight, descending."""
    rows = np.zeros((Lh, N, words), np.uint64)
    for q in range(N):
        docid = rng.permutation(Lh * K).astype(np.uint64).reshape(Lh, K) + np.uint64(q)
        weight = rng.integers(1000, 1400, (Lh, K)).astype(np.uint64)  # few distinct weights: ties down to the docid, as BM25 gives
        keys = ((weight ^ np.uint64(0x80000000)) << np.uint64(32)) | (~docid & np.uint64(0xFFFFFFFF))
        mk = rng.integers(0, 4, (Lh, K)).astype(np.uint64) if kind else np.zeros((Lh, K), np.uint64)
        if kind in ("ordered", "wfirst"):
            mk = (mk << np.uint64(32)) | (~rng.integers(0, 16, (Lh, K)).astype(np.uint64) & np.uint64(0xFFFFFFFF))
        for l in range(Lh):
            order = np.lexsort((keys[l].astype(np.uint32), mk[l], keys[l] >> np.uint64(32)) if kind == "wfirst" else (keys[l], mk[l]))[::-1]
            rows[l, q, :K] = keys[l][order]
            rows[l, q, K1] = K
            rows[l, q, K1 + 1] = 100_000 + l
            if kind == "sorted":
                plane = np.zeros(K1, "<u4")
                plane[:K] = mk[l][order].astype(np.uint32)
                rows[l, q, dist.SROW_MKEYS:dist.SROW_SPEC] = plane.view("<u8")
                rows[l, q, dist.SROW_SPEC] = dist.sort_spec_word(0, True, 1, 2)
            elif kind in ("ordered", "wfirst"):
                parts = [m.OrderPart(0, 2, desc=True), m.OrderPart(32, 4, desc=False)]
                rows[l, q, dist.OROW_MKEYS:dist.OROW_MKEYS + K] = mk[l][order]
                rows[l, q, dist.OROW_SPEC] = dist.order_spec_word(parts, 1) if kind == "ordered" else dist.order_spec_word(parts, 0, weight_first=1)
    return rows


def leg(name, fn, rows, verify):
    words = rows.shape[2]
    src, dst = dmalloc(rows.nbytes), dmalloc(N * words * 8)
    assert hip.hipMemcpy(src, C.c_void_p(rows.ctypes.data), C.c_size_t(rows.nbytes), 1) == 0
    for _ in range(args.warmup):
        _lib.check(fn(ctx._h, src, Lh, N, K, dst))
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        _lib.check(fn(ctx._h, src, Lh, N, K, dst))
        ms.append((time.perf_counter() - t0) * 1e3)
    if verify:
        got = np.zeros((N, words), np.uint64)
        assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), dst, C.c_size_t(got.nbytes), 2) == 0
        assert np.array_equal(got, verify(rows, K)), name
    hip.hipFree(src), hip.hipFree(dst)
    out = {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": args.reps, "bytes_in": int(rows.nbytes)}
    print(f"{name:44s} {out['ms_median']:8.3f} ms  [{out['ms_min']:.3f} .. {out['ms_max']:.3f}]", flush=True)
    return out


result = {"lists": Lh, "queries": N, "k": K, "legs": {}}
result["legs"]["narrow"] = leg("mrk_topk_merge_rows", lib.mrk_topk_merge_rows, rows_of(K1 + 2), None)
if has_wide:
    result["legs"]["wide relevance"] = leg("mrk_topk_merge_srows, all relevance", lib.mrk_topk_merge_srows, rows_of(dist.SROW_WORDS), dist.merge_srows_np)
    result["legs"]["wide sorted"] = leg("mrk_topk_merge_srows, all sorted", lib.mrk_topk_merge_srows, rows_of(dist.SROW_WORDS, "sorted"), dist.merge_srows_np)
if has_order:
    result["legs"]["order relevance"] = leg("mrk_topk_merge_orows, all relevance", lib.mrk_topk_merge_orows, rows_of(dist.OROW_WORDS), dist.merge_orows_np)
    result["legs"]["order ordered"] = leg("mrk_topk_merge_orows, all ordered", lib.mrk_topk_merge_orows, rows_of(dist.OROW_WORDS, "ordered"), dist.merge_orows_np)
if has_wfirst:
    result["legs"]["order weight-first"] = leg("mrk_topk_merge_orows, all weight-first", lib.mrk_topk_merge_orows, rows_of(dist.OROW_WORDS, "wfirst"), dist.merge_orows_np)
for k_, v in result["legs"].items():
    if k_ != "narrow":
        v["ratio_to_narrow"] = v["ms_median"] / result["legs"]["narrow"]["ms_median"]
        v["bytes_ratio_to_narrow"] = v["bytes_in"] / result["legs"]["narrow"]["bytes_in"]
        print(f"{k_}: {v['ratio_to_narrow']:.2f} x the narrow merge's time, {v['bytes_ratio_to_narrow']:.2f} x its bytes")
if args.parent:
    from timing_guard import guard, report

    result["guard"] = guard(json.load(open(args.parent))["legs"], result["legs"])
    result["guard_inside"] = report(result["guard"])
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
ctx.close()
