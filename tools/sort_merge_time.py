#!/usr/bin/env python3
"""tools/sort_merge_time.py [--lists L] [--queries N] [--k K] [--reps R] [--out FILE] -- the shard merges on their own: synthetic
sorted rows of L shards x N queries (every list full, K entries), merged by mrk_topk_merge_rows (narrow rows) and by
mrk_topk_merge_srows (wide rows), all-relevance and all-sorted.  Per leg: warm-up launches, then R synchronous calls timed one by
one (wall clock around the call, which launches the kernel and waits for it) -> median, min, max in ms, and the ratio to the
narrow merge.  The wide legs' results are checked against dist.merge_srows_np once.  Run on a checkout without wide rows it times
the narrow merge only (the figures of the commit before)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manticoresearch_amd as m  # noqa: E402
from manticoresearch_amd import _lib, dist  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lists", type=int, default=8)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--k", type=int, default=1000)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
Lh, N, K, K1 = args.lists, args.queries, args.k, 1024
has_wide = hasattr(dist, "SROW_WORDS")
hip = C.CDLL("libamdhip64.so")
ctx = m.Context(0)
lib = _lib.lib()
rng = np.random.default_rng(7)


def dmalloc(n):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
    return p


def rows_of(words, sorted_rows):
    """[Lh][N][words] rows: K entries per list, in the merge's order; docids are distinct over the lists of a query."""
    rows = np.zeros((Lh, N, words), np.uint64)
    for q in range(N):
        docid = rng.permutation(Lh * K).astype(np.uint64).reshape(Lh, K) + np.uint64(q)
        weight = rng.integers(1000, 1400, (Lh, K)).astype(np.uint64)  # few distinct weights: ties down to the docid, as BM25 gives
        keys = ((weight ^ np.uint64(0x80000000)) << np.uint64(32)) | (~docid & np.uint64(0xFFFFFFFF))
        mk = rng.integers(0, 4, (Lh, K)).astype(np.uint32) if sorted_rows else np.zeros((Lh, K), np.uint32)  # a 4-valued column
        for l in range(Lh):
            order = np.lexsort((keys[l], mk[l]))[::-1]
            rows[l, q, :K] = keys[l][order]
            rows[l, q, K1] = K
            rows[l, q, K1 + 1] = 100_000 + l
            if sorted_rows:
                plane = np.zeros(K1, "<u4")
                plane[:K] = mk[l][order]
                rows[l, q, dist.SROW_MKEYS:dist.SROW_SPEC] = plane.view("<u8")
                rows[l, q, dist.SROW_SPEC] = dist.sort_spec_word(0, True, 1, 2)
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
        assert np.array_equal(got, dist.merge_srows_np(rows, K)), name
    hip.hipFree(src), hip.hipFree(dst)
    out = {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": args.reps, "bytes_in": int(rows.nbytes)}
    print(f"{name:44s} {out['ms_median']:8.3f} ms  [{out['ms_min']:.3f} .. {out['ms_max']:.3f}]", flush=True)
    return out


result = {"lists": Lh, "queries": N, "k": K, "legs": {}}
result["legs"]["narrow"] = leg("mrk_topk_merge_rows", lib.mrk_topk_merge_rows, rows_of(K1 + 2, False), False)
if has_wide:
    result["legs"]["wide relevance"] = leg("mrk_topk_merge_srows, all relevance", lib.mrk_topk_merge_srows, rows_of(dist.SROW_WORDS, False), True)
    result["legs"]["wide sorted"] = leg("mrk_topk_merge_srows, all sorted", lib.mrk_topk_merge_srows, rows_of(dist.SROW_WORDS, True), True)
    for k_ in ("wide relevance", "wide sorted"):
        result["legs"][k_]["ratio_to_narrow"] = result["legs"][k_]["ms_median"] / result["legs"]["narrow"]["ms_median"]
        print(f"{k_}: {result['legs'][k_]['ratio_to_narrow']:.2f} x the narrow merge")
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
ctx.close()
