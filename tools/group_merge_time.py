#!/usr/bin/env python3
"""tools/group_merge_time.py [--lists L] [--queries N] [--reps R] [--out FILE] -- one merge call of GROUP rows (mrk_topk_merge_grows),
L lists x N queries, timed next to mrk_topk_merge_orows over the same lists and queries, the nearest existing merge:
    grows K = 20      every list holds 60 of the query's 80 group values (the merged row holds all 80 = 4 K)
    grows K = 1024    every list holds the same 4096 values: 4096 groups per list, the full-size table and sort
    orows ordered     order rows, every list full (1000 entries) under a two-part 64-bit key
Per leg: warm-up calls, then R synchronous calls timed one by one (wall clock around the call, which clears the tables, launches the
kernel and waits for it) -> median, min, max in ms.  The group legs' results are checked against dist.merge_grows_np in the same run."""
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
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
Lh, N, K1 = args.lists, args.queries, 1024
hip = C.CDLL("libamdhip64.so")
ctx = m.Context(0)
lib = _lib.lib()
rng = np.random.default_rng(7)


def dmalloc(n):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
    return p


def grows_of(K, pool, per_list):
    """[Lh][N][GROW_WORDS]: every list holds per_list of the query's `pool` group values, in group order (@count descending)"""
    rows = np.zeros((Lh, N, dist.GROW_WORDS), np.uint64)
    spec = dist.group_spec_word(1, True, 32, K)
    for q in range(N):
        values = (rng.permutation(pool).astype(np.uint64) * np.uint64(0x9E3779B1) + np.uint64(q)) & np.uint64(0xFFFFFFFF)
        for l in range(Lh):
            v = values[rng.permutation(pool)[:per_list]] if per_list < pool else values
            cnt = rng.integers(1, 1000, per_list).astype(np.uint64)
            rowid = (rng.permutation(1 << 20)[:per_list].astype(np.uint64) + np.uint64(l << 20))
            head = ((rng.integers(1000, 1400, per_list).astype(np.uint64) ^ np.uint64(0x80000000)) << np.uint64(32)) | (~rowid & np.uint64(0xFFFFFFFF))
            o = np.argsort(dist.group_order_keys(1, 1, v.astype(np.uint32), cnt.astype(np.uint32), head))[::-1]
            rows[l, q, :per_list] = head[o]
            rows[l, q, dist.GROW_PLANE:dist.GROW_PLANE + per_list] = (v[o] << np.uint64(32)) | cnt[o]
            rows[l, q, dist.GROW_CNT] = rows[l, q, dist.GROW_TOTAL] = per_list
            rows[l, q, dist.GROW_SPEC] = spec
    return rows


def orows_of(K):
    rows = np.zeros((Lh, N, dist.OROW_WORDS), np.uint64)
    parts = [m.OrderPart(0, 2, desc=True), m.OrderPart(32, 4, desc=False)]
    for q in range(N):
        docid = rng.permutation(Lh * K).astype(np.uint64).reshape(Lh, K) + np.uint64(q)
        weight = rng.integers(1000, 1400, (Lh, K)).astype(np.uint64)
        keys = ((weight ^ np.uint64(0x80000000)) << np.uint64(32)) | (~docid & np.uint64(0xFFFFFFFF))
        mk = (rng.integers(0, 4, (Lh, K)).astype(np.uint64) << np.uint64(32)) | (~rng.integers(0, 16, (Lh, K)).astype(np.uint64) & np.uint64(0xFFFFFFFF))
        for l in range(Lh):
            o = np.lexsort((keys[l], mk[l]))[::-1]
            rows[l, q, :K], rows[l, q, K1], rows[l, q, K1 + 1] = keys[l][o], K, 100_000 + l
            rows[l, q, dist.OROW_MKEYS:dist.OROW_MKEYS + K] = mk[l][o]
            rows[l, q, dist.OROW_SPEC] = dist.order_spec_word(parts, 1)
    return rows


def leg(name, fn, rows, k, verify):
    words = rows.shape[2]
    src, dst = dmalloc(rows.nbytes), dmalloc(N * words * 8)
    assert hip.hipMemcpy(src, C.c_void_p(rows.ctypes.data), C.c_size_t(rows.nbytes), 1) == 0
    for _ in range(args.warmup):
        _lib.check(fn(ctx._h, src, Lh, N, k, dst))
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        _lib.check(fn(ctx._h, src, Lh, N, k, dst))
        ms.append((time.perf_counter() - t0) * 1e3)
    got = np.zeros((N, words), np.uint64)
    assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), dst, C.c_size_t(got.nbytes), 2) == 0
    nv = min(N, 16)  # (the mirror is slow at 32768 entries a query: the first queries stand for the rest)
    assert np.array_equal(got[:nv], verify(rows[:, :nv], k)), name
    hip.hipFree(src), hip.hipFree(dst)
    out = {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": args.reps, "bytes_in": int(rows.nbytes),
           "entries_out": int(got[0, dist.GROW_CNT if words == dist.GROW_WORDS else K1])}
    print(f"{name:44s} {out['ms_median']:8.3f} ms  [{out['ms_min']:.3f} .. {out['ms_max']:.3f}]  {out['entries_out']} entries a row", flush=True)
    return out


result = {"lists": Lh, "queries": N, "legs": {}}
result["legs"]["grows K=20"] = leg("mrk_topk_merge_grows, K = 20, 60 of 80 groups", lib.mrk_topk_merge_grows, grows_of(20, 80, 60), 20, dist.merge_grows_np)
result["legs"]["grows K=1024"] = leg("mrk_topk_merge_grows, K = 1024, 4096 groups", lib.mrk_topk_merge_grows, grows_of(1024, 4096, 4096), 1024, dist.merge_grows_np)
result["legs"]["orows ordered"] = leg("mrk_topk_merge_orows, all ordered, K = 1000", lib.mrk_topk_merge_orows, orows_of(1000), 1000, dist.merge_orows_np)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
ctx.close()
