#!/usr/bin/env python3
"""tools/aggr_merge_time.py [--lists L] [--queries N] [--reps R] [--out FILE] -- ONE synchronous merge call of AGGREGATE rows
(mrk_topk_merge_arows), L lists x N queries, next to mrk_topk_merge_grows over the same groups in the same run:
    K = 20      every list holds 60 of the query's 80 group values (the merged row holds all 80 = 4 K)
    K = 1024    every list holds the same 4096 values: 4096 groups per list, the full-size table and sort
each with 0, 1 and 4 aggregates (SUM 32-bit; SUM widened, MIN, signed MAX, signed SUM).  Per leg: warm-up calls, then R synchronous
calls timed one by one (wall clock around the call, which clears the tables, launches the kernel and waits for it) -> median, min,
max in ms; results checked against dist.merge_arows_np / merge_grows_np in the same run.
The clear's share: the tool clears a buffer of its own of the call's arena size -- N tables of group_table_words(slots, 4) for
aggregate rows, (slots, 0) for group rows, rounded to 128-byte lines -- with hipMemsetAsync and waits, timestamps around it.
The export alone: mrk_batch_export_arows / _grows of N grouped queries over a 100 K-doc segment after mrk_batch_wait."""
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
Lh, N = args.lists, args.queries
G = dist.GROW_GROUPS
hip = C.CDLL("libamdhip64.so")
ctx = m.Context(0)
lib = _lib.lib()
rng = np.random.default_rng(7)


class A:  # what dist.aggr_spec_word reads of an aggregate
    def __init__(self, func, kind=0, widen=False):
        self.func, self.kind, self.widen = func, kind, widen


AGGRS = {0: [], 1: [A(m.AGGR_SUM)], 4: [A(m.AGGR_SUM, widen=True), A(m.AGGR_MIN), A(m.AGGR_MAX, kind=m.SORTKEY_INT64), A(m.AGGR_SUM, kind=m.SORTKEY_INT64)]}


def dmalloc(n):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
    return p


def rows_of(K, pool, per_list):
    """(grows [Lh][N][GROW_WORDS], {n: arows [Lh][N][AROW_WORDS]}): every list holds per_list of the query's `pool` group values in
    group order (@count descending); the same groups in every format, the aggregate planes random values of their kind"""
    grows = np.zeros((Lh, N, dist.GROW_WORDS), np.uint64)
    arows = {n: np.zeros((Lh, N, dist.AROW_WORDS), np.uint64) for n in AGGRS}
    spec = dist.group_spec_word(1, True, 32, K)
    for q in range(N):
        values = (rng.permutation(pool).astype(np.uint64) * np.uint64(0x9E3779B1) + np.uint64(q)) & np.uint64(0xFFFFFFFF)
        for l in range(Lh):
            v = values[rng.permutation(pool)[:per_list]] if per_list < pool else values
            cnt = rng.integers(1, 1000, per_list).astype(np.uint64)
            rowid = (rng.permutation(1 << 20)[:per_list].astype(np.uint64) + np.uint64(l << 20))
            head = ((rng.integers(1000, 1400, per_list).astype(np.uint64) ^ np.uint64(0x80000000)) << np.uint64(32)) | (~rowid & np.uint64(0xFFFFFFFF))
            o = np.argsort(dist.group_order_keys(1, 1, v.astype(np.uint32), cnt.astype(np.uint32), head))[::-1]
            row = grows[l, q]
            row[:per_list] = head[o]
            row[dist.GROW_PLANE:dist.GROW_PLANE + per_list] = (v[o] << np.uint64(32)) | cnt[o]
            row[dist.GROW_CNT] = row[dist.GROW_TOTAL] = per_list
            row[dist.GROW_SPEC] = spec
            for n, aggrs in AGGRS.items():
                ar = arows[n][l, q]
                ar[:dist.AROW_AGGR] = row[:dist.GROW_SPEC]
                ar[dist.AROW_GSPEC], ar[dist.AROW_ASPEC] = spec, dist.aggr_spec_word(aggrs)
                for a, g in enumerate(aggrs):
                    wide = g.widen or g.kind == m.SORTKEY_INT64
                    ar[dist.AROW_AGGR + a * G:dist.AROW_AGGR + a * G + per_list] = rng.integers(0, 1 << 63, per_list, dtype=np.uint64) * np.uint64(2) if wide else rng.integers(0, 1 << 32, per_list, dtype=np.uint64)
    return grows, arows


def timed(call):
    for _ in range(args.warmup):
        call()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": args.reps}


def show(name, out, tail=""):
    print(f"{name:58s} {out['ms_median']:8.3f} ms  [{out['ms_min']:.3f} .. {out['ms_max']:.3f}]  {tail}", flush=True)
    return out


def leg(name, fn, rows, k, verify):
    words = rows.shape[2]
    src, dst = dmalloc(rows.nbytes), dmalloc(N * words * 8)
    assert hip.hipMemcpy(src, C.c_void_p(rows.ctypes.data), C.c_size_t(rows.nbytes), 1) == 0
    out = timed(lambda: _lib.check(fn(ctx._h, src, Lh, N, k, dst)))
    got = np.zeros((N, words), np.uint64)
    assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), dst, C.c_size_t(got.nbytes), 2) == 0
    nv = min(N, 4)  # (the mirror is slow at 32768 entries a query: the first queries stand for the rest)
    assert np.array_equal(got[:nv], verify(rows[:, :nv], k)), name
    hip.hipFree(src), hip.hipFree(dst)
    out.update(bytes_in=int(rows.nbytes), entries_out=int(got[0, dist.GROW_CNT]))
    return show(name, out, f"{out['entries_out']} entries a row")


def clear_leg(name, k, n_planes):
    """the arena's clear alone: hipMemsetAsync of the call's N tables on the null stream and the wait for it"""
    slots = 8
    while slots < 2 * (4 * k + 1):
        slots <<= 1
    words = (1 + 2 * slots + slots // 2 + n_planes * slots + 15) & ~15
    nbytes = words * 8 * N
    buf = dmalloc(nbytes)

    def call():
        assert hip.hipMemsetAsync(buf, 0, C.c_size_t(nbytes), None) == 0
        assert hip.hipDeviceSynchronize() == 0

    out = timed(call)
    hip.hipFree(buf)
    out.update(bytes=int(nbytes), bytes_per_query=int(words * 8))
    return show(name, out, f"{words * 8} bytes a query")


def export_legs(result):
    """N grouped queries over one 100 K-doc segment (keyword 0 is in every doc): the export after the wait, alone"""
    n_docs = 100_000
    hi = m.synth_index(n_docs, [1.0, 0.5], seed=3, n_fields=4, max_pos=6)
    r = np.arange(n_docs, dtype=np.uint64)
    attrs = np.zeros((n_docs, 6), np.uint32)
    attrs[:, 0], attrs[:, 1] = (r % 80).astype(np.uint32), ((r * np.uint64(0x9E3779B1)) % np.uint64(4096)).astype(np.uint32)
    attrs[:, 2], attrs[:, 4], attrs[:, 5] = (r * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32), (r & np.uint64(0xFFFF)).astype(np.uint32), (r % 7).astype(np.uint32)
    seg = m.Segment(ctx, hi)
    seg.set_attrs(attrs)
    batch = m.Batch(ctx, N)
    I6 = m.SORTKEY_INT64
    sets = {0: None, 1: [m.Aggr(m.AGGR_SUM, 64, 32)], 4: [m.Aggr(m.AGGR_SUM, 64, 32, widen=True), m.Aggr(m.AGGR_MIN, 64, 32), m.Aggr(m.AGGR_MAX, 128, 64, kind=I6), m.Aggr(m.AGGR_SUM, 128, 64, kind=I6)]}
    root = m.XQNode.keyword(0, 1)
    dst = dmalloc(N * dist.AROW_WORDS * 8)
    for K, col in ((20, 0), (1024, 1)):
        for n, aggrs in sets.items():
            qs = [m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=K, group=m.Group(col * 32, 32, sort_by=m.GROUPSORT_COUNT), aggrs=aggrs) for _ in range(N)]
            batch.submit(seg, qs)
            batch.wait()
            assert all(g.status == 0 for g in batch.results())
            result["legs"][f"export arows K={K} aggrs={n}"] = show(f"mrk_batch_export_arows, K = {K}, {n} aggregates", timed(lambda: batch.export_arows(dst.value)))
            if n == 0:
                result["legs"][f"export grows K={K}"] = show(f"mrk_batch_export_grows, K = {K}", timed(lambda: batch.export_grows(dst.value)))
    hip.hipFree(dst)
    batch.close()
    seg.close()


result = {"lists": Lh, "queries": N, "legs": {}}
for K, pool, per_list in ((20, 80, 60), (1024, 4096, 4096)):
    grows, arows = rows_of(K, pool, per_list)
    what = f"K = {K}, {per_list} of {pool} groups"
    result["legs"][f"grows K={K}"] = leg(f"mrk_topk_merge_grows, {what}", lib.mrk_topk_merge_grows, grows, K, dist.merge_grows_np)
    for n in AGGRS:
        result["legs"][f"arows K={K} aggrs={n}"] = leg(f"mrk_topk_merge_arows, {what}, {n} aggregates", lib.mrk_topk_merge_arows, arows[n], K, dist.merge_arows_np)
    result["legs"][f"clear grows K={K}"] = clear_leg(f"the clear of {N} group-row tables, K = {K}", K, 0)
    result["legs"][f"clear arows K={K}"] = clear_leg(f"the clear of {N} aggregate-row tables, K = {K}", K, 4)
    del grows, arows
export_legs(result)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
ctx.close()
