#!/usr/bin/env python3
"""tools/sort_time.py [--docs D] [--queries N] [--reps R] [--out FILE] -- what ordering by an attribute costs next to the relevance
order: the bench corpus, N 2-way ANDs of common keywords per launch, every leg on the block-scan kernel's EXT instances (the
relevance legs are forced there by a pass-all RANGE filter).  Legs: BM25 by relevance; BM25 ORDER BY ts DESC; PROXIMITY_BM25 by
relevance with prox_prune = 0; PROXIMITY_BM25 ORDER BY ts DESC; and, where the checkout has Query.order, BM25 ORDER BY cat DESC, ts DESC
(a 4-valued category first) and BM25 ORDER BY big DESC (a signed 64-bit column), on rows of their own set behind the other legs, which
keep the one-dword rows they always ran on; and, where Order has weight_first, BM25 and PROXIMITY_BM25 ORDER BY weight() DESC, ts DESC
(relevance first, the timestamp as the tie-break: to be read against the relevance legs).  Per leg: warm-up launches, then R launches timed one by one
(submit -> wait, wall clock) -> median, min, max in ms, plus the scan's HIP-event time and n_cands / total_found.  Run on a checkout
without Query.sort it times the relevance legs only (the figures of the commit before)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import manticoresearch_amd as m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=10_000_000)
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
c = bench.zipf_c()
ranks, strata = bench.make_queries(c, 256)
probs = [min(0.5, c / r) for r in ranks]
hi = m.synth_index(args.docs, probs, seed=bench.CORPUS_SEED)
ctx = m.Context(0)
seg = m.Segment(ctx, hi)
rng = np.random.default_rng(1)
rows = np.zeros((args.docs, 1), np.uint32)
rows[:, 0] = np.uint32(1_700_000_000) + rng.integers(0, 50_000_000, args.docs).astype(np.uint32)  # timestamps in a narrow band
seg.set_attrs(rows)
kw = m.XQNode.keyword
N = args.queries
common = [strata["cc"][i] for i in range(256)]
has_sort = hasattr(m, "Sort")
pass_all = [m.Filter(0, 32, min=0, max=0xFFFFFFFF)]


def leg(name, ranker, sort, order=None):
    qs = []
    for i in range(N):
        a, b = common[i]
        q = m.Query(m.XQNode.AND(kw(a, 1), kw(b, 2)), ranker=ranker, max_matches=1000)
        if order is not None:
            q.order = order
        elif sort:
            q.sort = m.Sort(0, 32, desc=True, then_weight=1)
        else:
            q.filters = pass_all
        qs.append(q)
    cq = m.prepare(qs)
    batch = m.Batch(ctx, N)
    for _ in range(args.warmup):
        batch.submit_prepared(seg, cq, N)
        batch.wait()
    wall, scan = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        batch.submit_prepared(seg, cq, N)
        batch.wait()
        wall.append((time.perf_counter() - t0) * 1e3)
        scan.append(batch.stats()["scan_ms"])
    st = batch.stats()
    res = batch.results()
    assert all(r.status == 0 for r in res), [r.status for r in res]
    total = sum(r.total_found for r in res)
    batch.close()
    out = {"ms_median": float(np.median(wall)), "ms_min": float(min(wall)), "ms_max": float(max(wall)), "scan_ms_median": float(np.median(scan)),
           "n_cands": st["n_cands"], "total_found": int(total), "n_rerun": st["n_rerun"], "reps": args.reps}
    print(f"{name:48s} {out['ms_median']:8.3f} ms  [{out['ms_min']:.3f} .. {out['ms_max']:.3f}]  scan {out['scan_ms_median']:.3f}  cands/found {st['n_cands'] / max(total, 1):.4f}", flush=True)
    return out


result = {"docs": args.docs, "queries_per_launch": N, "legs": {}}
result["legs"]["bm25 relevance"] = leg("BM25 by relevance (pass-all filter)", m.SPH_RANK_BM25, False)
if has_sort:
    result["legs"]["bm25 order by ts desc"] = leg("BM25 ORDER BY ts DESC", m.SPH_RANK_BM25, True)
ctx.set("prox_prune", 0)
result["legs"]["proximity_bm25 relevance"] = leg("PROXIMITY_BM25 by relevance, prox_prune = 0", m.SPH_RANK_PROXIMITY_BM25, False)
if has_sort:
    result["legs"]["proximity_bm25 order by ts desc"] = leg("PROXIMITY_BM25 ORDER BY ts DESC", m.SPH_RANK_PROXIMITY_BM25, True)
if hasattr(m, "Order"):  # rows: ts | a 4-valued category | a bigint of both signs (low, high dword)
    wide = np.zeros((args.docs, 4), np.uint32)
    wide[:, 0] = rows[:, 0]
    wide[:, 1] = rng.integers(0, 4, args.docs).astype(np.uint32)
    wide[:, 2:4] = rng.integers(-(1 << 40), 1 << 40, args.docs).astype(np.int64).view(np.uint32).reshape(args.docs, 2)
    seg.set_attrs(wide)
    result["legs"]["bm25 order by cat desc, ts desc"] = leg("BM25 ORDER BY cat DESC, ts DESC", m.SPH_RANK_BM25, True,
                                                            m.Order([m.OrderPart(32, 2, desc=True), m.OrderPart(0, 32, desc=True)], then_weight=1))
    result["legs"]["bm25 order by big desc"] = leg("BM25 ORDER BY big DESC", m.SPH_RANK_BM25, True,
                                                   m.Order([m.OrderPart(64, 64, desc=True, kind=m.SORTKEY_INT64)], then_weight=1))
if hasattr(m, "Order") and "weight_first" in getattr(m.Order, "__dataclass_fields__", {}):  # relevance first, the timestamp as the tie-break
    wf = m.Order([m.OrderPart(0, 32, desc=True)], weight_first=1)
    result["legs"]["bm25 order by weight desc, ts desc"] = leg("BM25 ORDER BY weight() DESC, ts DESC", m.SPH_RANK_BM25, True, wf)
    result["legs"]["proximity_bm25 order by weight desc, ts desc"] = leg("PROXIMITY_BM25 ORDER BY weight() DESC, ts DESC", m.SPH_RANK_PROXIMITY_BM25, True, wf)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
seg.close()
ctx.close()
