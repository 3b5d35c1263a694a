#!/usr/bin/env python3
"""tools/group_time.py [--docs D] [--queries N] [--reps R] [--out FILE] -- what GROUP BY an integer attribute costs next to the nearest
existing path, ORDER BY the same attribute (same kernel instances, same row read): the bench corpus, one launch of N two-keyword BM25
ANDs of common keywords, max_matches 1024, over columns of 4, 1000 and 4096 distinct values -- grouped (Query.group, ordered by
@count desc) and sorted (Query.sort) on the column.  The legs run in turn, rep by rep (alternating: a drift of the machine falls on all
of them alike), after warm-up launches of each.  Per leg: the scan's and the selection's HIP-event times (mrk_batch_stats.scan_ms /
merge_ms), median, min and max in ms.  There is no threshold.  A 4-value column far slower than the 4096-value one would say that the
per-wave reduction in front of the group table (mrk_kgroup.h, group_flush_wave) is not doing its work."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import manticoresearch_amd as m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=10_000_000)
ap.add_argument("--queries", type=int, default=256)
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
CARDS = [4, 1000, 4096]
r = np.arange(args.docs, dtype=np.uint64)
rows = np.zeros((args.docs, len(CARDS)), np.uint32)
for j, card in enumerate(CARDS):  # rowid hashed into `card` values: neighbours in a block differ
    rows[:, j] = ((r * 0x9E3779B1 >> 7) % card).astype(np.uint32)
seg.set_attrs(rows)
kw = m.XQNode.keyword
N, K = args.queries, 1024
common = [strata["cc"][i % len(strata["cc"])] for i in range(N)]


def make(col, grouped):
    qs = []
    for a, b in common:
        q = m.Query(m.XQNode.AND(kw(a, 1), kw(b, 2)), ranker=m.SPH_RANK_BM25, max_matches=K)
        if grouped:
            q.group = m.Group(col * 32, 32, sort_by=m.GROUPSORT_COUNT, desc=True)
        else:
            q.sort = m.Sort(col * 32, 32, desc=True, then_weight=1)
        qs.append(q)
    return m.prepare(qs), m.Batch(ctx, N)


legs = {}
for j, card in enumerate(CARDS):
    legs[f"group by {card} values"] = make(j, True)
for j, card in enumerate(CARDS):
    legs[f"order by {card} values"] = make(j, False)
times = {name: {"scan": [], "select": []} for name in legs}
for rep in range(args.warmup + args.reps):
    for name, (cq, batch) in legs.items():
        batch.submit_prepared(seg, cq, N)
        batch.wait()
        if rep >= args.warmup:
            st = batch.stats()
            times[name]["scan"].append(st["scan_ms"]), times[name]["select"].append(st["merge_ms"])
result = {"docs": args.docs, "queries_per_launch": N, "max_matches": K, "reps": args.reps, "legs": {}}
for name, (cq, batch) in legs.items():
    res = batch.results()
    assert all(x.status == 0 for x in res), (name, [x.status for x in res][:8])
    st = batch.stats()
    t = times[name]
    both = np.array(t["scan"]) + np.array(t["select"])
    out = {"ms_median": float(np.median(both)), "ms_min": float(both.min()), "ms_max": float(both.max()), "scan_ms_median": float(np.median(t["scan"])),
           "select_ms_median": float(np.median(t["select"])), "n_rerun": st["n_rerun"], "total_found": int(sum(x.total_found for x in res))}
    result["legs"][name] = out
    print(f"{name:26s} {out['ms_median']:8.3f} ms  [{out['ms_min']:.3f} .. {out['ms_max']:.3f}]  scan {out['scan_ms_median']:.3f}  select {out['select_ms_median']:.3f}  reruns {st['n_rerun']}", flush=True)
    batch.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
seg.close()
ctx.close()
