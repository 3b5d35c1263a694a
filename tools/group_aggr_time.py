#!/usr/bin/env python3
"""tools/group_aggr_time.py [--docs D] [--queries N] [--reps R] [--out FILE] -- what the aggregates of a grouped query cost next to
the same grouped query without them: tools/group_time.py's launch (the bench corpus, N two-keyword BM25 ANDs of common keywords,
max_matches 1024, grouped by columns of 4, 1000 and 4096 distinct values, ordered by @count desc) with 0, 1 and 4 aggregates --
1 = a 32-bit SUM; 4 = a widened SUM, a MIN, a MAX and a SUM of a signed 64-bit attribute.  The legs run in turn, rep by rep
(alternating: a drift of the machine falls on all of them alike), after warm-up launches of each.  Per leg: the scan's and the
selection's HIP-event times (mrk_batch_stats.scan_ms / merge_ms), median, min and max in ms.  There is no threshold.
How to read it: the 0-aggregate legs run group_flush_wave as it stood.  With aggregates a flush costs one wave reduction and one
atomic per (distinct value of the buffer, aggregate): a 4-value column pays 4 rounds per aggregate and flush, a 4096-value column up
to 128 -- there nearly every buffered match is a group of its own and the reduction combines nothing.  A cost that grows with the
column's cardinality points at the rounds of the per-wave reduction; one that stayed flat across the columns and grew with the
number of aggregates alone would point at the slot atomics and the rows' re-read."""
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
VAL, I64 = len(CARDS), len(CARDS) + 1  # a 32-bit value column; a signed 64-bit one (two dwords, low first)
r = np.arange(args.docs, dtype=np.uint64)
rows = np.zeros((args.docs, len(CARDS) + 3), np.uint32)
for j, card in enumerate(CARDS):  # rowid hashed into `card` values: neighbours in a block differ
    rows[:, j] = ((r * 0x9E3779B1 >> 7) % card).astype(np.uint32)
rows[:, VAL] = (r * 0x85EBCA6B & 0xFFFFFFFF).astype(np.uint32)
v64 = r * np.uint64(0x9E3779B97F4A7C15)
rows[:, I64], rows[:, I64 + 1] = (v64 & np.uint64(0xFFFFFFFF)).astype(np.uint32), (v64 >> np.uint64(32)).astype(np.uint32)
seg.set_attrs(rows)
kw = m.XQNode.keyword
N, K = args.queries, 1024
common = [strata["cc"][i % len(strata["cc"])] for i in range(N)]
AGGRS = {0: None, 1: [m.Aggr(m.AGGR_SUM, VAL * 32, 32)],
         4: [m.Aggr(m.AGGR_SUM, VAL * 32, 32, widen=True), m.Aggr(m.AGGR_MIN, VAL * 32, 32), m.Aggr(m.AGGR_MAX, VAL * 32, 32), m.Aggr(m.AGGR_SUM, I64 * 32, 64, kind=m.SORTKEY_INT64)]}


def make(col, n_aggr):
    qs = [m.Query(m.XQNode.AND(kw(a, 1), kw(b, 2)), ranker=m.SPH_RANK_BM25, max_matches=K, group=m.Group(col * 32, 32, sort_by=m.GROUPSORT_COUNT, desc=True), aggrs=AGGRS[n_aggr])
          for a, b in common]
    return m.prepare(qs), m.Batch(ctx, N)


legs = {f"group by {card} values, {na} aggregates": make(j, na) for j, card in enumerate(CARDS) for na in AGGRS}
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
    assert all((x.aggr is None) == name.endswith(" 0 aggregates") for x in res), name
    st = batch.stats()
    t = times[name]
    both = np.array(t["scan"]) + np.array(t["select"])
    out = {"ms_median": float(np.median(both)), "ms_min": float(both.min()), "ms_max": float(both.max()), "scan_ms_median": float(np.median(t["scan"])),
           "select_ms_median": float(np.median(t["select"])), "n_rerun": st["n_rerun"], "total_found": int(sum(x.total_found for x in res))}
    result["legs"][name] = out
    print(f"{name:40s} {out['ms_median']:8.3f} ms  [{out['ms_min']:.3f} .. {out['ms_max']:.3f}]  scan {out['scan_ms_median']:.3f}  select {out['select_ms_median']:.3f}  reruns {st['n_rerun']}", flush=True)
    batch.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
seg.close()
ctx.close()
