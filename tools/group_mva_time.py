#!/usr/bin/env python3
"""tools/group_mva_time.py [--docs D] [--queries N] [--reps R] [--out FILE] -- what GROUP BY a multi-value attribute costs next to
GROUP BY a row attribute: tools/group_time.py's launch (the bench corpus, N two-keyword BM25 ANDs of common keywords, max_matches
1024, ordered by @count desc) grouped by
  - a row column of 1000 distinct values (group_flush_wave as it stood, in the instances it always ran in),
  - an MVA with 1 value per doc over the same domain -- the same value as the row column, so the same groups and counts,
  - an MVA with 4 values per doc over that domain.
The legs run in turn, rep by rep (alternating: a drift of the machine falls on all of them alike), after warm-up launches of each.
Per leg: median / min / max of the scan's and the selection's HIP-event times (mrk_batch_stats.scan_ms / merge_ms) in ms.  There is
no threshold.  How to read it: the 1-value leg against the row leg is the price of the blob walk -- the flush reads the rows again,
finds each match's span in the pool and reads its values byte-wise -- and of the AGGR instances the MVA batches run in; the 4-value
leg is the price of the expansion: four times the pairs, so four times the rounds of the combine and of the table updates."""
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
CARD, VALUES = 1000, 4
n = args.docs
r = np.arange(n, dtype=np.uint64)
first = (r * 0x9E3779B1 >> 7) % CARD  # rowid hashed into CARD values: neighbours in a block differ
# one blob row per doc, two blob attributes: [length class 0][end of attr 0 = 4][end of attr 1 = 20][1 value][4 values] = 23 bytes
ROW = 3 + 4 + 4 * VALUES
pool = np.zeros(8 + ROW * n, np.uint8)
rec = pool[8:].reshape(n, ROW)
rec[:, 1], rec[:, 2] = 4, 4 + 4 * VALUES
rec[:, 3:7] = first.astype("<u4").view(np.uint8).reshape(n, 4)
four = np.stack([(first + j * 251) % CARD for j in range(VALUES)], axis=1).astype("<u4")  # (251 j mod 1000: four distinct values per doc)
rec[:, 7:] = four.view(np.uint8).reshape(n, 4 * VALUES)
rows = np.zeros((n, 4), np.uint32)
rows[:, 0] = first.astype(np.uint32)
offs = 8 + ROW * r
rows[:, 2], rows[:, 3] = (offs & 0xFFFFFFFF).astype(np.uint32), (offs >> 32).astype(np.uint32)
seg.set_attrs(rows)
seg.set_blobs(pool, 2, rows)
kw = m.XQNode.keyword
N, K = args.queries, 1024
common = [strata["cc"][i % len(strata["cc"])] for i in range(N)]
GROUPS = {"row column": m.Group(0, 32, sort_by=m.GROUPSORT_COUNT, desc=True),
          "MVA, 1 value per doc": m.Group(0, 0, sort_by=m.GROUPSORT_COUNT, desc=True, mva_bits=32, blob_attr_id=0, n_blob_attrs=2),
          "MVA, 4 values per doc": m.Group(0, 0, sort_by=m.GROUPSORT_COUNT, desc=True, mva_bits=32, blob_attr_id=1, n_blob_attrs=2)}


def make(group):
    qs = [m.Query(m.XQNode.AND(kw(a, 1), kw(b, 2)), ranker=m.SPH_RANK_BM25, max_matches=K, group=group) for a, b in common]
    return m.prepare(qs), m.Batch(ctx, N)


legs = {f"group by {CARD} values, {name}": make(g) for name, g in GROUPS.items()}
times = {name: {"scan": [], "select": []} for name in legs}
for rep in range(args.warmup + args.reps):
    for name, (cq, batch) in legs.items():
        batch.submit_prepared(seg, cq, N)
        batch.wait()
        if rep >= args.warmup:
            st = batch.stats()
            times[name]["scan"].append(st["scan_ms"]), times[name]["select"].append(st["merge_ms"])
stat = lambda a: {"median": float(np.median(a)), "min": float(np.min(a)), "max": float(np.max(a))}
result = {"docs": args.docs, "queries_per_launch": N, "max_matches": K, "reps": args.reps, "legs": {}}
answers = {}
for name, (cq, batch) in legs.items():
    res = batch.results()
    assert all(x.status == 0 for x in res), (name, [x.status for x in res][:8])
    answers[name] = res
    st = batch.stats()
    t = times[name]
    out = {"scan_ms": stat(t["scan"]), "merge_ms": stat(t["select"]), "n_rerun": st["n_rerun"], "total_found": int(sum(x.total_found for x in res)),
           "pushes": int(sum(int(x.group_count.sum()) for x in res))}
    result["legs"][name] = out
    print(f"{name:44s} scan {out['scan_ms']['median']:8.3f} ms [{out['scan_ms']['min']:.3f} .. {out['scan_ms']['max']:.3f}]  select {out['merge_ms']['median']:.3f} "
          f"[{out['merge_ms']['min']:.3f} .. {out['merge_ms']['max']:.3f}]  reruns {st['n_rerun']}", flush=True)
    batch.close()
# the 1-value MVA holds the row column's value: the same groups, counts and heads
names = list(legs)
for a, b in zip(answers[names[0]], answers[names[1]]):
    assert a.total_found == b.total_found and np.array_equal(a.group_key, b.group_key) and np.array_equal(a.group_count, b.group_count) and np.array_equal(a.rowid, b.rowid)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
seg.close()
ctx.close()
