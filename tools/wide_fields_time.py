#!/usr/bin/env python3
"""tools/wide_fields_time.py [--docs D] [--reps R] [--queries Q] -- what the wide packed path (9-32 fields: the pk_fmask plane and
the scan kernel's WIDE instances) costs: the same seeded query mixes on the same synthetic corpus built with 8 fields and with 16
fields: 2-keyword ANDs under BM25, and 3-keyword PROXIMITY_BM25 mixes (a b c | (a|b) c | a (b|c) | a b -c, as bench.py's config 3).  The 8-field segment runs twice, with the bitmap kernels (bitmap_inv=64) and without them
(bitmap_inv=0): a wide segment never goes to the bitmap kernels.  Scan / selection times per launch from the library's HIP
events, one JSON line per run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manticoresearch_amd as m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--seed", type=int, default=0x5EED0016)
ap.add_argument("--only16", action="store_true", help="the 16-field runs alone (for a profiler)")
args = ap.parse_args()

n_terms = 64
probs = [min(0.3, 0.3 / (r + 1) ** 0.9) for r in range(n_terms)]  # a Zipf-like vocabulary: a few dense words, a long sparse tail
rng = np.random.default_rng(args.seed)
pairs = [tuple(int(x) for x in rng.choice(n_terms, 2, replace=False)) for _ in range(args.queries)]
triples = [tuple(int(x) for x in rng.choice(n_terms, 3, replace=False)) for _ in range(args.queries)]


def mixes():
    kw, X = m.XQNode.keyword, m.XQNode
    and2 = [m.Query(X.AND(kw(a, 1), kw(b, 2)), ranker=m.SPH_RANK_BM25, max_matches=1000) for a, b in pairs]
    prox3 = []
    for i, (a, b, c) in enumerate(triples):
        k = [kw(a, 1), kw(b, 2), kw(c, 3)]
        root = [X.AND(*k), X.AND(X(m.SPH_QUERY_OR, k[:2]), k[2]), X.AND(k[0], X(m.SPH_QUERY_OR, k[1:])), X(m.SPH_QUERY_ANDNOT, [X.AND(*k[:2]), k[2]])][i % 4]
        prox3.append(m.Query(root, ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=1000))
    return {"and2_bm25": and2, "prox3_proximity_bm25": prox3}


def run(n_fields, bitmap_inv):
    t0 = time.perf_counter()
    hi = m.synth_index(args.docs, probs, seed=args.seed, n_fields=n_fields)
    ctx = m.Context(0)
    ctx.set("bitmap_inv", bitmap_inv)
    seg = m.Segment(ctx, hi)
    for mix, qs in mixes().items():
        cq = m.prepare(qs)
        bs = [m.Batch(ctx, len(qs)), m.Batch(ctx, len(qs))]
        for b in bs:
            b.submit_prepared(seg, cq, len(qs))
            b.wait()
        scan = []
        t1 = time.perf_counter()
        for i in range(args.reps):
            bs[i % 2].wait()
            if i >= 2:
                scan.append(bs[i % 2].stats()["scan_ms"])
            bs[i % 2].submit_prepared(seg, cq, len(qs))
        for b in bs:
            b.wait()
        dt = time.perf_counter() - t1
        st = bs[0].stats()
        res = bs[0].results()
        print(json.dumps({"n_fields": n_fields, "bitmap_inv": bitmap_inv, "mix": mix, "queries": len(qs), "ms_per_launch": round(1000 * dt / args.reps, 3),
                          "scan_ms_median": round(float(np.median(scan)) if scan else st["scan_ms"], 4), "merge_ms": round(st["merge_ms"], 4),
                          "dev_MB": round(st["dev_bytes"] / 1e6, 2), "seg_MB": round(seg.device_bytes / 1e6, 1), "items_bm": st["n_items_bm"],
                          "packed": st["packed"], "ok": int(sum(r.status == 0 for r in res)), "matches": int(sum(r.total_found for r in res)),
                          "setup_s": round(t1 - t0, 1)}), flush=True)
        for b in bs:
            b.close()
    seg.close()
    ctx.close()


if not args.only16:
    run(8, 64)
    run(8, 0)
run(16, 0)
