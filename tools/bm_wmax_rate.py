"""tools/bm_wmax_rate.py [--docs N] [--sets S] -- how many match words of the benchmark's cc launches survive the per-word weight
bound (ctx key bm_wmax): bench.py's corpus and cc query sets, every set submitted once after a warm-up pass, the kernel's own
counters (Batch.stats(): bm_words_queued / bm_words_pruned) per set and summed.  Run on the GPU box; prints one JSON line.
The survival rate is what tools/bm_wmax_model.py's host-side figure is compared with."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--sets", type=int, default=0, help="cc sets to run (0 = the whole query file)")
    args = ap.parse_args()
    import manticoresearch_amd as m

    c = bench.zipf_c()
    n_qsets = max(1, (bench.QUERY_FILE // 3) // args.queries)
    ranks, strata = bench.make_queries(c, n_qsets * args.queries)
    probs = [min(0.5, c / r) for r in ranks]
    hi = m.synth_index(args.docs, probs, seed=bench.CORPUS_SEED, skiplist_block_size=128, n_threads=bench.usable_cpus())
    ctx = m.Context(0)
    seg = m.Segment(ctx, hi)
    batch = m.Batch(ctx, args.queries)
    kw = m.XQNode.keyword
    docs = hi.dict["docs"]
    n_run = args.sets if args.sets > 0 else n_qsets
    sets = []
    for s in range(n_run):
        pairs = strata["cc"][s * args.queries:(s + 1) * args.queries]
        sets.append(m.prepare([m.Query(m.XQNode.AND(kw(a, 1), kw(b, 2)), ranker=m.SPH_RANK_BM25, max_matches=1000, total_docs=args.docs,
                                       local_docs={a: int(docs[a]), b: int(docs[b])}) for a, b in pairs]))
    rows = []
    for rep in range(2):  # (the first pass warms the device up)
        rows = []
        for cq in sets:
            batch.submit_prepared(seg, cq, args.queries)
            batch.wait()
            st = batch.stats()
            q, p = st["bm_words_queued"], st["bm_words_pruned"]
            rows.append({"queued": q, "pruned": p, "survive": round(q / max(1, q + p), 5), "scan_ms": round(st["scan_ms"], 4), "cands": st["n_cands"]})
    q, p = sum(r["queued"] for r in rows), sum(r["pruned"] for r in rows)
    print(json.dumps({"docs": args.docs, "queries_per_set": args.queries, "sets": rows, "queued": q, "pruned": p, "survive": round(q / max(1, q + p), 5),
                      "device_MB": round(seg.device_bytes / 1e6, 1)}))
    batch.close()
    seg.close()
    ctx.close()


if __name__ == "__main__":
    main()
