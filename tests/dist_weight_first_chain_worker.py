"""Worker of tests/test_gpu_weight_first_merge.py (own process: torch must load its HIP runtime before libmrk.so does): the
stream-ordered exchange chain with ORDER rows that carry weight-first orders -- ShardMerger(order_rows=True, weight_first=True), one
rank, through the library's communicator (--lib-comm) or torch.distributed -- over a batch that mixes weight-first queries, queries
ordered by a 64-bit key, sorted and relevance queries; the merged Matches, order_key / sort_key included (order_key None for a
weight-first order without parts), must equal Batch.search."""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from dist_chain_worker import _free_port  # noqa: E402


def main(lib_comm: bool):
    import torch
    import torch.distributed as dist

    import manticoresearch_amd as m
    from manticoresearch_amd import dist as mdist
    from order_merge_common import fold_order_zero
    from sort_merge_common import fold_zero
    from test_gpu_sort import random_queries as random_sort_queries
    from test_gpu_weight_first import BIG, make_rows, orders

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        probs = [0.4, 0.3, 0.2, 0.1, 0.05, 0.04, 0.02, 0.01]
        n_docs, K, base = 200_000, 1024, 1000
        hi = m.synth_index(n_docs, probs, seed=79, max_pos=32)
        rng = np.random.default_rng(14)
        rows = make_rows(rng, n_docs)
        O = orders(m)
        S = random_sort_queries(m, rng, len(probs), 34)
        wfq = [dataclasses.replace(q, sort=None, order=O[i % len(O)]) for i, q in enumerate(S[:17])]
        big = [dataclasses.replace(q, sort=None, order=m.Order([m.OrderPart(BIG * 32, 64, desc=bool(i % 2), kind=m.SORTKEY_INT64)], then_weight=i % 3)) for i, q in enumerate(S[17:23])]
        rel = [dataclasses.replace(q, sort=None) for q in S[23:29]]
        others = big + rel + S[29:]
        qs = [q for i, w in enumerate(wfq) for q in ([w, others[i]] if i < len(others) else [w])]
        nq = len(qs)
        ctx = m.Context(0)
        if lib_comm:
            mdist.lib_comm_init(ctx)
        seg = m.Segment(ctx, hi, rowid_base=base)
        seg.set_attrs(rows)
        ref = m.Batch(ctx, nq)
        want = ref.search(seg, qs)
        assert all(w.status == 0 for w in want)
        is_wf = [q.order is not None and bool(q.order.weight_first) for q in qs]
        assert sum(is_wf) == 17 and sum(q.order is not None for q in qs) == 23 and sum(q.sort is not None for q in qs) == 5 and nq == 34

        def same(got):
            for q, g, w, wf in zip(qs, got, want, is_wf):
                assert g.status == 0 and g.total_found == w.total_found and len(g.rowid) == len(w.rowid)
                assert (g.rowid == w.rowid + base).all() and (g.weight == w.weight).all()
                if wf and not q.order.parts:
                    assert g.sort_key is None and g.order_key is None and w.order_key is None
                elif q.order is not None:
                    assert g.sort_key is None and g.order_key.dtype == np.uint64 and np.array_equal(g.order_key, fold_order_zero(w.order_key, q.order))
                elif q.sort is not None:
                    assert g.order_key is None and np.array_equal(g.sort_key, fold_zero(w.sort_key, q.sort.kind))
                else:
                    assert g.sort_key is None and g.order_key is None

        for kwa in ({}, {"sorted_rows": True}):
            try:
                mdist.ShardMerger(ctx, ref, nq, K, 1, 0, weight_first=True, **kwa)
                raise AssertionError("weight_first without order_rows must be refused")
            except ValueError:
                pass
        # without the switch the same chain declines the weight-first queries and answers the others
        plain = mdist.ShardMerger(ctx, ref, nq, K, 1, 0, order_rows=True)
        ref.submit(seg, qs)
        ref.wait()
        plain.merge()
        got = plain.results(0, allow_declined=True)
        assert [g is None for g in got] == is_wf
        n_sets = 2
        batches = [m.Batch(ctx, nq) for _ in range(n_sets)]
        merger = mdist.ShardMerger(ctx, batches[0], nq, K, 1, 0, n_batches=1, n_sets=n_sets, order_rows=True, weight_first=True)
        assert merger.row_words == mdist.OROW_WORDS
        for i in range(n_sets):
            merger.attach([batches[i]], set_index=i)
        cq = m.prepare(qs)
        for rnd in range(2):  # sets reused: the chain orders itself
            for i in range(n_sets):
                merger.wait(i)
                batches[i].submit_prepared(seg, cq, nq)
                merger.merge_attached(1, set_index=i, to_host=bool(rnd), after_submit=True)
        for i in range(n_sets):
            same(merger.results(i))
            batches[i].wait()
        first, mine = merger.results_slice(0)
        assert first == 0 and len(mine) == nq
        same(mine)
        # the synchronous single-batch form (mrk_batch_export_orows)
        b = m.Batch(ctx, nq)
        sm = mdist.ShardMerger(ctx, b, nq, K, 1, 0, order_rows=True, weight_first=True)
        b.submit_prepared(seg, cq, nq)
        b.wait()
        sm.merge()
        same(sm.results(0))
        for bb in batches + [b, ref]:
            bb.close()
        seg.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(lib_comm="--lib-comm" in sys.argv)
    print("weight-first dist chain ok")
