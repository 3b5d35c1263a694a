"""Worker of tests/test_gpu_aggr_merge.py (own process: it brings up an RCCL communicator): mrk_shard_exchange_arows with one rank,
the rows sent to the rank itself through RCCL (ctx key exchange_self_rccl), partitioned by query (argument 1) or all-gathered (0).
The merged rows of a batch that mixes grouped queries with and without aggregates, relevance and sorted queries must equal the
exported rows merged as one list -- by the kernel and by dist.merge_arows_np -- and mrk_shard_flags must report the declined row."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(part: int):
    import manticoresearch_amd as m
    import test_gpu_group as tg
    from manticoresearch_amd import _lib
    from manticoresearch_amd import dist as mdist
    from group_expect import GROUPSORT_COUNT
    from test_gpu_group import C16, C17, C64, shapes
    from test_gpu_group_aggr import Q, aggr_sets, make_rows
    from test_gpu_order_merge import Hip

    lib, chk = _lib.lib(), _lib.check
    n_docs, RW = 20_000, m.AROW_WORDS
    hi = m.synth_index(n_docs, [1.0, 0.6, 0.4, 0.3, 0.2], seed=9, n_fields=4, max_pos=6)
    ctx = m.Context(0)
    ctx.set("exchange_part", part)
    ctx.set("exchange_self_rccl", 1)
    ctx.comm_init(ctx.comm_unique_id(), 1, 0)
    assert lib.mrk_shard_partitioned(ctx._h) == part
    seg = m.Segment(ctx, hi, rowid_base=500)
    seg.set_attrs(make_rows(n_docs))
    S = aggr_sets(m)
    root2 = shapes(m)["and2"][0]
    qs = [Q(m, "and2", C64, S["four"], K=16, by=GROUPSORT_COUNT), m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10), tg.Q(m, "prox2", C16, K=8), Q(m, "one", C17, S["smm"], K=4),
          m.Query(root2, ranker=m.SPH_RANK_BM25, max_matches=10, sort=m.Sort(C64 * 32, 32)), Q(m, "none", C16, S["one"], K=1024, order=0)]
    nq = len(qs)
    batch = m.Batch(ctx, nq)
    hip = Hip()
    rows, out, ref = (hip.malloc(nq * RW * 8) for _ in range(3))
    for p in (rows, out, ref):
        hip.fill(p, 0xEE, nq * RW * 8)
    batch.submit(seg, qs)
    batch.wait()
    assert [r.status for r in batch.results()] == [0, 0, 0, -2, 0, 0]
    batch.export_arows(rows.value)
    chk(lib.mrk_topk_merge_arows(ctx._h, rows, 1, nq, 1024, ref))
    want = hip.to_host(ref, (nq, RW))
    mine = hip.to_host(rows, (1, nq, RW))
    assert np.array_equal(want, mdist.merge_arows_np(mine, 1024))
    for rnd in range(2):
        chk(lib.mrk_shard_exchange_arows(ctx._h, None, rows, nq, 1024, out, rnd))
        chk(lib.mrk_merge_wait(ctx._h, rnd))
        hip.sync()
        assert np.array_equal(hip.to_host(out, (nq, RW)), want), rnd
        if part:
            rr, dd = C.c_uint32(7), C.c_uint32(7)
            chk(lib.mrk_shard_flags(ctx._h, rnd, C.byref(rr), C.byref(dd)))
            assert (rr.value, dd.value) == (0, 1)
        hip.fill(out, 0xEE, nq * RW * 8)
    D = mdist.ROW_DECLINED
    assert int(want[0, mdist.GROW_TOTAL]) == 64 and int(want[3, mdist.GROW_TOTAL]) == D and int(want[4, mdist.GROW_TOTAL]) == D
    assert int(want[0, mdist.AROW_ASPEC]) == mdist.aggr_spec_word(S["four"]) and want[0, mdist.AROW_AGGR:mdist.AROW_AGGR + 64].all() and int(want[3, mdist.AROW_ASPEC]) == mdist.aggr_spec_word(S["smm"])
    assert int(want[1, mdist.GROW_CNT]) == 10 and int(want[1, mdist.AROW_GSPEC]) == 0 and int(want[2, mdist.AROW_ASPEC]) == 0 and int(want[2, mdist.AROW_GSPEC]) != 0
    assert int(want[4, mdist.AROW_GSPEC]) == 0 and int(want[5, mdist.GROW_CNT]) == 16 and int(want[5, mdist.AROW_ASPEC]) == mdist.aggr_spec_word(S["one"], 0)
    hip.free()
    batch.close()
    seg.close()
    ctx.close()


if __name__ == "__main__":
    main(int(sys.argv[1]))
    print("aggr exchange ok")
