"""Worker of tests/test_gpu_runtime_declines.py (own process: torch must load its HIP runtime before libmrk.so does): a query that is
declined while it runs, through ShardMerger on one rank with an attached batch, in the three row formats."""
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K1 = 1024


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def check_results(mdist, fmt, res, want_rows, what):
    """ShardMerger.results' entries against the rows the oracle's answers make: None where the row is declined"""
    for i, (r, w) in enumerate(zip(res, want_rows)):
        if int(w[K1 + 1]) & mdist.ROW_DECLINED:
            assert r is None, (what, i, "a declined query with an answer")
            continue
        assert r is not None, (what, i, "an answered query reported declined")
        docid, weight, tot = (r.rowid, r.weight, r.total_found) if fmt != "narrow" else r
        n = int(w[K1])
        assert tot == int(w[K1 + 1]) and len(docid) == n, (what, i, tot, int(w[K1 + 1]), len(docid), n)
        assert np.array_equal(docid, ~w[:n].astype(np.uint32)), (what, i, docid[:8])
        assert np.array_equal(weight, ((w[:n] >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)), (what, i, weight[:8])


def main():
    import torch
    import torch.distributed as dist

    import manticoresearch_amd as m
    import runtime_declines_common as rd
    from manticoresearch_amd import _lib
    from manticoresearch_amd import dist as mdist
    from oracle import oracle as orc

    orc.build()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        ctx = m.Context(0)
        for trigger in ("fsm", "arena"):
            c = rd.row_corpus(m, trigger)
            qs, declining = rd.row_queries(m, c)
            healthy_qs, _ = rd.row_queries(m, c, with_declining=False)
            nq = len(qs)
            seg = m.Segment(ctx, c.his[0])
            seg.set_attrs(c.seg_rows(0))
            for fmt in rd.FORMATS:
                what = (trigger, fmt)
                want = rd.expected_rows(mdist, orc, fmt, c.his[0], qs, declining, c.seg_rows(0), 0)
                want_healthy = rd.expected_rows(mdist, orc, fmt, c.his[0], healthy_qs, [], c.seg_rows(0), 0)
                batch = m.Batch(ctx, nq)
                sm = mdist.ShardMerger(ctx, batch, nq, rd.KROWS, 1, 0, sorted_rows=fmt == "wide", order_rows=fmt == "order")
                sm.attach([batch])
                with (rd.Settings(ctx, gen_lane_hits=16, gen_spill_mb=1) if trigger == "arena" else rd.Settings(ctx)):
                    batch.submit(seg, qs)
                    sm.merge_attached(1, set_index=0, to_host=True, after_submit=True)
                    rows = sm.finish(0)  # returns: a run-time decline is no overflow, and no rerun is asked for twice
                    res = sm.results(0, allow_declined=True)
                    batch.wait()
                    err = _lib.lib().mrk_last_error().decode(errors="replace")
                assert (rd.LIVE_STATES if trigger == "fsm" else rd.ARENA) in err, (what, err)
                assert [r.status for r in batch.results()] == [-2 if i in declining else 0 for i in range(nq)], what
                rd.assert_rows_equal(mdist, np.array(rows), rd.merge_model(mdist, fmt, want[None], rd.KROWS), (what, "merged rows"))
                for i in declining:
                    rd.assert_declined_row(mdist, rows[i], (what, "merged", i))
                    assert res[i] is None, (what, i)
                check_results(mdist, fmt, res, want, what)
                try:
                    sm.results(0)
                    raise AssertionError("a declined query must raise without allow_declined")
                except m.MrkError:
                    pass
                # the healthy batch behind it, same Batch, same merger: whole rows, no flag left over
                batch.submit(seg, healthy_qs)
                sm.merge_attached(1, set_index=0, to_host=True, after_submit=True)
                rows = sm.finish(0)
                rd.assert_rows_equal(mdist, np.array(rows), rd.merge_model(mdist, fmt, want_healthy[None], rd.KROWS), (what, "healthy batch"))
                check_results(mdist, fmt, sm.results(0, allow_declined=True), want_healthy, (what, "healthy batch"))
                batch.wait()
                _lib.check(sm._set_dst(batch._h, None))
                batch.close()
            seg.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
    print("runtime declines chain ok")
