"""CPU: sorted queries across shards without a device.  (1) the sort key map and its inverse under ASan + UBSan
(tests/cpp/sort_unmap.cpp); (2) dist.merge_srows_np -- the numpy mirror of the wide merge kernel -- against the oracle's answer on
the unsharded corpus, with per-shard wide rows built by the test from the oracle's per-shard answers; (3) the same rows through
the gloo exchange, all-gather and partitioned.  Every comparison is exact."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import sort_merge_common as smc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"

N_DOCS, CUTS, PROBS = 24_000, [0, 5_000, 17_001, 24_000], [0.5, 0.3, 0.2, 0.1]
GLOO_CUTS = [0, 9_001, 24_000]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_sort_unmap_inverts_the_map_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sort_unmap")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "cpp", "sort_unmap.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.startswith("ok unmap "), out.stdout


def test_library_unmap_and_constants():
    import manticoresearch_amd as m
    from manticoresearch_amd import _lib, dist

    assert m.SROW_WORDS == dist.SROW_WORDS == 1539 and m.ROW_WORDS == dist.ROW_WORDS == 1026 and hasattr(m.Batch, "export_srows")
    f = _lib.lib().mrk_sort_unmap_key
    rng = np.random.default_rng(1)
    for kind in (0, 1):
        raw = rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)
        raw[:4] = [0, 0x80000000, 0x7F800000, 0xFF800000]
        if kind:
            raw = raw[(raw & np.uint32(0x7FFFFFFF)) <= np.uint32(0x7F800000)]
        for desc in (False, True):
            spec = dist.sort_spec_word(kind, desc, 1, 32)
            mapped = smc.map_keys_np(raw, kind, desc)
            assert np.array_equal(dist.unmap_keys(spec, mapped), smc.fold_zero(raw, kind))
            assert f(spec, int(mapped[1])) == (0 if kind else 0x80000000)


def _corpus(cuts=CUTS):
    import manticoresearch_amd as m
    from test_gpu_sort import make_rows

    return smc.Corpus(m, make_rows, N_DOCS, cuts, PROBS, seed=77, rows_seed=5)


def _shard_srows(orc, corpus, qs):
    from manticoresearch_amd import dist
    from test_gpu_parity import orc_index_of, to_orc
    from test_gpu_sort import expected

    out = np.zeros((len(corpus.shards), len(qs), dist.SROW_WORDS), np.uint64)
    for s, sh in enumerate(corpus.shards):
        oi = orc_index_of(orc, sh)
        oi.attrs = corpus.shard_rows[s]
        for qi, q in enumerate(qs):
            out[s, qi] = smc.shard_answer_row(dist, orc, expected, to_orc, oi, q, corpus.shard_rows[s], len(corpus.shard_rows[s]), corpus.cuts[s])
    return out


def _check_against_whole(orc, corpus, qs, merged, what):
    from manticoresearch_amd import dist
    from test_gpu_parity import orc_index_of, to_orc
    from test_gpu_sort import expected

    oi = orc_index_of(orc, corpus.whole)
    oi.attrs = corpus.rows
    for qi, q in enumerate(qs):
        smc.check_merged_row(dist, orc, expected, to_orc, oi, q, corpus.rows, corpus.n_docs, merged[qi], (what, qi))


def test_merge_srows_np_equals_the_unsharded_answer(orc):
    import manticoresearch_amd as m
    from manticoresearch_amd import dist
    from test_gpu_parity import kw
    from test_gpu_sort import sorts

    corpus = _corpus()
    qs = smc.grid_queries(m, sorts, kw, corpus)
    assert sum(q.sort is None for q in qs) >= 5 and sum(q.sort is not None for q in qs) == 5 * 2 * 3 * 4
    srows = _shard_srows(orc, corpus, qs)
    merged = dist.merge_srows_np(srows, 1024)
    _check_against_whole(orc, corpus, qs, merged, "three shards")
    # the order of the lists is no part of the answer
    assert np.array_equal(dist.merge_srows_np(srows[::-1], 1024), merged)
    # k below the lists' counts cuts the merged row, and its mapped keys with it
    cut = dist.merge_srows_np(srows, 7)
    for qi in range(len(qs)):
        n = min(int(merged[qi, 1024]), 7)
        assert int(cut[qi, 1024]) == n and np.array_equal(cut[qi, :n], merged[qi, :n])
        assert np.array_equal(dist.srow_mkeys(cut[qi])[:n], dist.srow_mkeys(merged[qi])[:n])
        smc.assert_padding(dist, cut[qi])


def test_merge_srows_np_is_loud_and_keeps_flags_and_totals(orc):
    import manticoresearch_amd as m
    from manticoresearch_amd import dist
    from test_gpu_parity import kw
    from test_gpu_sort import sorts

    corpus = _corpus()
    off, cnt, kind = sorts(m)["ts"]
    root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
    qs = [corpus.globalize(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=50, sort=m.Sort(off, cnt, desc=True, then_weight=1, kind=kind))),
          corpus.globalize(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=50))]
    base = _shard_srows(orc, corpus, qs)
    good = dist.merge_srows_np(base, 50)
    totals = [int(base[:, qi, 1025].sum()) for qi in range(2)]
    assert [int(good[qi, 1025]) for qi in range(2)] == totals and int(good[0, 1024]) == 50
    D, R = np.uint64(dist.ROW_DECLINED), np.uint64(dist.ROW_RERUN)
    # differing spec words: another tie rule, another direction, another width, a relevance row next to sorted ones
    for other in (dist.sort_spec_word(kind, True, 2, 32), dist.sort_spec_word(kind, False, 1, 32), dist.sort_spec_word(kind, True, 1, 31),
                  dist.sort_spec_word(1, True, 1, 32), 0):
        for which in range(3):
            rows = base.copy()
            rows[which, 0, dist.SROW_SPEC] = other
            got = dist.merge_srows_np(rows, 50)
            assert int(got[0, 1025]) == totals[0] | dist.ROW_DECLINED and int(got[0, 1024]) == 0
            assert not got[0, :1024].any() and not got[0, dist.SROW_MKEYS:dist.SROW_SPEC].any()
            assert np.array_equal(got[1], good[1])  # the batch's other query is untouched
    rows = base.copy()  # a sorted row next to relevance rows
    rows[1, 1, dist.SROW_SPEC] = dist.sort_spec_word(kind, True, 1, 32)
    got = dist.merge_srows_np(rows, 50)
    assert int(got[1, 1025]) == totals[1] | dist.ROW_DECLINED and int(got[1, 1024]) == 0 and not got[1, :1024].any()
    # flags OR through, totals add; a relevance query keeps its keys (the narrow merge's behaviour), a sorted query that a
    # shard declined leaves without keys
    rows = base.copy()
    rows[2, :, 1025] |= R
    got = dist.merge_srows_np(rows, 50)
    for qi in range(2):
        assert int(got[qi, 1025]) == totals[qi] | dist.ROW_RERUN and np.array_equal(got[qi, :1025], good[qi, :1025])
    rows = base.copy()
    rows[0, :, :1025] = 0
    rows[0, :, dist.SROW_MKEYS:dist.SROW_SPEC] = 0
    rows[0, :, 1025] = D
    got = dist.merge_srows_np(rows, 50)
    assert int(got[0, 1025]) & dist.ROW_DECLINED and int(got[0, 1024]) == 0 and not got[0, :1024].any()
    assert int(got[1, 1025]) & dist.ROW_DECLINED and int(got[1, 1024]) == 50  # relevance: as the narrow merge
    assert int(got[0, 1025]) & ~(dist.ROW_DECLINED | dist.ROW_RERUN) == int(base[1:, 0, 1025].sum())


# ---------------------------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_queries(m, corpus):
    from test_gpu_parity import kw
    from test_gpu_sort import sorts

    qs = smc.grid_queries(m, sorts, kw, corpus)
    return [q for q in qs if q.sort is not None][::7] + [q for q in qs if q.sort is None][:3]


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    import torch.distributed as tdist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    import manticoresearch_amd as m
    from manticoresearch_amd import dist as mdist
    from oracle import oracle as orc
    from test_gpu_parity import orc_index_of, to_orc
    from test_gpu_sort import expected

    corpus = _corpus(GLOO_CUTS)
    qs = _gloo_queries(m, corpus)
    oi = orc_index_of(orc, corpus.shards[rank])
    oi.attrs = corpus.shard_rows[rank]
    mine = np.stack([smc.shard_answer_row(mdist, orc, expected, to_orc, oi, qq, corpus.shard_rows[rank], len(corpus.shard_rows[rank]), corpus.cuts[rank])
                     for qq in qs])
    rows = torch.from_numpy(mine.view(np.int64))
    rows_all = mdist.exchange_rows(rows)
    assert rows_all.shape == (world, len(qs), mdist.SROW_WORDS) and torch.equal(rows_all[rank], rows)
    merged = mdist.merge_srows_np(rows_all.numpy().view(np.uint64), 1024)
    recv, first, count = mdist.exchange_rows_partitioned(rows)
    per = (len(qs) + world - 1) // world
    assert recv.shape == (world, per, mdist.SROW_WORDS) and torch.equal(recv[:, :count], rows_all[:, first:first + count])
    part = mdist.merge_srows_np(recv.numpy().view(np.uint64)[:, :count], 1024)
    q.put((rank, merged, first, count, part))
    tdist.barrier()
    tdist.destroy_process_group()


def test_wide_rows_over_gloo(orc):
    import torch.multiprocessing as mp
    import manticoresearch_amd as m

    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, queue)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([queue.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    corpus = _corpus(GLOO_CUTS)
    qs = _gloo_queries(m, corpus)
    assert any(qq.sort is None for qq in qs) and sum(qq.sort is not None for qq in qs) >= 10
    assert np.array_equal(got[0][1], got[1][1])  # every rank of the all-gather form merges the same rows
    _check_against_whole(orc, corpus, qs, got[0][1], "gloo all-gather")
    together = np.concatenate([g[4] for g in got])  # the partitioned slices, rank after rank
    assert [g[2] for g in got] == [0, got[0][3]] and got[0][3] + got[1][3] == len(qs)
    assert np.array_equal(together, got[0][1])
