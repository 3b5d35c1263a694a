"""CPU: queries ordered by a 64-bit key across shards without a device.  (1) the 64-bit key map and its inverse under a spec word,
under ASan + UBSan (tests/cpp/order_unmap.cpp), and mrk_order_unmap_key / dist.unmap_order_keys against an independent numpy map;
(2) dist.merge_orows_np -- the numpy mirror of the order-row merge kernel -- against the oracle's answer on the unsharded corpus,
with per-shard order rows built by the test from the oracle's per-shard answers; (3) the loud cases; (4) the same rows through the
gloo exchange, all-gather and partitioned.  Every comparison is exact."""
import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import order_merge_common as omc
import sort_merge_common as smc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"

N_DOCS, CUTS, PROBS = 24_000, [0, 5_000, 17_001, 24_000], [0.5, 0.3, 0.2, 0.1]
GLOO_CUTS = [0, 9_001, 24_000]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_order_unmap_inverts_the_map_under_sanitizers(tmp_path):
    exe = str(tmp_path / "order_unmap")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "cpp", "order_unmap.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.startswith("ok order unmap "), out.stdout


def test_constants():
    import re

    import manticoresearch_amd as m
    from manticoresearch_amd import _lib, dist

    assert m.OROW_WORDS == _lib.OROW_WORDS == dist.OROW_WORDS == 2051 and hasattr(m.Batch, "export_orows")
    assert dist.OROW_MKEYS == 1026 and dist.OROW_SPEC == 2050
    hdr = open(os.path.join(ROOT, "include", "mrk.h")).read()
    assert re.search(r"#define\s+MRK_OROW_WORDS\s+\(MRK_ROW_WORDS \+ MRK_MAX_K \+ 1\)", hdr) and re.search(r"#define\s+MRK_ROW_WORDS\s+\(MRK_MAX_K \+ 2\)", hdr)
    assert re.search(r"#define\s+MRK_MAX_K\s+1024\b", hdr)
    for name in ("mrk_batch_export_orows", "mrk_batch_set_orows_dst", "mrk_topk_merge_orows", "mrk_topk_merge_orows_async", "mrk_topk_merge_orows_part",
                 "mrk_shard_exchange_orows", "mrk_order_unmap_key"):
        assert hasattr(_lib.lib(), name) and name in hdr, name


def test_library_unmap_inverts_the_map():
    import manticoresearch_amd as m
    from manticoresearch_amd import _lib, dist

    f = _lib.lib().mrk_order_unmap_key
    rng = np.random.default_rng(1)
    i64 = np.concatenate([np.array([np.iinfo(np.int64).min, -1, 0, 1, np.iinfo(np.int64).max], np.int64), rng.integers(-2 ** 63, 2 ** 63 - 1, 500, dtype=np.int64)])
    for desc in (False, True):
        o = m.Order([m.OrderPart(0, 64, desc=desc, kind=m.SORTKEY_INT64)], then_weight=1)
        spec = dist.order_spec_word(o.parts, 1)
        assert spec & dist.OSPEC_WIDE and spec & dist.OSPEC_INT64
        mapped = omc.map_order_np(i64.view(np.uint64), o)
        assert np.array_equal(np.argsort(mapped, kind="stable"), np.argsort(i64 if desc else ~i64, kind="stable"))  # larger = better
        assert np.array_equal(dist.unmap_order_keys(spec, mapped).view(np.int64), i64)
        assert [f(spec, int(x)) for x in mapped[:40]] == [int(x) for x in i64.view(np.uint64)[:40]]
    # every pair of <= 32-bit kinds and directions: integer, float (+-0.0, infinities), bit-fields of 1 and 5 bits
    kinds = [(0, 32), (1, 32), (0, 1), (0, 5)]
    edge = np.array([0, 1, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000], np.uint32)
    for ka, ba in kinds:
        for kb, bb in kinds:
            for da in (False, True):
                for db in (False, True):
                    o = m.Order([m.OrderPart(0, ba, desc=da, kind=ka), m.OrderPart(32, bb, desc=db, kind=kb)], then_weight=2)
                    spec = dist.order_spec_word(o.parts, 2)
                    assert spec & dist.OSPEC_WIDE and not spec & dist.OSPEC_INT64 and (spec >> 4) & 3 == 2
                    a = np.concatenate([np.repeat(edge, len(edge)), rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)]) & np.uint32((1 << ba) - 1)
                    b = np.concatenate([np.tile(edge, len(edge)), rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)]) & np.uint32((1 << bb) - 1)
                    ok = np.ones(len(a), bool)
                    if ka:
                        ok &= (a & np.uint32(0x7FFFFFFF)) <= np.uint32(0x7F800000)
                    if kb:
                        ok &= (b & np.uint32(0x7FFFFFFF)) <= np.uint32(0x7F800000)
                    okey = (a[ok].astype(np.uint64) << np.uint64(32)) | b[ok].astype(np.uint64)
                    mapped = omc.map_order_np(okey, o)
                    want = omc.fold_order_zero(okey, o)
                    assert np.array_equal(dist.unmap_order_keys(spec, mapped), want), (ka, ba, kb, bb, da, db)
                    assert [f(spec, int(x)) for x in mapped[:90]] == [int(x) for x in want[:90]], (ka, ba, kb, bb, da, db)
    # a sort's spec: the 32-bit key in the high dword, and the value is what the wide rows' inverse gives
    for kind in (0, 1):
        for desc in (False, True):
            s = m.Sort(0, 32, desc=desc, then_weight=0, kind=kind)
            spec = dist.order_spec_word([s], 0)
            assert spec and not spec & dist.OSPEC_WIDE
            raw = edge[(edge & np.uint32(0x7FFFFFFF)) <= np.uint32(0x7F800000)] if kind else edge
            mapped = smc.map_keys_np(raw, kind, desc)
            got = dist.unmap_order_keys(spec, mapped.astype(np.uint64) << np.uint64(32))
            assert np.array_equal(got, smc.fold_zero(raw, kind).astype(np.uint64) << np.uint64(32))
            assert np.array_equal((got >> np.uint64(32)).astype(np.uint32), dist.unmap_keys(dist.sort_spec_word(kind, desc, 0, 32), mapped))
    assert f(0, 77) == 0 and not dist.unmap_order_keys(0, np.array([5], np.uint64)).any()


def _corpus(cuts=CUTS):
    import manticoresearch_amd as m
    from test_gpu_order import make_rows

    return smc.Corpus(m, make_rows, N_DOCS, cuts, PROBS, seed=77, rows_seed=5)


def _exp():
    from test_gpu_order import expected as exp_order
    from test_gpu_parity import orc_index_of, to_orc
    from test_gpu_sort import expected as exp_sort

    return orc_index_of, to_orc, exp_order, exp_sort


def _shard_orows(orc, corpus, qs):
    from manticoresearch_amd import dist

    orc_index_of, to_orc, exp_order, exp_sort = _exp()
    out = np.zeros((len(corpus.shards), len(qs), dist.OROW_WORDS), np.uint64)
    for s, sh in enumerate(corpus.shards):
        oi = orc_index_of(orc, sh)
        oi.attrs = corpus.shard_rows[s]
        for qi, q in enumerate(qs):
            out[s, qi] = omc.shard_answer_orow(dist, orc, to_orc, exp_order, exp_sort, oi, q, corpus.shard_rows[s], len(corpus.shard_rows[s]), corpus.cuts[s])
    return out


def _check_against_whole(orc, corpus, qs, merged, what):
    from manticoresearch_amd import dist

    orc_index_of, to_orc, exp_order, exp_sort = _exp()
    oi = orc_index_of(orc, corpus.whole)
    oi.attrs = corpus.rows
    for qi, q in enumerate(qs):
        want = omc.answer(orc, to_orc, exp_order, exp_sort, oi, q, corpus.rows, corpus.n_docs)
        omc.check_merged_orow(dist, want, q, merged[qi], (what, qi))


def _grid(m, corpus):
    from test_gpu_order import all_orders
    from test_gpu_parity import kw
    from test_gpu_sort import sorts

    return omc.grid_queries(m, all_orders, sorts, kw, corpus)


def test_merge_orows_np_equals_the_unsharded_answer(orc):
    import manticoresearch_amd as m
    from manticoresearch_amd import dist

    corpus = _corpus()
    qs = _grid(m, corpus)
    n_ord = sum(q.order is not None for q in qs)
    assert n_ord == (8 + 20) * 3 * 2 and sum(q.order is None and q.sort is None for q in qs) >= 5 and sum(q.sort is not None for q in qs) >= 5
    orows = _shard_orows(orc, corpus, qs)
    merged = dist.merge_orows_np(orows, 1024)
    _check_against_whole(orc, corpus, qs, merged, "three shards")
    # the order of the lists is no part of the answer
    assert np.array_equal(dist.merge_orows_np(orows[::-1], 1024), merged)
    assert np.array_equal(dist.merge_orows_np(orows[[1, 2, 0]], 1024), merged)
    # k below the lists' counts cuts the merged row, and its mapped keys with it; padding stays zero
    cut = dist.merge_orows_np(orows, 7)
    for qi in range(len(qs)):
        n = min(int(merged[qi, 1024]), 7)
        assert int(cut[qi, 1024]) == n and np.array_equal(cut[qi, :n], merged[qi, :n])
        assert np.array_equal(dist.orow_mkeys(cut[qi])[:n], dist.orow_mkeys(merged[qi])[:n])
        omc.assert_padding(dist, cut[qi])
        assert np.array_equal(cut[qi, 1025:1026], merged[qi, 1025:1026]) and cut[qi, dist.OROW_SPEC] == merged[qi, dist.OROW_SPEC]


def _merge_rows_np(rows_all, k):
    """The narrow merge in numpy: (weight, docid) = the u64 key descending; totals add up, flags OR through."""
    n_lists, nq, _ = rows_all.shape
    out = np.zeros((nq, 1026), np.uint64)
    mask = np.uint64((1 << 63) | (1 << 62))
    for q in range(nq):
        keys = np.concatenate([rows_all[l, q, :int(rows_all[l, q, 1024])] for l in range(n_lists)])
        keys = np.sort(keys)[::-1][:k]
        out[q, :len(keys)] = keys
        out[q, 1024] = len(keys)
        tf = rows_all[:, q, 1025]
        out[q, 1025] = np.uint64(int((tf & ~mask).sum(dtype=np.uint64)) | int(np.bitwise_or.reduce(tf & mask)))
    return out


def test_merge_orows_np_is_loud_and_keeps_flags_and_totals(orc):
    import manticoresearch_amd as m
    from manticoresearch_amd import dist
    from test_gpu_order import BIG
    from test_gpu_parity import kw
    from test_gpu_sort import sorts

    corpus = _corpus()
    P = sorts(m)
    root = m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2))
    two = m.Order([m.OrderPart(P["cat"][0], P["cat"][1], desc=True, kind=P["cat"][2]), m.OrderPart(P["ts"][0], P["ts"][1], desc=False, kind=P["ts"][2])], then_weight=1)
    big = m.Order([m.OrderPart(BIG * 32, 64, desc=True, kind=m.SORTKEY_INT64)], then_weight=2)
    off, cnt, kind = P["ts"]
    Q = lambda **kwa: corpus.globalize(m.Query(root, ranker=m.SPH_RANK_BM25, max_matches=50, **kwa))
    qs = [Q(order=two), Q(), Q(order=big), Q(sort=m.Sort(off, cnt, desc=True, then_weight=1, kind=kind))]
    base = _shard_orows(orc, corpus, qs)
    good = dist.merge_orows_np(base, 50)
    _check_against_whole(orc, corpus, qs, good, "base")
    totals = [int(base[:, qi, 1025].sum()) for qi in range(4)]
    assert [int(good[qi, 1025]) for qi in range(4)] == totals and int(good[0, 1024]) == 50
    # a relevance query's words 0..1025 equal the narrow merge
    assert np.array_equal(good[1, :1026], _merge_rows_np(base[:, :, :1026], 50)[1]) and not good[1, 1026:].any()
    D, R = np.uint64(dist.ROW_DECLINED), np.uint64(dist.ROW_RERUN)
    spec = int(base[0, 0, dist.OROW_SPEC])
    sort_spec = int(base[0, 3, dist.OROW_SPEC])
    assert spec & dist.OSPEC_WIDE and not sort_spec & dist.OSPEC_WIDE
    # differing spec words: one bit of the second part (its direction; a bit of its width), the first part's direction, the tie rule,
    # a sort next to an order, a relevance row next to an order
    second_desc = spec ^ (dist.OSPEC_PART_DESC << 24)
    assert second_desc == dist.order_spec_word([two.parts[0], dataclasses.replace(two.parts[1], desc=True)], 1)
    for other in (second_desc, spec ^ (1 << 28), spec ^ (dist.OSPEC_PART_DESC << 8), spec ^ (1 << 4), sort_spec, 0):
        for which in range(3):
            rows = base.copy()
            rows[which, 0, dist.OROW_SPEC] = other
            got = dist.merge_orows_np(rows, 50)
            assert int(got[0, 1025]) == totals[0] | dist.ROW_DECLINED and int(got[0, 1024]) == 0
            assert not got[0, :1024].any() and not got[0, dist.OROW_MKEYS:dist.OROW_SPEC].any()
            for qi in (1, 2, 3):  # the batch's other queries are untouched
                assert np.array_equal(got[qi], good[qi])
    for qi, other in ((1, spec), (1, sort_spec), (3, spec)):  # an order / a sort row next to relevance rows; an order row next to sorts
        rows = base.copy()
        rows[1, qi, dist.OROW_SPEC] = other
        got = dist.merge_orows_np(rows, 50)
        assert int(got[qi, 1025]) == totals[qi] | dist.ROW_DECLINED and int(got[qi, 1024]) == 0 and not got[qi, :1024].any()
        assert not got[qi, dist.OROW_MKEYS:dist.OROW_SPEC].any()
    # flags OR through, totals add
    rows = base.copy()
    rows[2, :, 1025] |= R
    got = dist.merge_orows_np(rows, 50)
    for qi in range(4):
        assert int(got[qi, 1025]) == totals[qi] | dist.ROW_RERUN and np.array_equal(got[qi, :1025], good[qi, :1025])
        assert np.array_equal(got[qi, 1026:], good[qi, 1026:])
    # one declined list (e.g. a NaN in that shard's float part): an ordered or sorted query leaves without keys; a relevance query
    # keeps its keys, as in the narrow merge
    rows = base.copy()
    rows[0, :, :1025] = 0
    rows[0, :, dist.OROW_MKEYS:dist.OROW_SPEC] = 0
    rows[0, :, 1025] = D
    got = dist.merge_orows_np(rows, 50)
    for qi in (0, 2, 3):
        assert int(got[qi, 1025]) & dist.ROW_DECLINED and int(got[qi, 1024]) == 0 and not got[qi, :1024].any() and not got[qi, 1026:2050].any()
        assert int(got[qi, 1025]) & ~(dist.ROW_DECLINED | dist.ROW_RERUN) == int(base[1:, qi, 1025].sum())
    assert int(got[1, 1025]) & dist.ROW_DECLINED and int(got[1, 1024]) == 50
    assert np.array_equal(got[1, :1026], _merge_rows_np(rows[:, :, :1026], 50)[1])
    # a shard whose planner declined sends spec 0 with the flag: its spec word has no say, so the merged row -- declined, no keys,
    # under the answering lists' spec word -- is the same whichever list declined
    rows[0, :, dist.OROW_SPEC] = 0
    got0 = dist.merge_orows_np(rows, 50)
    for perm in ([1, 0, 2], [1, 2, 0]):
        assert np.array_equal(dist.merge_orows_np(rows[perm], 50), got0)
    for qi in (0, 2, 3):
        assert got0[qi, dist.OROW_SPEC] == base[1, qi, dist.OROW_SPEC] != 0 and int(got0[qi, 1025]) & dist.ROW_DECLINED and int(got0[qi, 1024]) == 0
    rows[:, :, :1025], rows[:, :, 1026:] = 0, 0  # every list declined: nothing to agree on
    rows[:, :, 1025] = D
    got = dist.merge_orows_np(rows, 50)
    assert (got[:, 1025] == D).all() and not got[:, :1025].any() and not got[:, 1026:].any()


# ---------------------------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_queries(m, corpus):
    qs = _grid(m, corpus)
    return [q for q in qs if q.order is not None][::9] + [q for q in qs if q.order is None and q.sort is None][:3] + [q for q in qs if q.sort is not None][:3]


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

    orc_index_of, to_orc, exp_order, exp_sort = _exp()
    corpus = _corpus(GLOO_CUTS)
    qs = _gloo_queries(m, corpus)
    oi = orc_index_of(orc, corpus.shards[rank])
    oi.attrs = corpus.shard_rows[rank]
    mine = np.stack([omc.shard_answer_orow(mdist, orc, to_orc, exp_order, exp_sort, oi, qq, corpus.shard_rows[rank], len(corpus.shard_rows[rank]), corpus.cuts[rank])
                     for qq in qs])
    rows = torch.from_numpy(mine.view(np.int64))
    rows_all = mdist.exchange_rows(rows)
    assert rows_all.shape == (world, len(qs), mdist.OROW_WORDS) and torch.equal(rows_all[rank], rows)
    merged = mdist.merge_orows_np(rows_all.numpy().view(np.uint64), 1024)
    recv, first, count = mdist.exchange_rows_partitioned(rows)
    per = (len(qs) + world - 1) // world
    assert recv.shape == (world, per, mdist.OROW_WORDS) and torch.equal(recv[:, :count], rows_all[:, first:first + count])
    part = mdist.merge_orows_np(recv.numpy().view(np.uint64)[:, :count], 1024)
    q.put((rank, merged, first, count, part))
    tdist.barrier()
    tdist.destroy_process_group()


def test_order_rows_over_gloo(orc):
    import torch.multiprocessing as mp
    import manticoresearch_amd as m

    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, queue)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([queue.get(timeout=900) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    corpus = _corpus(GLOO_CUTS)
    qs = _gloo_queries(m, corpus)
    assert sum(qq.order is not None for qq in qs) >= 15 and any(qq.sort is not None for qq in qs) and any(qq.order is None and qq.sort is None for qq in qs)
    assert np.array_equal(got[0][1], got[1][1])  # every rank of the all-gather form merges the same rows
    _check_against_whole(orc, corpus, qs, got[0][1], "gloo all-gather")
    together = np.concatenate([g[4] for g in got])  # the partitioned slices, rank after rank
    assert [g[2] for g in got] == [0, got[0][3]] and got[0][3] + got[1][3] == len(qs)
    assert np.array_equal(together, got[0][1])


def test_merge_format_models_accept_every_input():
    """tests/test_gpu_merge_formats.py's inputs (merge_formats_common) all pass through the numpy models, whole rows out; in every size
    case the second query holds fewer entries than k and the third exactly k."""
    import merge_formats_common as mfc

    ref = mfc.references()
    assert {key[:2] for key in ref} == {(kind, fmt) for kind in ("size", "flags") for fmt in mfc.FLAVORS}
    for key, (rows, want) in ref.items():
        for w in ([want] if key[0] == "size" else want.values()):
            assert w.dtype == np.uint64 and w.shape == (mfc.NQ, mfc.words_of(key[1]))
        if key[0] == "size":
            k = key[4]
            assert int(want[1, mfc.K1]) < k and int(want[2, mfc.K1]) == k
