"""Shared by the tests of the order rows (queries ordered by a 64-bit key across shards): an independent numpy statement of the
64-bit key map, packing of per-shard results into order rows, decoding and checking of merged rows.  Nothing here calls the
library's map or merge; the spec word is dist.order_spec_word's (it is carried, not interpreted, by what is under test here)."""
import dataclasses

import numpy as np

import sort_merge_common as smc

K1 = smc.K1
U32 = np.uint64(32)


def map_order_np(okey, order):
    """64-bit mapped key (larger = better) of raw order keys in Matches.order_key's format, from the order's definition: an INT64
    part compares as a signed integer; else map32(first) << 32 | map32(second), each part by sort_merge_common.map_keys_np."""
    okey = np.asarray(okey, dtype=np.uint64)
    p0 = order.parts[0]
    if int(p0.kind) == 2:
        m = okey ^ np.uint64(1 << 63)
        return m if p0.desc else ~m
    hi = smc.map_keys_np((okey >> U32).astype(np.uint32), int(p0.kind), p0.desc).astype(np.uint64) << U32
    if len(order.parts) == 1:
        return hi
    p1 = order.parts[1]
    return hi | smc.map_keys_np(okey.astype(np.uint32), int(p1.kind), p1.desc).astype(np.uint64)


def fold_order_zero(okey, order):
    """Raw order keys with every float part's -0.0 folded onto +0.0 (the map does not keep the sign of zero)."""
    okey = np.asarray(okey, dtype=np.uint64)
    if int(order.parts[0].kind) == 2:
        return okey
    hi = smc.fold_zero((okey >> U32).astype(np.uint32), int(order.parts[0].kind)).astype(np.uint64) << U32
    lo = okey.astype(np.uint32)
    if len(order.parts) > 1:
        lo = smc.fold_zero(lo, int(order.parts[1].kind))
    return hi | lo.astype(np.uint64)


def spec_of(mdist, q):
    if q.order is not None:
        return mdist.order_spec_word(q.order.parts, q.order.then_weight)
    if q.sort is not None:
        return mdist.order_spec_word([q.sort], q.sort.then_weight)
    return 0


def pack_orow(mdist, docid, weight, total, spec=0, mapped=None):
    """One order row from a shard's answer (global docids, in the sorter's order)."""
    row = np.zeros(mdist.OROW_WORDS, np.uint64)
    n = len(docid)
    row[:n] = smc.make_keys(weight, docid)
    row[K1] = n
    row[K1 + 1] = total
    if spec:
        row[mdist.OROW_MKEYS:mdist.OROW_MKEYS + n] = mapped
        row[mdist.OROW_SPEC] = spec
    return row


def answer(orc, to_orc, exp_order, exp_sort, oi, q, rows, n_docs):
    """(rowid, weight, mapped keys or None, raw values, total) of q on one index, from the oracle + numpy."""
    if q.order is not None:
        rid, w, okey, total = exp_order(orc, oi, q, rows, n_docs)
        return rid, w, map_order_np(okey, q.order), okey, total
    if q.sort is not None:
        rid, w, raw, total = exp_sort(orc, oi, q, rows, n_docs)
        return rid, w, smc.map_keys_np(raw, q.sort.kind, q.sort.desc).astype(np.uint64) << U32, raw, total
    r = to_orc(orc, q).run(oi)
    return r.rowid, r.weight, None, None, int(r.total_found)


def shard_answer_orow(mdist, orc, to_orc, exp_order, exp_sort, oi, q, rows, n_docs, base):
    rid, w, mapped, _, total = answer(orc, to_orc, exp_order, exp_sort, oi, q, rows, n_docs)
    return pack_orow(mdist, rid.astype(np.int64) + base, w, total, spec_of(mdist, q), mapped)


def decode_orow(row, k):
    n = min(int(row[K1]), k)
    keys = row[:n]
    weight = ((keys >> U32).astype(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)
    return ~keys.astype(np.uint32), weight, int(row[K1 + 1])


def assert_padding(mdist, row):
    """Zero past count: keys and mapped keys; a relevance row's whole plane."""
    n = int(row[K1])
    assert not row[n:K1].any() and not row[mdist.OROW_MKEYS + n:mdist.OROW_SPEC].any()
    if not int(row[mdist.OROW_SPEC]):
        assert not row[mdist.OROW_MKEYS:mdist.OROW_SPEC].any()


def check_merged_orow(mdist, want, q, row, what=""):
    """A merged order row against the unsharded expectation `want` = answer(...) on the whole corpus."""
    rid, w, _, raw, tot = want
    assert not int(row[K1 + 1]) & (mdist.ROW_RERUN | mdist.ROW_DECLINED), (what, "flagged")
    assert_padding(mdist, row)
    assert int(row[mdist.OROW_SPEC]) == spec_of(mdist, q), what
    docid, weight, total = decode_orow(row, q.max_matches)
    assert total == tot, (what, total, tot)
    assert len(docid) == len(rid) and np.array_equal(docid, rid), (what, q.order, q.sort, q.max_matches, docid[:8], rid[:8])
    assert np.array_equal(weight, w), (what, weight[:8], w[:8])
    n = len(docid)
    vals = mdist.unmap_order_keys(int(row[mdist.OROW_SPEC]), mdist.orow_mkeys(row)[:n])
    if q.order is not None:
        assert np.array_equal(vals, fold_order_zero(raw, q.order)), (what, q.order, vals[:4], raw[:4])
    elif q.sort is not None:
        assert np.array_equal((vals >> U32).astype(np.uint32), smc.fold_zero(raw, q.sort.kind)) and not (vals & np.uint64(0xFFFFFFFF)).any(), (what, q.sort)


def every_order(m, all_orders):
    """test_gpu_order.all_orders (every bigint column x direction, every ordered pair of the <= 32-bit columns) under each tie rule"""
    return [dataclasses.replace(o, then_weight=t) for o in all_orders(m) for t in (0, 1, 2)]


def grid_queries(m, all_orders, sorts, kw, corpus):
    """Every order of every_order at K = 10 and K = 1000 over three query shapes, with relevance and Sort queries in the same set."""
    roots = [(kw(m, 0, 1), m.SPH_RANK_BM25), (m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2)), m.SPH_RANK_PROXIMITY_BM25),
             (m.XQNode.AND(kw(m, 1, 1), kw(m, 2, 2)), m.SPH_RANK_NONE)]
    S = list(sorts(m).items())
    qs, i = [], 0
    for o in every_order(m, all_orders):
        for K in (10, 1000):
            root, rk = roots[i % 3]
            qs.append(corpus.globalize(m.Query(root, ranker=rk, max_matches=K, order=o)))
            if i % 12 == 0:
                qs.append(corpus.globalize(m.Query(root, ranker=rk, max_matches=K)))
            if i % 12 == 6:
                off, cnt, kind = S[(i // 12) % len(S)][1]
                qs.append(corpus.globalize(m.Query(root, ranker=rk, max_matches=K, sort=m.Sort(off, cnt, desc=i % 24 == 6, then_weight=(i // 12) % 3, kind=kind))))
            i += 1
    return qs
