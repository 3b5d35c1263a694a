"""Multi-GPU plumbing: one process per GPU, segments = contiguous rowid ranges (the reference's
disk-chunk model, sphinxrt.cpp:6018-6108), torch.distributed (RCCL on ROCm) for the one exchange
step the path has: partial top-K lists are all-gathered and merged, totals are all-reduced, and
document frequencies are summed once so that every shard ranks with the same IDF
(local_df: sphinxrt.cpp:6501-6521, sphinxsearch.cpp:4308-4315).

Merge order across shards: weight desc, then GLOBAL docid (rowid_base + rowid) asc -- the
reference compares (weight, local rowid) and leaves cross-chunk ties to arrival order
(sphinxsort.cpp:4541-4547); we fix the order so results are deterministic.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import MRK_MAX_K, check, lib


def lib_comm_init(ctx):
    """Give the context its own RCCL communicator (mrk_comm_init): rank 0's id travels over the torch.distributed group
    the launcher set up -- any other transport would do, the library itself only needs the 128 bytes.  From here on the
    exchange (ShardMerger) and the document-frequency sums (global_df) are C-ABI calls; torch.distributed only keeps
    bench.py's barrier and timing reduction."""
    import torch.distributed as dist

    box = [ctx.comm_unique_id() if dist.get_rank() == 0 else None]
    dist.broadcast_object_list(box, src=0)
    ctx.comm_init(box[0], dist.get_world_size(), dist.get_rank())


def global_df(local_docs: np.ndarray, shard_docs: int, device=None, ctx=None):
    """Sum per-term document counts and the document total over all ranks (through the library's communicator when the
    context has one, else torch.distributed)."""
    if ctx is not None and ctx.has_comm:
        t = ctx.comm_allreduce(np.concatenate([local_docs.astype(np.int64), [shard_docs]]))
        return t[:-1].copy(), int(t[-1])
    import torch
    import torch.distributed as dist

    dev = "cpu" if dist.get_backend() == "gloo" else f"cuda:{device}"
    t = torch.tensor(np.concatenate([local_docs.astype(np.int64), [shard_docs]]), dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    t = t.cpu().numpy()
    return t[:-1].copy(), int(t[-1])


def exchange_partial_topk(keys, counts, totals):
    """all-gather [nq, MRK_MAX_K] keys and [nq] counts, all-reduce [nq] totals (in place).
    Works on CPU tensors (gloo) and device tensors (nccl = RCCL)."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size()
    keys_all = torch.empty((world,) + tuple(keys.shape), dtype=keys.dtype, device=keys.device)
    counts_all = torch.empty((world,) + tuple(counts.shape), dtype=counts.dtype, device=counts.device)
    # list-of-views form: identical on gloo and nccl (RCCL gathers straight into the slices)
    dist.all_gather([keys_all[i] for i in range(world)], keys.contiguous())
    dist.all_gather([counts_all[i] for i in range(world)], counts.contiguous())
    dist.all_reduce(totals, op=dist.ReduceOp.SUM)
    return keys_all, counts_all, totals


ROW_WORDS = MRK_MAX_K + 2  # MRK_ROW_WORDS: keys | count | total_found
ROW_RERUN, ROW_DECLINED = 1 << 63, 1 << 62  # MRK_ROW_RERUN / MRK_ROW_DECLINED: flag bits of the total_found word
# MRK_SROW_WORDS, the wide row that carries a sorted query (mrk_query.sort) across shards:
#   keys | count | total_found | MRK_MAX_K mapped sort keys (u32, two per word) | sort spec word (0 = a relevance query)
SROW_WORDS = ROW_WORDS + MRK_MAX_K // 2 + 1
SROW_MKEYS, SROW_SPEC = MRK_MAX_K + 2, SROW_WORDS - 1  # word offsets of the u32 plane and of the spec word
SPEC_SORTED, SPEC_FLOAT, SPEC_DESC = 1, 2, 4           # + then_weight << 4 + bit_count << 8 (mrk_sortkey.h, sort_spec_word)


def sort_spec_word(kind: int, desc: bool, then_weight: int, bit_count: int) -> int:
    """The spec word of a sorted query's wide row (kind: SORTKEY_INT 0 / SORTKEY_FLOAT 1)."""
    return SPEC_SORTED | (SPEC_FLOAT if kind else 0) | (SPEC_DESC if desc else 0) | ((then_weight & 3) << 4) | ((bit_count & 63) << 8)


def srow_mkeys(srows: np.ndarray) -> np.ndarray:
    """[..., MRK_MAX_K] u32 view of wide rows' mapped-key plane (rows: uint64 [..., SROW_WORDS], C-contiguous)."""
    return np.ascontiguousarray(srows[..., SROW_MKEYS:SROW_SPEC]).view("<u4")


def unmap_keys(spec: int, mapped: np.ndarray) -> np.ndarray:
    """Raw attribute values behind mapped sort keys (mrk_sort_unmap_key per entry; a float's -0.0 reads +0.0)."""
    f = lib().mrk_sort_unmap_key
    return np.fromiter((f(spec, int(m)) for m in mapped), dtype=np.uint32, count=len(mapped))


def merge_srows_np(srows_all: np.ndarray, k: int) -> np.ndarray:
    """What merge_srows_kernel computes, in numpy: srows_all uint64 [n_lists, nq, SROW_WORDS] -> [nq, SROW_WORDS].  A sorted query
    orders by (mapped key, the weight as then_weight says, global docid asc), a relevance query (spec 0) by (weight, docid);
    totals add up, the two flag bits are OR-ed through; lists whose spec words differ, and a sorted query some list carries
    with ROW_DECLINED, give ROW_DECLINED and no keys.  The CPU mirror the kernel is tested against; a gloo-only host's merge."""
    srows_all = np.ascontiguousarray(srows_all, dtype=np.uint64)
    n_lists, nq, _ = srows_all.shape
    out = np.zeros((nq, SROW_WORDS), dtype=np.uint64)
    mask = np.uint64(ROW_RERUN | ROW_DECLINED)
    for q in range(nq):
        rows = srows_all[:, q]
        spec = int(rows[0, SROW_SPEC])
        cnt = np.minimum(rows[:, MRK_MAX_K], np.uint64(MRK_MAX_K)).astype(np.int64)
        tf = rows[:, MRK_MAX_K + 1]
        total = int((tf & ~mask).sum(dtype=np.uint64))
        flags = int(np.bitwise_or.reduce(tf & mask))
        mismatch = bool((rows[:, SROW_SPEC] != np.uint64(spec)).any())
        if mismatch:
            flags |= ROW_DECLINED
        out[q, MRK_MAX_K + 1] = np.uint64((total & ~(ROW_RERUN | ROW_DECLINED)) | flags)
        out[q, SROW_SPEC] = np.uint64(spec)
        if mismatch or (spec and flags & ROW_DECLINED):
            continue
        keys = np.concatenate([rows[l, :cnt[l]] for l in range(n_lists)])
        mk = np.concatenate([srow_mkeys(rows[l])[:cnt[l]] for l in range(n_lists)]) if spec else np.zeros(len(keys), np.uint32)
        w = (keys >> np.uint64(32)).astype(np.uint32)  # weight ^ 0x80000000: larger = heavier
        tie = (spec >> 4) & 3 if spec else 1
        wpart = w if tie == 1 else ~w if tie == 2 else np.zeros_like(w)
        nd = keys.astype(np.uint32)                    # ~docid: larger = smaller docid
        order = np.lexsort((nd, wpart, mk))[::-1]       # descending by (mapped key, weight part, ~docid)
        n = min(len(keys), k)
        order = order[:n]
        out[q, :n] = keys[order]
        out[q, MRK_MAX_K] = np.uint64(n)
        if spec:
            plane = np.zeros(MRK_MAX_K, dtype="<u4")
            plane[:n] = mk[order]
            out[q, SROW_MKEYS:SROW_SPEC] = plane.view("<u8")
    return out


# MRK_OROW_WORDS, the order row that carries a query ordered by a 64-bit key (mrk_query.order) across shards:
#   keys | count | total_found | MRK_MAX_K mapped keys (u64) | order spec word (0 = a relevance query)
OROW_WORDS = _lib.OROW_WORDS
OROW_MKEYS, OROW_SPEC = MRK_MAX_K + 2, OROW_WORDS - 1  # word offsets of the u64 plane and of the spec word
OSPEC_ORDERED, OSPEC_WIDE, OSPEC_INT64 = 1, 2, 4       # + then_weight << 4 + part p << (8 + 16 p) (mrk_sortkey.h, order_spec_word)
OSPEC_WFIRST = 8                                       # the weight leads the order; bits 4-5 = ITS direction, 1 DESC / 2 ASC
OSPEC_PART_FLOAT, OSPEC_PART_DESC, OSPEC_PART_SIGNED = 1, 2, 4  # + bit_count << 4


def order_spec_word(parts, then_weight: int, weight_first: int = 0) -> int:
    """The spec word of an ordered query's order row.  parts: one or two objects with kind / desc / bit_count (api.OrderPart;
    an api.Sort is one part).  One part of <= 32 bits is a sort (wide bit clear); kind SORTKEY_INT64 stands alone.
    weight_first 1 / 2 (Order.weight_first: weight DESC / ASC in front of the parts): OSPEC_WFIRST, the direction in then_weight's
    place (then_weight itself is not read), the parts as without it; no parts at all only with weight_first 2."""
    def part(kind, desc, bits, signed=False):
        return (OSPEC_PART_FLOAT if kind == 1 else 0) | (OSPEC_PART_DESC if desc else 0) | (OSPEC_PART_SIGNED if signed else 0) | ((bits & 63) << 4)

    parts = list(parts)
    assert weight_first in (0, 1, 2)
    assert 1 <= len(parts) <= 2 or (not parts and weight_first == 2)
    w = OSPEC_ORDERED | ((then_weight & 3) << 4)
    if weight_first:
        w = OSPEC_ORDERED | OSPEC_WFIRST | (weight_first << 4)
        if not parts:
            return w
    p0 = parts[0]
    if int(p0.kind) == 2:  # high dword signed, low dword plain, one direction
        assert len(parts) == 1
        return w | OSPEC_WIDE | OSPEC_INT64 | (part(0, p0.desc, 32, True) << 8) | (part(0, p0.desc, 32) << 24)
    w |= part(int(p0.kind), p0.desc, int(p0.bit_count)) << 8
    if len(parts) == 2:
        w |= OSPEC_WIDE | (part(int(parts[1].kind), parts[1].desc, int(parts[1].bit_count)) << 24)
    return w


def orow_mkeys(orows: np.ndarray) -> np.ndarray:
    """[..., MRK_MAX_K] u64 view of order rows' mapped-key plane (rows: uint64 [..., OROW_WORDS])."""
    return orows[..., OROW_MKEYS:OROW_SPEC]


def _unmap_part(m: np.ndarray, f: int) -> np.ndarray:
    m = m.astype(np.uint32)
    if not f & OSPEC_PART_DESC:
        m = ~m
    if f & OSPEC_PART_FLOAT:
        m = np.where(m & np.uint32(0x80000000), m ^ np.uint32(0x80000000), ~m).astype(np.uint32)
    return m ^ np.uint32(0x80000000) if f & OSPEC_PART_SIGNED else m


def unmap_order_keys(spec: int, mapped: np.ndarray) -> np.ndarray:
    """The values behind 64-bit mapped keys of a row with this order spec word (mrk_order_unmap_key per entry, in numpy), in
    Matches.order_key's format: the raw int64 as u64, or raw0 << 32 | raw1; a sort spec: raw0 << 32.  A float's -0.0 reads +0.0."""
    mapped = np.asarray(mapped, dtype=np.uint64)
    if not spec or (spec & OSPEC_WFIRST and not (spec >> 12) & 63):  # (a weight-first spec without parts)
        return np.zeros(len(mapped), np.uint64)
    r0 = _unmap_part(mapped >> np.uint64(32), (spec >> 8) & 0xFFFF).astype(np.uint64) << np.uint64(32)
    if not spec & OSPEC_WIDE:
        return r0
    return r0 | _unmap_part(mapped & np.uint64(0xFFFFFFFF), (spec >> 24) & 0xFFFF).astype(np.uint64)


def merge_orows_np(orows_all: np.ndarray, k: int) -> np.ndarray:
    """What merge_orows_kernel computes, in numpy: orows_all uint64 [n_lists, nq, OROW_WORDS] -> [nq, OROW_WORDS].  An ordered query
    orders by (64-bit mapped key, the weight as then_weight says, global docid asc), a relevance query (spec 0) by (weight, docid), a
    weight-first one (OSPEC_WFIRST) by (the weight as bits 4-5 say, 64-bit mapped key, global docid asc) -- bits 4-5 neither 1 nor 2 is
    no spec and counts as a mismatch; totals add up, the two flag bits are OR-ed through; answering lists whose spec words differ in any bit, and an ordered query some
    list carries with ROW_DECLINED (its spec word, 0 from a shard whose planner declined, is not compared), give ROW_DECLINED and no
    keys under the answering lists' spec word.  The CPU mirror the kernel is tested against; a gloo-only host's merge."""
    orows_all = np.ascontiguousarray(orows_all, dtype=np.uint64)
    n_lists, nq, _ = orows_all.shape
    out = np.zeros((nq, OROW_WORDS), dtype=np.uint64)
    mask = np.uint64(ROW_RERUN | ROW_DECLINED)
    for q in range(nq):
        rows = orows_all[:, q]
        cnt = np.minimum(rows[:, MRK_MAX_K], np.uint64(MRK_MAX_K)).astype(np.int64)
        tf = rows[:, MRK_MAX_K + 1]
        total = int((tf & ~mask).sum(dtype=np.uint64))
        flags = int(np.bitwise_or.reduce(tf & mask))
        # the spec word is that of the lists which answer the query (a declining shard sends spec 0 and has no say): they must agree
        specs = rows[(tf & np.uint64(ROW_DECLINED)) == 0, OROW_SPEC]
        spec = int(specs[0]) if len(specs) else 0
        mismatch = bool((specs != np.uint64(spec)).any())
        wfirst = bool(spec & OSPEC_WFIRST)
        if wfirst and (spec >> 4) & 3 not in (1, 2):
            mismatch = True
        if mismatch:
            flags |= ROW_DECLINED
        out[q, MRK_MAX_K + 1] = np.uint64((total & ~(ROW_RERUN | ROW_DECLINED)) | flags)
        out[q, OROW_SPEC] = np.uint64(spec)
        if mismatch or (spec and flags & ROW_DECLINED):
            continue
        keys = np.concatenate([rows[l, :cnt[l]] for l in range(n_lists)])
        mk = np.concatenate([rows[l, OROW_MKEYS:OROW_MKEYS + cnt[l]] for l in range(n_lists)]) if spec else np.zeros(len(keys), np.uint64)
        w = (keys >> np.uint64(32)).astype(np.uint32)  # weight ^ 0x80000000: larger = heavier
        tie = (spec >> 4) & 3 if spec else 1
        wpart = w if tie == 1 else ~w if tie == 2 else np.zeros_like(w)
        nd = keys.astype(np.uint32)                    # ~docid: larger = smaller docid
        if wfirst:
            order = np.lexsort((nd, mk, wpart))[::-1]   # descending by (weight part, mapped key as u64, ~docid)
        else:
            order = np.lexsort((nd, wpart, mk))[::-1]   # descending by (mapped key as u64, weight part, ~docid)
        n = min(len(keys), k)
        order = order[:n]
        out[q, :n] = keys[order]
        out[q, MRK_MAX_K] = np.uint64(n)
        if spec:
            out[q, OROW_MKEYS:OROW_MKEYS + n] = mk[order]
    return out


# MRK_GROW_WORDS, the group row that carries a grouped query (api.Group) across segments and shards -- ALL the groups of its list:
#   GROW_GROUPS head keys in group order | count | total_found | GROW_GROUPS (group value << 32 | @count) | group spec word
GROW_WORDS, GROW_GROUPS = _lib.GROW_WORDS, _lib.GROW_GROUPS
GROW_CNT, GROW_TOTAL, GROW_PLANE, GROW_SPEC = GROW_GROUPS, GROW_GROUPS + 1, GROW_GROUPS + 2, GROW_WORDS - 1  # word offsets
GROUPBY_FACTOR = 4


def group_spec_word(sort_by: int, desc, bit_count: int, max_matches: int) -> int:
    """The spec word of a grouped query's group row (mrk_kgroup.h, group_spec_word): bit 0 grouped | bits 1-2 sort_by
    (GROUPSORT_*) | bit 3 desc | bits 8-13 bit_count | bits 16-26 max_matches.  0 = a relevance query."""
    return 1 | ((int(sort_by) & 3) << 1) | ((1 if desc else 0) << 3) | ((int(bit_count) & 63) << 8) | ((int(max_matches) & 2047) << 16)


def group_spec_unpack(spec: int):
    """(sort_by, desc, bit_count, max_matches) of a grouped spec word, or None where it is not one group_spec_word writes for a query
    the library answers (a stray bit, sort_by 3, bit_count outside 1..32, max_matches outside 1..MRK_MAX_K)."""
    spec = int(spec)
    sort_by, desc, bits, k = (spec >> 1) & 3, (spec >> 3) & 1, (spec >> 8) & 63, (spec >> 16) & 2047
    if not spec & 1 or spec != group_spec_word(sort_by, desc, bits, k) or sort_by > 2 or not 1 <= bits <= 32 or not 1 <= k <= MRK_MAX_K:
        return None
    return sort_by, desc, bits, k


def group_order_keys(sort_by: int, desc: int, value: np.ndarray, count: np.ndarray, head: np.ndarray) -> np.ndarray:
    """mrk_kgroup.h group_order_key per group: the part the groups are ordered by, in its direction, over ~head rowid; larger = better."""
    head = np.asarray(head, np.uint64)
    p = (np.asarray(count, np.uint32) if sort_by == 1 else np.asarray(value, np.uint32) if sort_by == 0 else (head >> np.uint64(32)).astype(np.uint32))
    p = p if desc else ~p
    return (p.astype(np.uint64) << np.uint64(32)) | (head & np.uint64(0xFFFFFFFF))


def grow_groups(row: np.ndarray):
    """A group row's answer -> (head rowid, head weight, group key, @count, total_found): the first min(n, max_matches) entries of a
    grouped row (all of a spec-0 row's, with key and count None).  rowids are GLOBAL.  A flagged row gives empty arrays and total None."""
    row = np.asarray(row, dtype=np.uint64)
    n, tf, spec = int(row[GROW_CNT]), int(row[GROW_TOTAL]), int(row[GROW_SPEC])
    flagged = bool(tf & (ROW_RERUN | ROW_DECLINED))
    un = group_spec_unpack(spec) if spec else None
    n = 0 if flagged else min(n, un[3]) if un else min(n, MRK_MAX_K)
    keys = row[:n]
    rowid = ~keys.astype(np.uint32)
    weight = ((keys >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0x80000000)).astype(np.int32)
    plane = row[GROW_PLANE:GROW_PLANE + n]
    gkey = (plane >> np.uint64(32)).astype(np.uint32) if un else None
    gcnt = plane.astype(np.uint32) if un else None
    return rowid, weight, gkey, gcnt, None if flagged else tf


def merge_grows_np(grows_all: np.ndarray, k: int) -> np.ndarray:
    """What merge_grows_kernel computes, in numpy, word for word: grows_all uint64 [n_lists, nq, GROW_WORDS] -> [nq, GROW_WORDS].
    A list with more than GROW_GROUPS entries or a spec word that does not unpack reads as ROW_DECLINED and empty.  The spec word is
    that of the first list that is not ROW_DECLINED under spec 0; the other such lists must agree in every bit.  Spec 0: merge_rows_np over the first
    ROW_WORDS words (keys, count, total word; flags OR-ed through).  Grouped: counts add per group value, the largest head key stays,
    the groups leave ordered by group_order_keys, ALL of them, total_found = their number.  Any flag, a mismatch, a max_matches
    above k, more than 4 * max_matches merged groups or a count above 2^32 - 1: no entries, the flags (ROW_DECLINED for the latter
    four) and the spec word.  The CPU mirror the kernel is tested against; a gloo-only host's merge."""
    grows_all = np.ascontiguousarray(grows_all, dtype=np.uint64)
    n_lists, nq, _ = grows_all.shape
    out = np.zeros((nq, GROW_WORDS), dtype=np.uint64)
    fmask = ROW_RERUN | ROW_DECLINED
    for q in range(nq):
        rows = grows_all[:, q]
        cnt, tw, specs = [], [], []
        for l in range(n_lists):
            c, t, sp = int(rows[l, GROW_CNT]), int(rows[l, GROW_TOTAL]), int(rows[l, GROW_SPEC])
            if c > GROW_GROUPS or (sp and group_spec_unpack(sp) is None):
                c, t, sp = 0, (t & ROW_RERUN) | ROW_DECLINED, 0
            cnt.append(c), tw.append(t), specs.append(sp)
        flags = 0
        for t in tw:
            flags |= t & fmask
        answering = [specs[l] for l in range(n_lists) if not tw[l] & ROW_DECLINED or specs[l]]  # (declined without a spec: no say)
        spec = answering[0] if answering else 0
        mismatch = any(sp != spec for sp in answering)
        if mismatch:
            flags |= ROW_DECLINED
        out[q, GROW_SPEC] = np.uint64(spec)
        if spec == 0:
            total = sum(t & ~fmask for t in tw) & 0xFFFFFFFFFFFFFFFF
            out[q, GROW_TOTAL] = np.uint64((total & ~fmask) | flags)
            if mismatch:
                continue
            keys = np.concatenate([rows[l, :min(cnt[l], MRK_MAX_K)] for l in range(n_lists)])
            n = min(len(keys), k)
            out[q, :n] = np.sort(keys)[::-1][:n]
            out[q, GROW_CNT] = np.uint64(n)
            continue
        sort_by, desc, _bits, kq = group_spec_unpack(spec)
        if kq > k:
            flags |= ROW_DECLINED
        if not flags:
            heads = np.concatenate([rows[l, :cnt[l]] for l in range(n_lists)])
            plane = np.concatenate([rows[l, GROW_PLANE:GROW_PLANE + cnt[l]] for l in range(n_lists)])
            values, inv = np.unique((plane >> np.uint64(32)).astype(np.uint32), return_inverse=True)
            inv = inv.reshape(-1)
            counts = np.zeros(len(values), np.uint64)
            np.add.at(counts, inv, plane & np.uint64(0xFFFFFFFF))
            head = np.zeros(len(values), np.uint64)
            np.maximum.at(head, inv, heads)
            if len(values) > GROUPBY_FACTOR * kq or (len(values) and int(counts.max()) > 0xFFFFFFFF):
                flags |= ROW_DECLINED
            else:
                # (descending by the order key; equal keys -- groups of a multi-value attribute that one doc heads -- the smaller value first)
                order = np.lexsort((values, ~group_order_keys(sort_by, desc, values, counts.astype(np.uint32), head)))
                n = len(values)
                out[q, :n] = head[order]
                out[q, GROW_PLANE:GROW_PLANE + n] = (values[order].astype(np.uint64) << np.uint64(32)) | counts[order]
                out[q, GROW_CNT] = np.uint64(n)
                out[q, GROW_TOTAL] = np.uint64(n)
        if flags:
            out[q, GROW_TOTAL] = np.uint64(flags)
    return out


# MRK_AROW_WORDS, the aggregate row that carries a grouped query WITH its aggregates (api.Aggr): a group row's first 2 G + 2 words |
#   MAX_AGGRS planes of GROW_GROUPS aggregate values (plane a at AROW_AGGR + a * GROW_GROUPS) | group spec word | aggregate spec word
AROW_WORDS = _lib.AROW_WORDS
AROW_AGGR, AROW_GSPEC, AROW_ASPEC = GROW_PLANE + GROW_GROUPS, AROW_WORDS - 2, AROW_WORDS - 1  # word offsets
MAX_AGGRS = _lib.MRK_MAX_AGGRS
_M64, _SIGN = 0xFFFFFFFFFFFFFFFF, 1 << 63


def aggr_spec_word(aggrs, order_by: int = -1) -> int:
    """The aggregate spec word of a grouped query's aggregate row (mrk_kgroup.h, aggr_spec_word): bit 0 set | bits 1-3 n | bits 4-6
    1 + order_by | per aggregate a, bits 8 + 4 a ..: func (2 bits) | a signed 64-bit source | widened.  0 = no aggregates.
    aggrs: api.Aggr-like objects (func, kind, widen)."""
    if not aggrs:
        return 0
    w = 1 | ((len(aggrs) & 7) << 1) | (((int(order_by) + 1) & 7) << 4)
    for a, g in enumerate(aggrs[:MAX_AGGRS]):
        w |= ((int(g.func) & 3) | (4 if int(g.kind) == 2 else 0) | (8 if g.widen else 0)) << (8 + 4 * a)
    return w


def aggr_spec_unpack(spec: int, group_sort_by: int = 0):
    """(n, order_by, [(func, signed 64-bit source, widened)] * n) of an aggregate spec word next to a group spec with this sort_by, or
    None where it is not one the library writes: a stray bit, n outside 1..MAX_AGGRS, func 0 inside n or a nonzero field beyond it,
    both width bits, an order that names a 64-bit result or an index >= n, an order next to a sort_by other than GROUPSORT_KEY."""
    spec = int(spec)
    n, order = (spec >> 1) & 7, (spec >> 4) & 7
    if not spec & 1 or spec >> 24 or spec & 0x80 or not 1 <= n <= MAX_AGGRS or order > n:
        return None
    nibs = [(spec >> (8 + 4 * a)) & 15 for a in range(MAX_AGGRS)]
    for a, nib in enumerate(nibs):
        if (nib & 3 == 0 or nib & 12 == 12) if a < n else nib:
            return None
    if order and (nibs[order - 1] & 12 or group_sort_by != 0):
        return None
    return n, order - 1, [(nib & 3, bool(nib & 4), bool(nib & 8)) for nib in nibs[:n]]


def _arow_head(row):
    """mrk_kgroup.h aggr_row_head: (entries, total word, group spec, aggregate spec); a hostile row reads declined, empty, specs 0"""
    c, t, gsp, asp = int(row[GROW_CNT]), int(row[GROW_TOTAL]), int(row[AROW_GSPEC]), int(row[AROW_ASPEC])
    gs = group_spec_unpack(gsp) if gsp else None
    if c > GROW_GROUPS or (gsp and gs is None) or (asp and (not gsp or aggr_spec_unpack(asp, gs[0]) is None)):
        return 0, (t & ROW_RERUN) | ROW_DECLINED, 0, 0
    return c, t, gsp, asp


def arow_groups(row: np.ndarray):
    """An aggregate row's answer -> grow_groups' tuple (head rowid, head weight, group key, @count, total_found) plus the aggregates'
    values, uint64 (n, n_aggrs): the first min(n, max_matches) entries.  A row without aggregates gives an (n, 0) array."""
    row = np.asarray(row, dtype=np.uint64)
    as_group = np.concatenate([row[:AROW_AGGR], row[AROW_GSPEC:AROW_GSPEC + 1]])
    rowid, weight, gkey, gcnt, total = grow_groups(as_group)
    asp = int(row[AROW_ASPEC])
    un = aggr_spec_unpack(asp, (int(row[AROW_GSPEC]) >> 1) & 3) if asp else None
    n_aggrs = un[0] if un else 0
    vals = np.stack([row[AROW_AGGR + a * GROW_GROUPS:AROW_AGGR + a * GROW_GROUPS + len(rowid)] for a in range(n_aggrs)], axis=1) if n_aggrs else np.zeros((len(rowid), 0), np.uint64)
    return rowid, weight, gkey, gcnt, total, vals


def merge_arows_np(arows_all: np.ndarray, k: int) -> np.ndarray:
    """What merge_arows_kernel computes, in numpy, word for word: arows_all uint64 [n_lists, nq, AROW_WORDS] -> [nq, AROW_WORDS].
    merge_grows_np's rules over both spec words: the election is the group spec's, the answering lists' aggregate spec words must be
    equal in every bit too ("without aggregates" next to "with" is a mismatch), a hostile list (_arow_head) reads declined under spec
    words 0.  Per group value counts add, the largest head stays and every aggregate merges as its accumulator does: SUM adds modulo
    2^64 (a 32-bit result is the low dword), MIN / MAX compare unsigned for INT sources and signed for INT64 ones.  The groups leave
    by the group spec's order, or by the ordering aggregate's merged 32-bit value in its direction, then by head rowid ascending."""
    arows_all = np.ascontiguousarray(arows_all, dtype=np.uint64)
    n_lists, nq, _ = arows_all.shape
    out = np.zeros((nq, AROW_WORDS), dtype=np.uint64)
    fmask = ROW_RERUN | ROW_DECLINED
    for q in range(nq):
        rows = arows_all[:, q]
        heads_ = [_arow_head(rows[l]) for l in range(n_lists)]
        cnt, tw = [h[0] for h in heads_], [h[1] for h in heads_]
        flags = 0
        for t in tw:
            flags |= t & fmask
        answering = [(h[2], h[3]) for h in heads_ if not h[1] & ROW_DECLINED or h[2]]  # (declined without a spec: no say)
        spec, aspec = answering[0] if answering else (0, 0)
        mismatch = any(sa != (spec, aspec) for sa in answering)
        if mismatch:
            flags |= ROW_DECLINED
        out[q, AROW_GSPEC], out[q, AROW_ASPEC] = np.uint64(spec), np.uint64(aspec)
        if spec == 0:
            total = sum(t & ~fmask for t in tw) & _M64
            out[q, GROW_TOTAL] = np.uint64((total & ~fmask) | flags)
            if mismatch:
                continue
            keys = np.concatenate([rows[l, :min(cnt[l], MRK_MAX_K)] for l in range(n_lists)])
            n = min(len(keys), k)
            out[q, :n] = np.sort(keys)[::-1][:n]
            out[q, GROW_CNT] = np.uint64(n)
            continue
        sort_by, desc, _bits, kq = group_spec_unpack(spec)
        n_aggrs, order_by, kinds = aggr_spec_unpack(aspec, sort_by) if aspec else (0, -1, [])
        if kq > k:
            flags |= ROW_DECLINED
        if not flags:
            heads = np.concatenate([rows[l, :cnt[l]] for l in range(n_lists)])
            plane = np.concatenate([rows[l, GROW_PLANE:GROW_PLANE + cnt[l]] for l in range(n_lists)])
            values, inv = np.unique((plane >> np.uint64(32)).astype(np.uint32), return_inverse=True)
            inv = inv.reshape(-1)
            counts = np.zeros(len(values), np.uint64)
            np.add.at(counts, inv, plane & np.uint64(0xFFFFFFFF))
            head = np.zeros(len(values), np.uint64)
            np.maximum.at(head, inv, heads)
            merged = np.zeros((n_aggrs, len(values)), np.uint64)
            for a, (func, src64, widen) in enumerate(kinds):  # the accumulator's arithmetic (mrk_kgroup.h aggr_map / aggr_unmap) over a zero word
                at = AROW_AGGR + a * GROW_GROUPS
                v = np.concatenate([rows[l, at:at + cnt[l]] for l in range(n_lists)])
                sign = np.uint64(_SIGN if src64 else 0)
                if func == 1:
                    np.add.at(merged[a], inv, v)  # (uint64: modulo 2^64)
                elif func == 3:
                    np.maximum.at(merged[a], inv, v ^ sign)
                    merged[a] ^= sign
                else:
                    np.maximum.at(merged[a], inv, ~(v ^ sign))
                    merged[a] = ~merged[a] ^ sign
                if not (src64 or widen):
                    merged[a] &= np.uint64(0xFFFFFFFF)
            if len(values) > GROUPBY_FACTOR * kq or (len(values) and int(counts.max()) > 0xFFFFFFFF):
                flags |= ROW_DECLINED
            else:
                if order_by >= 0:
                    p = merged[order_by].astype(np.uint32)
                    okeys = ((p if desc else ~p).astype(np.uint64) << np.uint64(32)) | (head & np.uint64(0xFFFFFFFF))
                else:
                    okeys = group_order_keys(sort_by, desc, values, counts.astype(np.uint32), head)
                order = np.lexsort((values, ~okeys))  # (descending by the order key, equal keys the smaller value first: as merge_grows_np)
                n = len(values)
                out[q, :n] = head[order]
                out[q, GROW_PLANE:GROW_PLANE + n] = (values[order].astype(np.uint64) << np.uint64(32)) | counts[order]
                for a in range(n_aggrs):
                    out[q, AROW_AGGR + a * GROW_GROUPS:AROW_AGGR + a * GROW_GROUPS + n] = merged[a][order]
                out[q, GROW_CNT] = np.uint64(n)
                out[q, GROW_TOTAL] = np.uint64(n)
        if flags:
            out[q, GROW_TOTAL] = np.uint64(flags)
    return out


def exchange_rows(rows):
    """ONE all-gather of [nq, W] result rows -> [world, nq, W] (gloo on CPU tensors, RCCL on device); W = ROW_WORDS, SROW_WORDS,
    OROW_WORDS, GROW_WORDS or AROW_WORDS: the row width is the tensor's."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size()
    rows_all = torch.empty((world,) + tuple(rows.shape), dtype=rows.dtype, device=rows.device)
    dist.all_gather([rows_all[i] for i in range(world)], rows.contiguous())
    return rows_all


def shard_slice(n_queries: int, world: int, rank: int):
    """(per, first, count) of the queries rank `rank` merges under the partitioned exchange: mrk_shard_slice's arithmetic
    (per = ceil(Q / N); the last ranks may get fewer, or none)."""
    per = (n_queries + world - 1) // world
    first = min(per * rank, n_queries)
    return per, first, min(per, n_queries - first)


def exchange_rows_partitioned(rows):
    """The exchange partitioned by QUERY over torch.distributed (gloo on CPU tensors, RCCL on device tensors): every rank sends each
    owner its rows of the owner's queries and receives every shard's rows of its own -> (recv [world, per, W], first, count), W the
    rows' own width (narrow, wide, order or group rows).
    The same all-to-all of row slices mrk_shard_exchange issues through the library's communicator (grouped ncclSend / ncclRecv)."""
    import torch
    import torch.distributed as dist

    world, rank = dist.get_world_size(), dist.get_rank()
    nq = rows.shape[0]
    per, first, count = shard_slice(nq, world, rank)
    recv = torch.zeros((world, per) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    ops = []
    for p in range(world):
        _, pf, pc = shard_slice(nq, world, p)
        if p == rank:
            recv[p, :count] = rows[first:first + count]
            continue
        if pc:
            ops.append(dist.P2POp(dist.isend, rows[pf:pf + pc].contiguous(), p))
        if count:
            ops.append(dist.P2POp(dist.irecv, recv[p, :count], p))
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()
    return recv, first, count


class ShardMerger:
    """Device-side merge of per-shard results.  One row per query carries the partial top-K keys, their count and
    total_found, so a step costs one collective and one merge launch.  attach() gives each batch a standing slice
    of an exchange buffer that its submits fill on their own stream; merge_attached() then queues all-gather ->
    merge -> host copy as a stream-ordered chain (RCCL stream -> event -> the library's merge stream) and returns
    without blocking; wait(set) blocks until that set's merged rows are in host memory.  merge() is the simple
    synchronous form for one batch."""

    def __init__(self, ctx, batch, n_queries: int, k: int, world: int, device: int, n_batches: int = 1, n_sets: int = 1,
                 sorted_rows: bool = False, order_rows: bool = False, weight_first: bool = False):
        """weight_first=True (needs order_rows): the order rows carry weight-first queries (Order.weight_first) too -- the merger's
        batch and every batch it attaches are told so (Batch.orows_weight_first); results() hands back their order_key (None without
        parts).  Every rank of the exchange must run a library that knows OSPEC_WFIRST.
        order_rows=True (excludes sorted_rows): ORDER rows (OROW_WORDS) through the order-row entry points -- queries ordered by
        a 64-bit key (Query.order) and sorted queries are merged across the shards in the sorter's order; results() hands back
        order_key for the former and sort_key for the latter, decoded from the spec word alone; relevance queries travel along.
        sorted_rows=True: WIDE rows (SROW_WORDS) through the wide entry points -- sorted queries (Query.sort) are merged
        across the shards in the sorter's order and results() hands back their sort_key; relevance queries travel along."""
        import torch

        assert n_sets <= 8  # MRK_MERGE_SLOTS
        self.torch = torch
        self.ctx, self.batch, self.k, self.world = ctx, batch, k, world
        self.per_batch = n_queries
        self.nq = n_queries * n_batches
        dev = f"cuda:{device}"

        def z(*shape):
            return torch.zeros(shape, dtype=torch.int64, device=dev)

        if sorted_rows and order_rows:
            raise ValueError("ShardMerger: sorted_rows and order_rows are mutually exclusive (a batch has one standing destination)")
        if weight_first and not order_rows:
            raise ValueError("ShardMerger: weight_first needs order_rows (no other exchange row carries the weight's position)")
        self.sorted_rows, self.order_rows, self.weight_first = bool(sorted_rows), bool(order_rows), bool(weight_first)
        self.row_words = rw = OROW_WORDS if order_rows else SROW_WORDS if sorted_rows else ROW_WORDS
        L = lib()
        # the narrow entry points or their wide / order-row twins: same arguments
        kind = "orows" if order_rows else "srows" if sorted_rows else "rows"
        self._set_dst = getattr(L, f"mrk_batch_set_{kind}_dst")
        self._export = getattr(L, f"mrk_batch_export_{kind}")
        self._exchange = getattr(L, f"mrk_shard_exchange_{kind}") if kind != "rows" else L.mrk_shard_exchange
        self._merge_async = getattr(L, f"mrk_topk_merge_{kind}_async")
        self.rows = [z(self.nq, rw) for _ in range(n_sets)]
        self.rows_all = [z(world, self.nq, rw) for _ in range(n_sets)]
        self.out_rows = [z(self.nq, rw) for _ in range(n_sets)]
        self.host_rows = [torch.zeros((self.nq, rw), dtype=torch.int64).pin_memory() for _ in range(n_sets)]
        self.gathered = [torch.cuda.Event() for _ in range(n_sets)]
        self.ready = [torch.cuda.Event() for _ in range(n_sets)]
        for ev in self.ready:  # created by their first record; the library re-records them on the batch streams
            ev.record()
        self.attached = [[] for _ in range(n_sets)]
        self.on_host = [False] * n_sets  # where the set's last merge wrote: pinned host rows or device rows
        self.rank = 0
        # the library partitions the merge by query: this rank's merged rows are [first, first + count) only
        self.partitioned = False
        self.first, self.count = 0, self.nq
        self.timing = {} if __import__("os").environ.get("MRK_DIST_TIMING") else None  # host ms per phase, summed
        if self.weight_first and batch is not None:
            batch.orows_weight_first(True)

    def attach(self, batches, set_index: int = 0):
        """Every later submit of batches[i] writes its rows into slice i of exchange buffer `set_index`."""
        n = self.per_batch
        assert len(batches) * n <= self.nq
        for i, b in enumerate(batches):
            check(self._set_dst(b._h, self.rows[set_index][i * n:].data_ptr()))
            if self.weight_first:
                b.orows_weight_first(True)
        self.attached[set_index] = list(batches)

    def merge(self):
        check(self._export(self.batch._h, self.rows[0].data_ptr()))
        self.merge_attached(1, 0)
        self.wait(0)
        return self.out_rows[0][: self.per_batch]


    def merge_attached(self, n_batches: int, set_index: int = 0, to_host: bool = False, after_submit: bool = False):
        """Rows of the attached batches of one set -> all-gather over RCCL -> merge (-> pinned host rows), queued
        back to back; call wait(set_index) before reading or before reusing the set.  after_submit=True: the
        batches were only submitted, not waited for -- the collective is ordered behind their streams by events,
        so the host blocks nowhere (single attached batch per set)."""
        import time
        import torch.distributed as dist

        nq = n_batches * self.per_batch
        assert nq == self.nq, "merge_attached merges the whole attached set"
        t0 = time.perf_counter()
        if self.ctx.has_comm:
            # the library's own chain (mrk_shard_exchange): event on the batch's stream -> RCCL all-gather on the
            # communicator's stream -> merge kernel -> out rows; nothing of torch in it
            if after_submit:
                assert len(self.attached[set_index]) == 1
            bh = self.attached[set_index][0]._h if after_submit else None
            if lib().mrk_shard_partitioned(self.ctx._h):
                import ctypes as C
                import torch.distributed as tdist

                self.partitioned, self.rank = True, (tdist.get_rank() if tdist.is_initialized() else 0)
                f, c = C.c_uint32(), C.c_uint32()
                check(lib().mrk_shard_slice(nq, self.world, self.rank, C.byref(f), C.byref(c)))
                self.first, self.count = f.value, c.value
            check(self._exchange(self.ctx._h, bh, self.rows[set_index].data_ptr(), nq, self.k,
                                           (self.host_rows if to_host else self.out_rows)[set_index].data_ptr(), set_index))
            self.on_host[set_index] = to_host
            if self.timing is not None:
                self.timing["exchange"] = self.timing.get("exchange", 0.0) + (time.perf_counter() - t0) * 1e3
                self.timing["calls"] = self.timing.get("calls", 0) + 1
            return
        rows_all = self.rows_all[set_index]
        if after_submit:
            assert len(self.attached[set_index]) == 1
            ready = self.ready[set_index]
            check(lib().mrk_batch_record_event(self.attached[set_index][0]._h, ready.cuda_event))
            self.torch.cuda.current_stream().wait_event(ready)
        # list-of-views form: identical on gloo and nccl (RCCL gathers straight into the slices)
        dist.all_gather([rows_all[i] for i in range(self.world)], self.rows[set_index])
        ev = self.gathered[set_index]
        ev.record()  # on torch's current stream, behind the collective's completion
        t1 = time.perf_counter()
        check(self._merge_async(self.ctx._h, rows_all.data_ptr(), self.world, nq, self.k,
                                (self.host_rows if to_host else self.out_rows)[set_index].data_ptr(),
                                ev.cuda_event, set_index))
        self.on_host[set_index] = to_host
        t2 = time.perf_counter()
        if self.timing is not None:
            for k_, v in zip(("exchange", "merge"), (t1 - t0, t2 - t1)):
                self.timing[k_] = self.timing.get(k_, 0.0) + v * 1e3
            self.timing["calls"] = self.timing.get("calls", 0) + 1

    def wait(self, set_index: int = 0):
        check(lib().mrk_merge_wait(self.ctx._h, set_index))

    def _merged(self, set_index: int):
        return (self.host_rows[set_index] if self.on_host[set_index] else self.out_rows[set_index].cpu()).numpy().view(np.uint64)

    def finish(self, set_index: int = 0):
        """wait() + never a silently partial answer: a merged row whose total_found word carries MRK_ROW_RERUN (some
        shard's candidate list overflowed and its row left before the rerun) makes EVERY rank -- all of them see the
        same merged rows -- run mrk_batch_wait on its attached batches (the rerun), export the repaired rows, and redo
        the exchange and the merge; a row with MRK_ROW_DECLINED (a shard declined the query) is left flagged for
        results() to report.  Returns the merged rows [nq, ROW_WORDS] as uint64."""
        self.wait(set_index)
        rows = self._merged(set_index)
        if self.partitioned:
            # only [first, first + count) of `rows` is this rank's; whether ANY rank saw a flagged row comes through the
            # all-reduced flag words: every rank reads the same values and takes the same path
            import ctypes as C

            rerun, decl = C.c_uint32(), C.c_uint32()
            check(lib().mrk_shard_flags(self.ctx._h, set_index, C.byref(rerun), C.byref(decl)))
            need_rerun = bool(rerun.value)
        else:
            need_rerun = bool((rows[:, MRK_MAX_K + 1] & np.uint64(ROW_RERUN)).any())
        if not self.attached[set_index] or not need_rerun:
            return rows
        n = self.per_batch
        for i, b in enumerate(self.attached[set_index]):
            check(lib().mrk_batch_wait(b._h))  # reruns this shard's overflowed queries, repairs the device-side lists
            check(self._export(b._h, self.rows[set_index][i * n:].data_ptr()))
        self.merge_attached(len(self.attached[set_index]), set_index, to_host=self.on_host[set_index])
        self.wait(set_index)
        rows = self._merged(set_index)
        if self.partitioned:
            rows_mine = rows[self.first:self.first + self.count]
            bad = self.first + np.flatnonzero(rows_mine[:, MRK_MAX_K + 1] & np.uint64(ROW_RERUN))
        else:
            bad = np.flatnonzero(rows[:, MRK_MAX_K + 1] & np.uint64(ROW_RERUN))
        if bad.size:
            raise _lib.MrkError(_lib.MRK_E_UNSUPPORTED, f"queries {bad.tolist()[:8]}: a shard's candidate list overflowed again on the rerun")
        return rows

    def results_slice(self, set_index: int = 0, allow_declined: bool = False):
        """(first query, decoded results) of the queries THIS rank merged (the partitioned exchange; all of them with one rank)."""
        world, self.world = self.world, 1
        try:
            res = self.results(set_index, allow_declined=allow_declined)
        finally:
            self.world = world
        return self.first, res[self.first:self.first + self.count]

    def results(self, set_index: int = 0, nq=None, allow_declined: bool = False):
        """Decoded (global docid, weight) lists per query + total_found.  A query some shard declined raises MrkError
        (allow_declined=True: its entry is None instead).  With sorted_rows the entries are Matches (rowid = global docid),
        a sorted query's with sort_key (the attribute's raw value per row), a relevance query's with sort_key None.  With
        order_rows: a 64-bit order's entry carries order_key (Matches.order_key's format), a sort's sort_key, a weight-first order's
        order_key (None without parts) and sort_key None."""
        rows = self.finish(set_index)
        out = []
        if self.partitioned and self.world > 1:
            raise RuntimeError("partitioned exchange: this rank holds the queries of results_slice() only")
        for q in range(nq if nq is not None else self.nq):
            cnt, tot = int(rows[q, MRK_MAX_K]), int(rows[q, MRK_MAX_K + 1])
            if tot & ROW_DECLINED:
                if not allow_declined:
                    raise _lib.MrkError(_lib.MRK_E_UNSUPPORTED, f"query {q}: declined on a shard (MRK_E_UNSUPPORTED there); no merged answer")
                out.append(None)
                continue
            k = rows[q, :cnt]
            weight = ((k >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)
            docid = ~k.astype(np.uint32)
            if self.order_rows:
                from .api import Matches

                spec = int(rows[q, OROW_SPEC])
                vals = unmap_order_keys(spec, orow_mkeys(rows[q])[:cnt]) if spec else None
                if spec & OSPEC_WFIRST:  # order_key = the parts behind the weight; none without parts
                    out.append(Matches(docid, weight, tot, 0, None, vals if (spec >> 12) & 63 else None))
                elif spec & OSPEC_WIDE:
                    out.append(Matches(docid, weight, tot, 0, None, vals))
                else:
                    out.append(Matches(docid, weight, tot, 0, (vals >> np.uint64(32)).astype(np.uint32) if spec else None))
                continue
            if self.sorted_rows:
                from .api import Matches

                spec = int(rows[q, SROW_SPEC])
                out.append(Matches(docid, weight, tot, 0, unmap_keys(spec, srow_mkeys(rows[q])[:cnt]) if spec else None))
                continue
            out.append((docid, weight, tot))
        return out
