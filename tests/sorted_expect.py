"""The expectation every sorted / ordered test compares against, in one place: the oracle's unsorted answer for the same query
with max_matches = number of docs (every match with its weight), ordered on the host by numpy and cut to K.

    lexsort over (first part, [second part,] weight per the tie rule, rowid ascending)

with the parts as numpy reads the raw attribute rows -- unsigned compare for integers of <= 32 bits, float32 compare for floats
(-0.0 == +0.0), the int64 view for a 64-bit attribute -- and never through the library's key map.  then_weight: 0 = the weight is no
part of the order, 1 = weight descending, 2 = weight ascending.  rowid ascending comes last whatever the attributes' directions.

This reading of the reference's sorter is itself pinned on results the reference recorded (tests/test_sorted_golden_cpu.py,
tests/golden/sorted_vectors.json); the GPU tests (test_gpu_sort.py, test_gpu_order.py, the merge tests) call the same functions."""
import dataclasses

import numpy as np

from test_gpu_parity import to_orc


def raw_of(rows, rowid, off, cnt):
    """the raw value of a <= 32-bit attribute (bit offset, bit count) per row"""
    dw = rows[rowid, off >> 5]
    return dw if cnt == 32 else (dw >> np.uint32(off & 31)) & np.uint32((1 << cnt) - 1)


def part_key(raw, kind, desc):
    """what np.lexsort orders ascending, best first"""
    key = raw.view(np.float32).astype(np.float64) + 0.0 if kind == 1 else raw.astype(np.float64)  # (exact: 32-bit values; -0.0 == +0.0)
    return -key if desc else key


def weight_key(weight, then_weight):
    w = weight.astype(np.int64)
    return -w if then_weight == 1 else w if then_weight == 2 else np.zeros_like(w)


def all_matches(orc, oi, q, n_docs):
    full = to_orc(orc, dataclasses.replace(q, sort=None, order=None, max_matches=max(n_docs, 1))).run(oi)
    assert len(full.rowid) == full.total_found
    return full


def expected_sort(orc, oi, q, rows, n_docs):
    """(rowid, weight, raw sort key, total_found) of a query with a Sort"""
    full = all_matches(orc, oi, q, n_docs)
    s = q.sort
    raw = raw_of(rows, full.rowid, s.bit_offset, s.bit_count)
    order = np.lexsort((full.rowid, weight_key(full.weight, s.then_weight), part_key(raw, s.kind, s.desc)))[: q.max_matches]
    return full.rowid[order], full.weight[order], raw[order], int(full.total_found)


def expected_order(orc, oi, q, rows, n_docs):
    """(rowid, weight, order key in Matches.order_key's format, total_found) of a query with an Order"""
    full = all_matches(orc, oi, q, n_docs)
    o = q.order
    p0 = o.parts[0]
    if p0.kind == 2:
        item = p0.bit_offset >> 5
        v = np.ascontiguousarray(rows[full.rowid, item:item + 2]).view(np.int64).reshape(-1)
        keys = [~v if p0.desc else v]  # (~v = -v - 1: descending without overflowing at INT64_MIN)
        okey = v.view(np.uint64)
    else:
        raws = [raw_of(rows, full.rowid, p.bit_offset, p.bit_count) for p in o.parts]
        keys = [part_key(r, p.kind, p.desc) for r, p in zip(raws, o.parts)]
        okey = (raws[0].astype(np.uint64) << np.uint64(32)) | (raws[1].astype(np.uint64) if len(raws) > 1 else np.uint64(0))
    order = np.lexsort(tuple([full.rowid, weight_key(full.weight, o.then_weight)] + keys[::-1]))[: q.max_matches]
    return full.rowid[order], full.weight[order], okey[order], int(full.total_found)
