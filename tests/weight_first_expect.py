"""The expectation of a weight-first order (Order.weight_first: 'ORDER BY weight() DESC, attr', '@weight DESC, date_added DESC',
'ORDER BY weight() ASC'): the oracle's unsorted answer for the same query with max_matches = number of docs (every match with its
weight), ordered on the host by numpy and cut to K.

    lexsort over (weight in the asked direction, [first part, [second part,]] rowid ascending)

with the parts as numpy reads the raw attribute rows -- unsigned compare for integers of <= 32 bits, float32 compare for floats
(-0.0 == +0.0), the int64 view for a 64-bit attribute -- and never through the library's key map: MatchGeneric2_fn / 3_fn with
SPH_KEYPART_WEIGHT as key part 0 (sphinxsort.cpp:4723-4753).  Beside sorted_expect.py, whose helpers it uses, because that file is
one of the existing tests' own."""
import numpy as np

from sorted_expect import all_matches, part_key, raw_of


def order_of(weight, rowid, rows, o):
    """(the permutation that puts the matches in the sorter's order, their order keys in Matches.order_key's format or None)"""
    assert o.weight_first in (1, 2) and o.then_weight == 0
    w = weight.astype(np.int64)
    wkey = -w if o.weight_first == 1 else w
    if not o.parts:
        keys, okey = [], None
    elif o.parts[0].kind == 2:
        p0 = o.parts[0]
        item = p0.bit_offset >> 5
        v = np.ascontiguousarray(rows[rowid, item:item + 2]).view(np.int64).reshape(-1)
        keys = [~v if p0.desc else v]  # (~v = -v - 1: descending without overflowing at INT64_MIN)
        okey = v.view(np.uint64)
    else:
        raws = [raw_of(rows, rowid, p.bit_offset, p.bit_count) for p in o.parts]
        keys = [part_key(r, p.kind, p.desc) for r, p in zip(raws, o.parts)]
        okey = (raws[0].astype(np.uint64) << np.uint64(32)) | (raws[1].astype(np.uint64) if len(raws) > 1 else np.uint64(0))
    return np.lexsort(tuple([rowid] + keys[::-1] + [wkey])), okey


def expected_weight_first(orc, oi, q, rows, n_docs):
    """(rowid, weight, order key or None, total_found) of a query whose Order has weight_first set"""
    full = all_matches(orc, oi, q, n_docs)
    order, okey = order_of(full.weight, full.rowid, rows, q.order)
    order = order[: q.max_matches]
    return full.rowid[order], full.weight[order], None if okey is None else okey[order], int(full.total_found)
