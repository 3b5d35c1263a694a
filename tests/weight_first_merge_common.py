"""Shared by tests/test_weight_first_merge_cpu.py and tests/test_gpu_weight_first_merge.py: weight-first orders (Order.weight_first)
in ORDER rows.  Synthetic lists in the style of merge_formats_common.make_list, the merged row they must give -- written here from
the order's definition, a lexsort over decoded (weight, mapped key, docid), and never through dist.merge_orows_np, which is under
test --, and the packing of a shard's oracle answer into an order row."""
import functools
import zlib

import numpy as np

import order_merge_common as omc
from merge_formats_common import KS, LISTS, LOW, NQ, U32, counts_of

K1 = 1024
# flavour -> the three mapped keys its entries draw from (d1 : d2 of mrk_sortkey.h): one part of <= 32 bits keeps the low dword
# zero; two parts and an INT64 differ in either dword; no parts: the plane is zero
TABLES = {
    "one": [7 << 32, 8 << 32, 9 << 32],
    "two": [(7 << 32) | 0xFFFFFFFF, (7 << 32) | 0xFFFFFFFE, (8 << 32) | 0xFFFFFFFF],
    "int64": [(0x7FFFFFFF << 32) | 5, (0x80000000 << 32) | 0, (0x80000000 << 32) | 7],
    "none": [0, 0, 0],
}
FLAVORS = [(f, wf) for f in ("one", "two", "int64") for wf in (1, 2)] + [("none", 2)]


def mdist():
    from manticoresearch_amd import dist

    return dist


def parts_of(flavor):
    import manticoresearch_amd as m

    P = m.OrderPart
    return {"one": [P(0, 2, desc=True)], "two": [P(0, 2, desc=True), P(32, 4, desc=False)], "int64": [P(64, 64, desc=True, kind=m.SORTKEY_INT64)], "none": []}[flavor]


def spec_of(flavor, wf):
    return mdist().order_spec_word(parts_of(flavor), 0, weight_first=wf)


def query_spec(q):
    """omc.spec_of for every query, a weight-first one included"""
    if q.order is not None and q.order.weight_first:
        return mdist().order_spec_word(q.order.parts, 0, weight_first=q.order.weight_first)
    return omc.spec_of(mdist(), q)


def decode(row):
    """(weight as a signed integer, mapped key, docid) of a row's entries"""
    n = int(row[K1])
    keys = row[:n]
    weight = ((keys >> U32).astype(np.uint32) ^ np.uint32(0x80000000)).view(np.int32).astype(np.int64)
    return weight, row[K1 + 2:K1 + 2 + n].copy(), (~keys & LOW).astype(np.int64)


def definition_order(weight, mapped, docid, wf):
    """The permutation into a weight-first order: the weight as wf says (1 descending, 2 ascending), then the mapped key (larger =
    better), then docid ascending."""
    assert wf in (1, 2)
    return np.lexsort((docid, ~np.asarray(mapped, np.uint64), -weight if wf == 1 else weight))  # (~m: descending in an unsigned key)


def make_list(rng, flavor, wf, count, docid0, total=None, flags=0, spec=None):
    """One list's order row: `count` entries, docids docid0 .. (distinct over a query's lists), 5 distinct weights and the flavour's 3
    mapped keys, so that ties reach every level; in the order its shard would hand it in."""
    row = np.zeros(mdist().OROW_WORDS, np.uint64)
    docid = (rng.permutation(count) + docid0).astype(np.int64)
    weight = rng.integers(1000, 1005, count).astype(np.int64)
    mk = np.array(TABLES[flavor], np.uint64)[rng.integers(0, 3, count)]
    order = definition_order(weight, mk, docid, wf)
    row[:count] = ((weight[order].astype(np.uint64) ^ np.uint64(0x80000000)) << U32) | (~docid[order].astype(np.uint64) & LOW)
    row[K1] = count
    row[K1 + 1] = np.uint64((100_000 + docid0 if total is None else total) | flags)
    row[K1 + 2:K1 + 2 + count] = mk[order]
    row[-1] = spec_of(flavor, wf) if spec is None else spec
    return row


def expected_merge(rows_all, k):
    """The merged rows of valid, unflagged weight-first lists [n_lists][nq][OROW_WORDS] that share a spec word, from the definition."""
    n_lists, nq, W = rows_all.shape
    out = np.zeros((nq, W), np.uint64)
    for q in range(nq):
        spec = int(rows_all[0, q, -1])
        assert spec & 8 and all(int(rows_all[l, q, -1]) == spec for l in range(n_lists))
        wf = (spec >> 4) & 3
        dec = [decode(rows_all[l, q]) for l in range(n_lists)]
        weight, mapped, docid = (np.concatenate([d[i] for d in dec]) for i in range(3))
        order = definition_order(weight, mapped, docid, wf)[:k]
        n = len(order)
        out[q, :n] = ((weight[order].astype(np.uint64) ^ np.uint64(0x80000000)) << U32) | (~docid[order].astype(np.uint64) & LOW)
        out[q, K1] = n
        out[q, K1 + 1] = rows_all[:, q, K1 + 1].sum(dtype=np.uint64)
        out[q, K1 + 2:K1 + 2 + n] = mapped[order]
        out[q, -1] = spec
    return out


def levels_decided(rows_all, k):
    """Which levels of the order decide between neighbours of the merged top k that come from DIFFERENT lists: {1: the weight, 2: the
    mapped key, 3: the docid}, computed from the inputs."""
    n_lists, nq, _ = rows_all.shape
    seen = set()
    for q in range(nq):
        wf = (int(rows_all[0, q, -1]) >> 4) & 3
        dec = [decode(rows_all[l, q]) for l in range(n_lists)]
        weight, mapped, docid = (np.concatenate([d[i] for d in dec]) for i in range(3))
        src = np.concatenate([np.full(len(d[0]), l) for l, d in enumerate(dec)])
        o = definition_order(weight, mapped, docid, wf)[:k + 1]
        for a, b in zip(o, o[1:]):
            if src[a] != src[b]:
                seen.add(1 if weight[a] != weight[b] else 2 if mapped[a] != mapped[b] else 3)
    return seen


def size_case(flavor, wf, n_lists, k, seed):
    rng = np.random.default_rng(seed)
    rows = np.zeros((n_lists, NQ, mdist().OROW_WORDS), np.uint64)
    for q, cnts in enumerate(counts_of(n_lists, k)):
        for l, c in enumerate(cnts):
            rows[l, q] = make_list(rng, flavor, wf, c, 1 + l * 2048 + q)
    return rows


SIZE_CASES = [(f, wf, n, k) for f, wf in FLAVORS for n in LISTS for k in KS]


@functools.lru_cache(maxsize=None)
def size_references():
    """{(flavor, wf, n_lists, k): (rows_all, expected)}, computed once"""
    ref = {}
    for i, (f, wf, n, k) in enumerate(SIZE_CASES):
        rows = size_case(f, wf, n, k, 7000 + i)
        ref[(f, wf, n, k)] = (rows, expected_merge(rows, k))
    return ref


@functools.lru_cache(maxsize=None)
def loud_cases():
    """[(name, rows_all [n_lists][NQ][W])]: every query of a case must come out
    MRK_ROW_DECLINED with zero count, zero keys and a zero plane; the odd list stands first / last / in the middle (query 0 / 1 / 2)."""
    d = mdist()
    out = []

    def build(name, n_lists, plan):
        rng = np.random.default_rng(zlib.crc32(f"wf/{name}/{n_lists}".encode()))
        rows = np.zeros((n_lists, NQ, d.OROW_WORDS), np.uint64)
        for q in range(NQ):
            for l in range(n_lists):
                rows[l, q] = plan(rng, l, l == (0, n_lists - 1, n_lists // 2)[q], 1 + l * 2048 + q)
        out.append((f"{name}/{n_lists}", rows))

    two = parts_of("two")
    attr_first = d.order_spec_word(two, 1)
    for n_lists in (2, 3, 5, 8):
        for bad_dir in (0, 3):  # every list carries the same spec, whose direction of the weight is none
            bad = (spec_of("two", 1) & ~(3 << 4)) | (bad_dir << 4)
            build(f"invalid-direction-{bad_dir}", n_lists, lambda rng, l, odd, d0, bad=bad: make_list(rng, "two", 1, 40, d0, spec=bad))
        # weight-first next to the same parts attribute-first (then_weight 1), either way round
        build("wfirst-next-to-attribute-first", n_lists, lambda rng, l, odd, d0: make_list(rng, "two", 1, 40, d0, spec=attr_first if odd else None))
        build("attribute-first-next-to-wfirst", n_lists, lambda rng, l, odd, d0: make_list(rng, "two", 1, 40, d0, spec=None if odd else attr_first))
        build("desc-next-to-asc", n_lists, lambda rng, l, odd, d0: make_list(rng, "one", 2 if odd else 1, 40, d0))
        # a shard whose planner declined sends MRK_ROW_DECLINED, no keys and spec 0
        build("declined-spec0", n_lists, lambda rng, l, odd, d0: make_list(rng, "int64", 2, 0, d0, flags=d.ROW_DECLINED, spec=0) if odd else make_list(rng, "int64", 2, 40, d0))
    return out


def assert_loud(d, rows_all, got, what):
    """every query: MRK_ROW_DECLINED, no count, no keys, a zero plane, totals carried, the other flag OR-ed through"""
    mask = d.ROW_RERUN | d.ROW_DECLINED
    for q in range(rows_all.shape[1]):
        tf = [int(x) for x in rows_all[:, q, K1 + 1]]
        assert int(got[q, K1 + 1]) & d.ROW_DECLINED, (what, q)
        assert int(got[q, K1 + 1]) & ~mask == sum(t & ~mask for t in tf), (what, q, "totals are carried")
        assert bool(int(got[q, K1 + 1]) & d.ROW_RERUN) == any(t & d.ROW_RERUN for t in tf), (what, q)
        assert int(got[q, K1]) == 0 and not got[q, :K1].any() and not got[q, K1 + 2:-1].any(), (what, q)


def wf_answer(orc, oi, q, rows, n_docs, expected_weight_first):
    """(rowid, weight, mapped keys, raw order keys or None, total) of a weight-first query on one index: the oracle + numpy"""
    rid, w, okey, total = expected_weight_first(orc, oi, q, rows, n_docs)
    mapped = np.zeros(len(rid), np.uint64) if okey is None else omc.map_order_np(okey, q.order)
    return rid, w, mapped, okey, total


def pack_wf_orow(rid, w, mapped, total, base, q):
    return omc.pack_orow(mdist(), rid.astype(np.int64) + base, w, total, query_spec(q), mapped)
