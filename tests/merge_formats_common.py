"""The inputs and modelled outputs of tests/test_gpu_merge_formats.py, built on the host: synthetic exchange rows of the three formats
(narrow, wide, order) and what dist.merge_srows_np / dist.merge_orows_np make of them.  tests/test_order_merge_cpu.py runs every input
through its model without a GPU."""
import functools
import zlib

import numpy as np

K1 = 1024
NQ = 3
LISTS, KS = (1, 2, 3, 5, 8), (1, 7, 1024)
U32 = np.uint64(32)
LOW = np.uint64(0xFFFFFFFF)


def mdist():
    from manticoresearch_amd import dist

    return dist


def words_of(fmt):
    d = mdist()
    return {"narrow": d.ROW_WORDS, "wide": d.SROW_WORDS, "order": d.OROW_WORDS}[fmt]


def spec_of(fmt, flavor):
    """The spec word of a flavor: "rel" = relevance; "tie0/1/2" = sorted / ordered under that tie rule; "lowdw" = an order over two
    parts whose first part is constant; "sort" (order rows) = a one-part order, i.e. a sort."""
    import manticoresearch_amd as m

    d = mdist()
    if flavor == "rel":
        return 0
    if fmt == "wide":
        return d.sort_spec_word(0, True, int(flavor[3]), 2)
    if flavor == "sort":
        return d.order_spec_word([m.OrderPart(0, 2, desc=True)], 1)
    tie = 1 if flavor == "lowdw" else int(flavor[3])
    return d.order_spec_word([m.OrderPart(0, 2, desc=True), m.OrderPart(32, 4, desc=False)], tie)


def tie_of(spec):
    return (spec >> 4) & 3 if spec else 1


def make_list(rng, fmt, flavor, spec, count, docid0, total=None, flags=0):
    """One list's row: `count` entries with docids docid0 .. (distinct over a query's lists), in the order the merge keeps under
    `spec`; weights of 5 distinct values and mapped keys of 3, so that ties reach the weight and the docid."""
    d = mdist()
    row = np.zeros(words_of(fmt), np.uint64)
    docid = (rng.permutation(count) + docid0).astype(np.uint64)
    weight = rng.integers(1000, 1005, count).astype(np.uint64)
    keys = ((weight ^ np.uint64(0x80000000)) << U32) | (~docid & LOW)
    mk = np.zeros(count, np.uint64)
    if spec:
        if fmt == "wide":
            mk = rng.integers(7, 10, count).astype(np.uint64)
        elif flavor == "lowdw":
            mk = (np.uint64(5) << U32) | (~rng.integers(0, 3, count).astype(np.uint64) & LOW)
        elif flavor == "sort":
            mk = rng.integers(7, 10, count).astype(np.uint64) << U32
        else:
            mk = (rng.integers(7, 10, count).astype(np.uint64) << U32) | (~rng.integers(0, 2, count).astype(np.uint64) & LOW)
    w = (keys >> U32).astype(np.uint32)
    tie = tie_of(spec)
    wpart = w if tie == 1 else ~w if tie == 2 else np.zeros_like(w)
    order = np.lexsort((keys.astype(np.uint32), wpart, mk))[::-1]
    row[:count] = keys[order]
    row[K1] = count
    row[K1 + 1] = np.uint64((100_000 + docid0 if total is None else total) | flags)
    if fmt == "wide":
        plane = np.zeros(K1, "<u4")
        plane[:count] = mk[order].astype(np.uint32)
        row[d.SROW_MKEYS:d.SROW_SPEC] = plane.view("<u8")
        row[d.SROW_SPEC] = spec
    elif fmt == "order":
        row[d.OROW_MKEYS:d.OROW_MKEYS + count] = mk[order]
        row[d.OROW_SPEC] = spec
    return row


def model(fmt, rows_all, k):
    d = mdist()
    if fmt == "order":
        return d.merge_orows_np(rows_all, k)
    if fmt == "wide":
        return d.merge_srows_np(rows_all, k)
    wide = np.zeros(rows_all.shape[:2] + (d.SROW_WORDS,), np.uint64)  # spec 0, a zero plane
    wide[..., :d.ROW_WORDS] = rows_all
    out = d.merge_srows_np(wide, k)
    assert not out[:, d.ROW_WORDS:].any()
    return np.ascontiguousarray(out[:, :d.ROW_WORDS])


def counts_of(n_lists, k):
    """Per query, per list: q0 mixes 0, 1, a partial count and 1024; q1 holds fewer entries than k in all; q2 is full."""
    mix = [1024, 0, 1, 300, 1024, 517, 0, 1]
    have = min(k - 1, n_lists, 5)
    return [[mix[l] for l in range(n_lists)], [1 if l < have else 0 for l in range(n_lists)], [1024] * n_lists]


def size_case(fmt, flavor, n_lists, k, seed):
    rng = np.random.default_rng(seed)
    spec = spec_of(fmt, flavor)
    rows = np.zeros((n_lists, NQ, words_of(fmt)), np.uint64)
    for q, cnts in enumerate(counts_of(n_lists, k)):
        for l, c in enumerate(cnts):
            rows[l, q] = make_list(rng, fmt, flavor, spec, c, 1 + l * 2048 + q)
    return rows


FLAVORS = {"narrow": ("rel",), "wide": ("rel", "tie0", "tie1", "tie2"), "order": ("rel", "tie0", "tie1", "tie2", "lowdw")}
SIZE_CASES = [(fmt, fl, n) for fmt in FLAVORS for fl in FLAVORS[fmt] for n in LISTS]


def flag_cases(fmt):
    """[(name, rows_all [n_lists][NQ][W])]: flags and spec words.  Lists of 40 entries; every query of a case takes the same
    treatment at another list count (2, 3 and 5 lists would need three arrays: the case is built per list count instead)."""
    d = mdist()
    out = []
    srt = "tie1"
    other = "tie2"

    def build(name, n_lists, plan):
        # plan(l, n_lists) -> (flavor, count, flags) of list l
        rng = np.random.default_rng(zlib.crc32(f"{fmt}/{name}/{n_lists}".encode()))
        rows = np.zeros((n_lists, NQ, words_of(fmt)), np.uint64)
        for q in range(NQ):
            for l in range(n_lists):
                fl, c, flags = plan(l, n_lists, q)
                rows[l, q] = make_list(rng, fmt, fl, spec_of(fmt, fl), c, 1 + l * 2048 + q, flags=flags)
        out.append((f"{name}/{n_lists}", rows))

    kinds = ("rel",) if fmt == "narrow" else ("rel", srt)
    for n_lists in (2, 3, 5, 8):
        for base in kinds:
            # one list flagged MRK_ROW_RERUN (empty, as pack writes it), in a different place per query
            build(f"rerun-{base}", n_lists, lambda l, n, q, base=base: (base, 0, d.ROW_RERUN) if l == (q % n) else (base, 40, 0))
            # one list MRK_ROW_DECLINED carrying the others' spec word: as list 0, as the last list, in between
            build(f"declined-same-spec-{base}", n_lists,
                  lambda l, n, q, base=base: (base, 0, d.ROW_DECLINED) if l == (0, n - 1, n // 2)[q] else (base, 40, 0))
        if fmt == "narrow":
            continue
        # ... carrying spec 0, as a shard whose planner declined sends it: list 0 / the last list are where the two formats' rules differ
        build("declined-spec0", n_lists, lambda l, n, q: ("rel", 0, d.ROW_DECLINED) if l == (0, n - 1, n // 2)[q] else (srt, 40, 0))
        # two answering lists with different spec words (tie rule); a sorted row next to a relevance row (either first)
        build("spec-mismatch", n_lists, lambda l, n, q: (other if l == (0, n - 1, n // 2)[q] else srt, 40, 0))
        build("sorted-next-to-relevance", n_lists, lambda l, n, q: ("rel" if l == (0, n - 1, n // 2)[q] else srt, 40, 0))
        build("relevance-next-to-sorted", n_lists, lambda l, n, q: (srt if l == (0, n - 1, n // 2)[q] else "rel", 40, 0))
        if fmt == "order":
            build("sort-next-to-order", n_lists, lambda l, n, q: ("sort" if l == (0, n - 1, n // 2)[q] else srt, 40, 0))
    return out


@functools.lru_cache(maxsize=None)
def references():
    """Every case's input and its modelled output, computed once: {(kind, fmt, ...): (rows_all, {k: expected})}."""
    ref = {}
    for i, (fmt, fl, n) in enumerate(SIZE_CASES):
        for k in KS:
            rows = size_case(fmt, fl, n, k, 1000 + i)
            ref[("size", fmt, fl, n, k)] = (rows, model(fmt, rows, k))
    for fmt in FLAVORS:
        for name, rows in flag_cases(fmt):
            ref[("flags", fmt, name)] = (rows, {k: model(fmt, rows, k) for k in KS})
    return ref
