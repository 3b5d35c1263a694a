"""GPU: the sorted top-K selection (csrc/mrk_sortsel.hip: sort_select_kernel -- the streaming pass over the 128-bit candidates, the
compaction sortsel_compact with its bitonic sort, the bin filter cand_bin) at its edges: rank K on the last row of a key class and
the first of the next, classes several buffers long whose best rows arrive last, columns of exactly 1023 / 1024 / 1025 key values
and of the whole 32 and 64 bits, keys on either side of every bin boundary, bit-fields, float zeros and edges, INT64 and two-part
keys, the weight in front, candidate lists of CAND - WG - 1 .. CAND + 1 entries, a segment that ends at rowid 2^32 - 1, every layout
in one launch, and the rows the kernel writes itself.  Small deterministic corpora (tests/sortsel_edges_common.py);
tests/test_sortsel_edges_cpu.py asserts on the CPU that each has the structure its case names and that the planner gives the geometry
it relies on.

Every result is bit-exact against the numpy models of the sorter's order (sorted_expect.py, weight_first_expect.py) applied to the
oracle's full match list: status, rowids in order, weights, the raw sort_key / order_key as the host rows hold them, total_found.
Every batch is searched twice and must give the same bytes.  packed == 1, n_rerun == 0 (no list here comes near 2^20 slots), and
n_cands >= the matches that tie the expected K-th row on the binned quantity, summed over the batch: they share its bin under any
monotone bin map, so the scan must have listed them all."""
import contextlib

import numpy as np
import pytest

import manticoresearch_amd as m
import sortsel_edges_common as sc

pytestmark = pytest.mark.gpu

PRODUCERS = {"bm25": m.SPH_RANK_BM25, "proximity_bm25": m.SPH_RANK_PROXIMITY_BM25}  # scan_pk's sort instance / rank_kernel's


@pytest.fixture(scope="module")
def corpora(orc):
    return sc.Corpora(m, orc)


@contextlib.contextmanager
def device(hi, rows, max_queries, rowid_base=0):
    """one context, segment (with its attribute rows) and batch, closed whatever happens"""
    ctx = m.Context(0)
    seg = batch = None
    try:
        seg = m.Segment(ctx, hi, rowid_base=rowid_base)
        seg.set_attrs(rows)
        batch = m.Batch(ctx, max_queries)
        yield ctx, seg, batch
    finally:
        if batch is not None:
            batch.close()
        if seg is not None:
            seg.close()
        ctx.close()


def same_bytes(a, b):
    return (a.status == b.status and a.total_found == b.total_found and a.rowid.tobytes() == b.rowid.tobytes() and a.weight.tobytes() == b.weight.tobytes()
            and all((x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes())
                    for x, y in ((a.sort_key, b.sort_key), (a.order_key, b.order_key), (a.group_key, b.group_key), (a.group_count, b.group_count))))


def check_one(what, i, q, g, want):
    rid, w, key, total = want
    assert g.status == 0, (what, i, g.status)
    assert g.total_found == total, (what, i, g.total_found, total)
    n = min(len(rid), len(g.rowid))
    assert np.array_equal(g.rowid, rid), (what, i, q.sort, q.order, q.max_matches, len(g.rowid), len(rid), np.flatnonzero(g.rowid[:n] != rid[:n])[:4], g.rowid[:4], rid[:4])
    assert np.array_equal(g.weight, w), (what, i, q.sort, q.order, q.max_matches, g.weight[:4], w[:4])
    got_key = g.sort_key if q.sort is not None else g.order_key
    assert (g.order_key if q.sort is not None else g.sort_key) is None, (what, i)
    if key is None:
        assert got_key is None, (what, i)  # (weight ASC alone: no part of the row is in the order)
    else:
        assert got_key is not None and got_key.dtype == key.dtype and np.array_equal(got_key, key), (what, i, q.sort, q.order, q.max_matches)


def run(what, corpora, name, seg, batch, queries):
    """search twice; every result against the model on the oracle's full list; packed, no rerun, n_cands >= the ties' floor"""
    wants = [corpora.want(name, q) for q in queries]
    floor = sum(corpora.floor(name, q, w) for q, w in zip(queries, wants))
    got = batch.search(seg, queries)
    st = batch.stats()
    again = batch.search(seg, queries)
    for i, (q, g, a, want) in enumerate(zip(queries, got, again, wants)):
        check_one(what, i, q, g, want)
        assert same_bytes(g, a), (what, i, "second search differs")
    assert st["packed"] == 1 and st["n_rerun"] == 0, (what, st["packed"], st["n_rerun"])
    print("%s: %d queries, n_cands %d floor %d scan %.3f ms" % (what, len(queries), st["n_cands"], floor, st["scan_ms"]))
    assert st["n_cands"] >= floor, (what, st["n_cands"], floor)
    return got


# ------------------------------------------------------------------ 1: key ladders
@pytest.mark.parametrize("weights", ["even", "high"])
@pytest.mark.parametrize("producer", list(PRODUCERS))
def test_key_ladders(corpora, producer, weights):
    """Key classes of 300 / 500 / 7392 rows at low, high and evenly spread rowids under three weight classes placed independently:
    rank K as the last row of a class, the first of the next and, ascending, inside a class more than four buffers long; with
    then_weight 1 the heavy rows keep beating the running threshold after every compaction (weights "high": they arrive last)."""
    name = ("S", weights)
    hi, oi, rows = corpora.get(*name)
    qs = sc.case1(m, PRODUCERS[producer])
    with device(hi, rows, len(qs)) as (ctx, seg, batch):
        run(f"ladders {producer} {weights}", corpora, name, seg, batch, qs)


# ------------------------------------------------------------------ 2: one key, one bin
@pytest.mark.parametrize("producer", list(PRODUCERS))
def test_one_key_one_bin(corpora, producer):
    """A constant column: span 0, every match in bin 0, all 8192 pass the filter; the tie rule and the rowid decide alone."""
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    qs = sc.case2(m, PRODUCERS[producer])
    with device(hi, rows, len(qs)) as (ctx, seg, batch):
        got = run(f"const {producer}", corpora, name, seg, batch, qs)  # (the floor is every match of every query: nothing can be pruned)
    k1024 = [g for q, g in zip(qs, got) if q.max_matches == 1024 and q.sort.then_weight == 0]
    assert k1024 and all(g.rowid.tolist() == [4 * i for i in range(1024)] for g in k1024)


# ------------------------------------------------------------------ 3: bin geometry
def test_bin_geometry(corpora):
    """FULL32 (shift 22, keys on either side of every bin boundary), SPAN1023 / 1024 / 1025 (where the shift goes from 0 to 1 and the bin
    clamps at 1023), BAND (a sliver of a 32-bit range: every match in ONE bin, the K-th key's class 7 or 8 rows)."""
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    qs = sc.case3(m)
    with device(hi, rows, len(qs)) as (ctx, seg, batch):
        run("geometry", corpora, name, seg, batch, qs)
        band = [q for q in qs if q.sort.bit_offset == sc.BAND * 32]
        run("band", corpora, name, seg, batch, band)
        assert batch.stats()["n_cands"] >= len(band) * sc.S_MATCHES  # the threshold bin holds every match (the CPU test: one bin)


# ------------------------------------------------------------------ 4: bit-fields
def test_bit_fields(corpora):
    """1 bit at bit 31, 1 bit at bit 0, 31 bits at bit 1, 5 bits at bit 27, noise in the dwords' other bits."""
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    qs = sc.case4(m)
    with device(hi, rows, len(qs)) as (ctx, seg, batch):
        run("bit-fields", corpora, name, seg, batch, qs)


# ------------------------------------------------------------------ 5: floats
def test_float_zeros_and_edges(corpora):
    """-0.0 and +0.0 interleaved by rowid are ONE key: rank K inside the merged class falls through to the tie rule and the rowid, and
    every row leaves with its own bits; +-inf, +-FLT_MAX and the denormals at either end; both directions."""
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    qs = sc.case5(m)
    with device(hi, rows, len(qs)) as (ctx, seg, batch):
        got = run("floats", corpora, name, seg, batch, qs)
    both = [g for q, g in zip(qs, got) if q.max_matches == 1024 and (q.sort.bit_offset == sc.FLTD * 32) == q.sort.desc]
    assert both and all({0, 0x80000000} <= set(g.sort_key.tolist()) for g in both)


# ------------------------------------------------------------------ 6: INT64 and two parts
def test_int64_and_two_parts(corpora):
    """One INT64 column that cycles INT64_MIN, INT64_MAX and the values around 0 and +-2^31 (the low dword compares unsigned under a
    signed high dword; K = 911 is the last row of the best class); two-part orders over (CAT4, FULL32), (FULL32, CAT4), (CONST, SPAN1024),
    second parts of range 255 and 256 (nb 8 and 9), (1 bit at bit 31, float), in equal and opposite directions."""
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    qs = sc.case6(m)
    with device(hi, rows, len(qs)) as (ctx, seg, batch):
        run("orders", corpora, name, seg, batch, qs)


# ------------------------------------------------------------------ 7: weight-first
@pytest.mark.parametrize("weights", ["plain", "fallback", "negative"])
def test_weight_first(corpora, weights):
    """The weight in front, both directions, over no part, LAD ascending, the INT64 column and (CAT4, SPAN1024): under weight ASC the class
    of 7392 rows leads and fills one bin, under DESC the heavy rows arrive last.  fallback: field weights that leave bins_by_weight with
    bin_lo = INT32_MIN and shift 31.  negative: every weight below zero, also behind the key of a plain sort (then_weight 1 and 2)."""
    name = ("S", "high")
    hi, oi, rows = corpora.get(*name)
    qs = sc.case7(m) if weights == "plain" else sc.case7(m, field_weights=list(sc.FALLBACK_FIELD_WEIGHTS)) if weights == "fallback" else sc.case7_negative(m)
    with device(hi, rows, len(qs)) as (ctx, seg, batch):
        got = run(f"weight first {weights}", corpora, name, seg, batch, qs)
        if weights == "fallback":
            assert batch.stats()["n_cands"] >= len(qs) * sc.S_MATCHES  # one bin holds every match (the CPU test: bin_lo INT32_MIN, shift 31)
    assert all(((g.weight < 0).all() if weights == "negative" else (g.weight > 0).all()) for g in got)


# ------------------------------------------------------------------ 8: list lengths
def test_list_lengths(corpora):
    """Candidate lists of 1, WG - 1 .. WG + 1, CAND - WG - 1 .. CAND - WG + 1 (the compaction trigger), CAND - 1 .. CAND + 1 and 2 CAND + 1
    entries, back to back in one batch, under a constant column (every entry passes the bin filter) and under distinct values; two
    queries that match nothing answer status 0, no rows, total 0."""
    name = ("L",)
    hi, oi, rows = corpora.get(*name)
    qs = sc.case8(m)
    with device(hi, rows, len(qs)) as (ctx, seg, batch):
        got = run("list lengths", corpora, name, seg, batch, qs)
        const = [q for q in qs[:-2] if q.sort.bit_offset == sc.L_CONST * 32]
        run("list lengths, constant", corpora, name, seg, batch, const)
        assert batch.stats()["n_cands"] >= 2 * sum(sc.LIST_COUNTS)  # whole lists: these are the lengths the kernel streams
    for g in got[-2:]:
        assert g.status == 0 and g.total_found == 0 and len(g.rowid) == 0 and len(g.weight) == 0 and len(g.sort_key) == 0


# ------------------------------------------------------------------ 9: rowid base
@pytest.mark.parametrize("base", sc.S_BASES, ids=["ends_at_2p32", "straddles_2p31"])
def test_rowid_base(corpora, base):
    """The segment's last rowid is 2^32 - 1, or 2^31 lies in its middle (the low word's ~rowid dword changes its top bit inside every
    key class): ~global rowid in either half of the candidate's low word (a sort's, a weight-first order's)."""
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    qs = sc.case9(m)
    with device(hi, rows, len(qs), rowid_base=base) as (ctx, seg, batch):
        run("rowid base", corpora, name, seg, batch, qs)


# ------------------------------------------------------------------ 10: one launch, every layout
def test_every_layout_in_one_launch(corpora):
    """Sort, one-part order, INT64 order, two-part order, weight-first, relevance and grouped queries interleaved so that each kind
    stands next to each other one (blocks of sort_on == 0 queries return early): every answer equals the one of a batch of its own."""
    name = ("S", "even")
    hi, oi, rows = corpora.get(*name)
    seq, qs = sc.case10(m)
    with device(hi, rows, len(qs)) as (ctx, seg, batch):
        got = batch.search(seg, qs)
        assert batch.stats()["packed"] == 1 and batch.stats()["n_rerun"] == 0
        again = batch.search(seg, qs)
        solo = {}
        for i, (kind, q, g, a) in enumerate(zip(seq, qs, got, again)):
            assert g.status == 0 and same_bytes(g, a), (i, kind)
            if (kind, q.max_matches) not in solo:
                solo[kind, q.max_matches] = batch.search(seg, [q])[0]
                if kind < 5:
                    check_one("solo", i, q, solo[kind, q.max_matches], corpora.want(name, q))
            assert same_bytes(g, solo[kind, q.max_matches]), (i, kind, q.max_matches)
        assert len(solo) == 7 * 3
        assert all(g.group_key is not None and len(g.rowid) == min(4, q.max_matches) and g.total_found == 4 for kind, q, g in zip(seq, qs, got) if kind == 6)
        assert all(g.group_key is None and g.sort_key is None and g.order_key is None and len(g.rowid) == q.max_matches for kind, q, g in zip(seq, qs, got) if kind == 5)


# ------------------------------------------------------------------ 11: rows the kernel writes itself
@pytest.mark.parametrize("kind", ["srows", "orows"])
def test_standing_rows_equal_the_export(corpora, kind):
    """A standing wide / order-row destination selects sort_select_kernel<DST_WIDE> / <DST_ORDER>: its rows equal, word for word, the
    rows exported from the same batch without a standing destination (orows_weight_first on: the weight-first queries answer in order
    rows; in wide rows they, and the 64-bit keys, leave declined either way)."""
    from test_gpu_order_merge import Hip
    from test_gpu_row_kinds import export, lib_of, words

    name = ("S", "high")
    hi, oi, rows = corpora.get(*name)
    qs = sc.case1(m, m.SPH_RANK_BM25, placements=("high",))[::4] + sc.case6(m)[::3] + sc.case7(m)[::3]
    n, wd = len(qs), words(m, kind)
    lib, chk = lib_of()
    hip = Hip()
    try:
        with device(hi, rows, n) as (ctx, seg, batch):
            batch.orows_weight_first(True)
            got = batch.search(seg, qs)
            assert [g.status for g in got] == [0] * n and batch.stats()["n_rerun"] == 0
            for i, (q, g) in enumerate(zip(qs, got)):
                check_one("before the standing rows", i, q, g, corpora.want(name, q))
            exported = export(m, hip, batch, kind, n)
            dst = hip.malloc(n * wd * 8)
            hip.fill(dst, 0xEE, n * wd * 8)
            chk(getattr(lib, f"mrk_batch_set_{kind}_dst")(batch._h, dst))
            again = batch.search(seg, qs)
            assert batch.stats()["n_rerun"] == 0 and all(same_bytes(a, g) for a, g in zip(again, got))
            standing = hip.to_host(dst, (n, wd))
            chk(getattr(lib, f"mrk_batch_set_{kind}_dst")(batch._h, None))
            for i in range(n):
                assert np.array_equal(standing[i], exported[i]), (kind, i, qs[i].sort, qs[i].order, np.flatnonzero(standing[i] != exported[i])[:4])
            from manticoresearch_amd import dist as mdist

            declined = [bool(int(r[sc.KCAP + 1]) & mdist.ROW_DECLINED) for r in standing]
            wide_key = [q.order is not None and (q.order.weight_first != 0 or len(q.order.parts) == 2 or q.order.parts[0].kind == m.SORTKEY_INT64) for q in qs]
            assert declined == ([False] * n if kind == "orows" else wide_key) and not all(declined)
            assert all(int(r[sc.KCAP]) == (0 if d else len(g.rowid)) for r, d, g in zip(standing, declined, got))
    finally:
        hip.free()
