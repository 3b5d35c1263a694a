"""GPU: the merge of <= 8 exchange rows per query in its three row formats -- narrow (MRK_ROW_WORDS), wide (MRK_SROW_WORDS), order
(MRK_OROW_WORDS) -- on synthetic rows built on the host: no index.  Every entry point (mrk_topk_merge_rows / _srows / _orows and
their _part forms) must give WHOLE output rows equal to the numpy models dist.merge_srows_np / dist.merge_orows_np (the narrow
model: merge_srows_np over spec-0 rows, cut to the narrow width) -- keys, count, total | flags, mapped-key plane, spec word, zero
padding.  The shapes are the smallest at which the merge network can go wrong: 1, 2, 3, 5 and 8 lists (3 and 5 leave zero-padded
list slots, 8 needs the raised LDS limit), k = 1, 7 and 1024, lists of 0, 1, some and 1024 entries inside one query, a query
with fewer entries than k; every tie rule over few distinct mapped keys, order keys that differ in the low dword only; flagged
and declined lists in the two places where the formats elect the spec word differently; differing spec words."""
import numpy as np
import pytest

from merge_formats_common import FLAVORS, K1, KS, LISTS, NQ, SIZE_CASES, mdist, model, references, size_case, spec_of, words_of
from test_gpu_order_merge import Hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    hip = Hip()
    yield m, ctx, hip
    hip.free()
    ctx.close()


def entry(fmt, part=False):
    from manticoresearch_amd import _lib

    name = {"narrow": "mrk_topk_merge_rows", "wide": "mrk_topk_merge_srows", "order": "mrk_topk_merge_orows"}[fmt] + ("_part" if part else "")
    return getattr(_lib.lib(), name), _lib.check


def gpu_merge(ctx, hip, fmt, rows_all, k):
    n_lists, nq, W = rows_all.shape
    fn, chk = entry(fmt)
    src, dst = hip.malloc(rows_all.nbytes), hip.malloc(nq * W * 8)
    hip.to_dev(src, rows_all)
    hip.fill(dst, 0xEE, nq * W * 8)
    chk(fn(ctx._h, src, n_lists, nq, k, dst))
    return hip.to_host(dst, (nq, W))


def gpu_merge_part(ctx, hip, fmt, rows_all, k, stride, first, n_out):
    """rows_all [n_lists][nq][W] laid out with `stride` rows per list (the rows past nq hold 0xEE..), merged into rows
    [first, first + nq) of an output of n_out rows filled with 0xEE."""
    n_lists, nq, W = rows_all.shape
    recv = np.full((n_lists, stride, W), 0xEEEEEEEEEEEEEEEE, np.uint64)
    recv[:, :nq] = rows_all
    fn, chk = entry(fmt, part=True)
    src, dst = hip.malloc(recv.nbytes), hip.malloc(n_out * W * 8)
    hip.to_dev(src, recv)
    hip.fill(dst, 0xEE, n_out * W * 8)
    chk(fn(ctx._h, src, n_lists, stride, first, nq, k, dst))
    return hip.to_host(dst, (n_out, W))


@pytest.mark.parametrize("fmt,flavor,n_lists", SIZE_CASES)
def test_sizes_counts_and_orders(dev, fmt, flavor, n_lists):
    """Whole merged rows equal the model's at every list count, k and tie rule; the _part form writes the same rows at `first` and
    nothing else."""
    m, ctx, hip = dev
    for k in KS:
        rows, want = references()[("size", fmt, flavor, n_lists, k)]
        got = gpu_merge(ctx, hip, fmt, rows, k)
        assert np.array_equal(got, want), (fmt, flavor, n_lists, k, np.argwhere(got != want)[:4])
        part = gpu_merge_part(ctx, hip, fmt, rows, k, stride=NQ + 2, first=2, n_out=NQ + 3)
        assert np.array_equal(part[2:2 + NQ], want), (fmt, flavor, n_lists, k, "part")
        assert (part[:2] == np.uint64(0xEEEEEEEEEEEEEEEE)).all() and (part[2 + NQ:] == np.uint64(0xEEEEEEEEEEEEEEEE)).all()
        hip.free()


@pytest.mark.parametrize("fmt", list(FLAVORS))
def test_flags_and_spec_words(dev, fmt):
    """MRK_ROW_RERUN and MRK_ROW_DECLINED lists, declined as list 0 and as the last list (where the wide rule -- list 0's spec word,
    every list must agree -- and the order rule -- the first answering list's, declined lists have no say -- part ways), differing
    spec words, a sorted row next to a relevance row: whole rows as the format's own model gives them."""
    m, ctx, hip = dev
    d = mdist()
    seen = set()
    for key, (rows, wants) in references().items():
        if key[0] != "flags" or key[1] != fmt:
            continue
        for k, want in wants.items():
            got = gpu_merge(ctx, hip, fmt, rows, k)
            assert np.array_equal(got, want), (key, k, np.argwhere(got != want)[:4])
            part = gpu_merge_part(ctx, hip, fmt, rows, k, stride=NQ + 1, first=1, n_out=NQ + 2)
            assert np.array_equal(part[1:1 + NQ], want), (key, k, "part")
            assert (part[0] == np.uint64(0xEEEEEEEEEEEEEEEE)).all() and (part[-1] == np.uint64(0xEEEEEEEEEEEEEEEE)).all()
        hip.free()
        seen.add(key[2].split("/")[0])
    if fmt != "narrow":  # the two election rules do differ on these inputs, and each entry point keeps its own
        spec = spec_of(fmt, "tie1")
        want = references()[("flags", fmt, "declined-spec0/3")][1][1024]
        specs, declined = [int(w[-1]) for w in want], [bool(int(w[K1 + 1]) & d.ROW_DECLINED) for w in want]
        assert declined == [True] * 3 and not want[:, :K1 + 1].any()
        assert specs == ([0, spec, spec] if fmt == "wide" else [spec] * 3)
        assert {"spec-mismatch", "sorted-next-to-relevance", "relevance-next-to-sorted", "declined-spec0", "rerun-tie1"} <= seen


def test_relevance_rows_agree_across_the_formats(dev):
    """All-relevance rows: keys, count and total of the three formats' merges are the same words."""
    m, ctx, hip = dev
    d = mdist()
    for n_lists in LISTS:
        for k in KS:
            narrow = size_case("narrow", "rel", n_lists, k, 77 + n_lists)
            want = model("narrow", narrow, k)
            for fmt in ("narrow", "wide", "order"):
                rows = np.zeros((n_lists, NQ, words_of(fmt)), np.uint64)
                rows[..., :d.ROW_WORDS] = narrow
                got = gpu_merge(ctx, hip, fmt, rows, k)
                assert np.array_equal(got[:, :d.ROW_WORDS], want) and not got[:, d.ROW_WORDS:].any(), (fmt, n_lists, k)
            hip.free()


def test_second_device_raises_its_own_limit(dev):
    """An 8-list merge needs the kernel's dynamic LDS limit raised on the device it runs on: after device 0 has merged, a context on
    device 1 merges 8 narrow and 8 wide lists."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    m, ctx, hip = dev
    rows, want = references()[("size", "narrow", "rel", 8, 1024)]
    assert np.array_equal(gpu_merge(ctx, hip, "narrow", rows, 1024), want)  # device 0 first
    rows_w, want_w = references()[("size", "wide", "tie1", 8, 1024)]
    assert np.array_equal(gpu_merge(ctx, hip, "wide", rows_w, 1024), want_w)
    ctx1 = m.Context(1)
    hip1 = Hip()
    try:
        assert hip1.hip.hipSetDevice(1) == 0
        assert np.array_equal(gpu_merge(ctx1, hip1, "narrow", rows, 1024), want)
        assert np.array_equal(gpu_merge(ctx1, hip1, "wide", rows_w, 1024), want_w)
    finally:
        hip1.free()
        assert hip1.hip.hipSetDevice(0) == 0
        ctx1.close()
