"""GPU: the two-bitmap AND kernel's weight bound tested against a per-threshold cutoff (bm_wmax_cut, csrc/mrk_kcommon.h).

A wave of scan_bm_kernel's WMAX instances no longer evaluates `weight_bin((bmw + rmax1000) * index_weight) < tau_bin` for every match
word: it keeps the smallest bmw that passes, worked out again when its threshold bin has moved, and compares.  Results must not move:
status, total_found, rowids and weights are bit-equal between a segment with the plane, one without (bm_wmax=0: the kernel's untouched
instances) and the oracle -- for groups of 4 / 3 / 2 / 1 queries and a lone one, K = 10 and 1000, index weights 1 and 7, field weights
(3, -2, 0) and (1, 1, 1), and a set whose weights are all negative (negative idfs, negative field weights), where the cutoff's T <= 0
branch runs.  The corpus is test_gpu_bm_wmax's: 150 001 docs (74 windows, no multiple of 2048), keywords with negative idf, the planted
rows, the 300-tf escape.  bm_words_pruned shows that the cutoff drops words where a threshold exists; no exact counts, they depend on
when thresholds arrive."""
import pytest

from test_gpu_bm_wmax import AND, FAT, ROW_15, ROW_255, ROW_BEST, corpus, dev, grouped, oracle, plain, run  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


def sets_of(m, k, fw, iw):
    """The grouped set (groups of 4, 3, 2 and 1) with the planted pair, and a query that is alone in its batch."""
    return grouped(m, k, fw, iw) + [AND(m, 6, 7, k=k, fw=fw, iw=iw), AND(m, FAT, 6, k=k, fw=fw, iw=iw)], [AND(m, 2, 4, k=k, fw=fw, iw=iw)]


@pytest.mark.parametrize("iw", [1, 7])
@pytest.mark.parametrize("fw", [(3, -2, 0), (1, 1, 1)])
def test_results_do_not_move(orc, dev, plain, fw, iw):
    m, ctx, batch = dev
    pair, oi = plain
    for k in (10, 1000):
        for qs in sets_of(m, k, list(fw), iw):
            want = oracle(orc, oi, qs)
            st = run(dev, pair, qs, want)
            assert st["bm_words_queued"] > 0, st
            # K = 10 with more matches than K: a threshold forms, and words of tf-1 postings lie behind it
            if k == 10 and all(w.total_found > 10 * k for w in want):
                assert st["bm_words_pruned"] > 0, (k, fw, iw, st)
    if (fw, iw) == ((1, 1, 1), 1):
        want = oracle(orc, oi, [AND(m, 6, 7, k=10)])
        assert list(want[0].rowid[:3]) == [ROW_255, ROW_15, ROW_BEST]


@pytest.mark.parametrize("iw", [1, 7])
def test_all_weights_negative(orc, dev, plain, iw):
    """Keywords 0 and 1 have negative idfs and every field weight is negative: every weight, and with them bin_lo and the
    threshold T = bin_lo + (tau_bin << bin_shift) of the first bins, is negative.  (The bound adds no field weight then, the
    matches' own sums are -1000 and less: the bound is loose, so only the results are checked, not that words were dropped.)"""
    m, ctx, batch = dev
    pair, oi = plain
    fw = [-3, -2, -1]
    for k in (10, 1000):
        qs = [AND(m, 0, 1, k=k, fw=fw, iw=iw), AND(m, 1, 0, k=k, fw=fw, iw=iw)]
        want = oracle(orc, oi, qs)
        assert all(w.total_found > 1000 and w.weight[0] < 0 for w in want)
        st = run(dev, pair, qs, want)
        assert st["bm_words_queued"] > 0, st
        lone = [AND(m, 1, 0, k=k, fw=fw, iw=iw)]
        run(dev, pair, lone, oracle(orc, oi, lone))


def test_ineligible_shapes_count_nothing(orc, dev, plain):
    m, ctx, batch = dev
    pair, oi = plain
    qs = [AND(m, 0, 2, k=10, ranker=m.SPH_RANK_NONE), AND(m, 2, 3, k=1000, ranker=m.SPH_RANK_NONE, iw=7), AND(m, 0, 2, k=10, mask=(1, 0xFFFFFFFF)),
          AND(m, 4, 5, k=10, mask=(0xFFFFFFFF, 6), fw=[3, -2, 0], iw=7)]
    st = run(dev, pair, qs, oracle(orc, oi, qs))
    assert st["bm_words_pruned"] == 0 and st["bm_words_queued"] == 0, st
