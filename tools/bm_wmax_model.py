"""tools/bm_wmax_model.py [--docs N] [--pairs P] [--out FILE] -- what the per-word weight bound of the two-bitmap AND kernel (ctx key
bm_wmax) can drop at best, computed on the host (numpy, no GPU) from a real synth_index with bench.py's corpus and cc pairs.

Per pair: the postings of both keywords are decoded from the doclists, every match is scored with score()'s fp32 operations, and the
exact K-th weight (K = 1000) is the threshold -- the FINAL one, from the first window on, which the kernel never has.  Then, per
match word (32 rowids), the bound of the kernel (the two keywords' largest-tf classes, Rmax = every field) and two variants that
say where the slack is: the same bound compared by weight instead of by pruning bin, and a bound that takes the fields the two
keywords' postings of the word really hold instead of Rmax.  A word survives when its bound reaches the threshold.  Counted: match
words, survivors, and the 128-byte lines of the slot-ordered tf / field plane (64 postings each) that the matches of all words /
of the surviving words touch.  Bytes are summed over the pairs like bench.py's algo_bytes_detail: two bitmaps per pair, the class
plane (1/8 of them), the lines x 128 B.  Prints one JSON object; the survival rate is what the measured
bm_words_queued / (queued + pruned) of tools/bm_wmax_rate.py is compared with."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

K = 1000
F32 = np.float32


def decode(spd: np.ndarray, e) -> tuple:
    """(rowid, tf, fields) of one keyword's doclist in the inline hit format: four VLB varints per doc (rowid delta, hits, then the
    inlined hit and its field word for one hit, or the field mask and the hitlist offset delta), big-endian base 128."""
    b = spd[int(e["doclist_off"]):int(e["doclist_off"]) + int(e["doclist_len"])].astype(np.uint64)
    end = (b & 0x80) == 0
    ends = np.nonzero(end)[0]
    starts = np.concatenate([[0], ends[:-1] + 1])
    group = np.cumsum(end) - end
    shift = (7 * (ends[group] - np.arange(b.size))).astype(np.uint64)
    vals = np.add.reduceat((b & 0x7F) << shift, starts)
    n = int(e["docs"])
    v = vals[:4 * n].reshape(n, 4)
    rowid = (np.cumsum(v[:, 0]) - 1).astype(np.int64)
    tf = v[:, 1].astype(np.int64)
    fields = np.where(tf == 1, np.uint64(1) << ((v[:, 3] >> np.uint64(1)) & np.uint64(255)), v[:, 2]).astype(np.int64)
    return rowid, tf, fields


def tfidf(tf: np.ndarray, idf: float) -> np.ndarray:
    fh = tf.astype(F32)
    return fh / (fh + F32(1.2)) * F32(idf)


def bound(cls: np.ndarray, idf: float) -> np.ndarray:
    """mrk::bm_wmax_bound (mrk_kcommon.h)"""
    if idf < 0:
        return np.full(cls.shape, tfidf(np.array([1]), idf)[0], F32)
    return np.where(cls == 15, F32(idf), tfidf(cls, idf)).astype(F32)


def weight(ta: np.ndarray, tb: np.ndarray, rank: np.ndarray) -> np.ndarray:
    acc = (F32(0.0) + ta) + tb
    return ((acc + F32(0.5)) * F32(1000.0)).astype(np.int32).astype(np.int64) + rank * 1000


def word_max(words: np.ndarray, x: np.ndarray, op) -> tuple:
    """per distinct word (ascending): op-reduction of x over the postings of the word"""
    first = np.concatenate([[0], np.nonzero(np.diff(words))[0] + 1])
    return words[first], op.reduceat(x, first)


def bins_of(idf_a: float, idf_b: float, n_fields: int) -> tuple:
    """bin_lo / bin_shift as bins_by_weight (mrk_plan.cpp) sets them for a pure AND under BM25 with default field weights"""
    lo = hi = 0.0
    for idf in (idf_a, idf_b):
        a0, a1 = idf / 2.2, idf
        lo += min(a0, a1)
        hi += max(a0, a1)
    bm_lo, bm_hi = int(np.floor((lo + 0.5) * 1000.0)) - 2, int(np.ceil((hi + 0.5) * 1000.0)) + 2
    wlo, whi = bm_lo + 1000, bm_hi + 1000 * n_fields
    sh = 0
    while sh < 31 and ((whi - wlo) >> sh) >= 1024:
        sh += 1
    return wlo, sh


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--pairs", type=int, default=256, help="cc pairs of the query file's first set(s)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import manticoresearch_amd as m

    c = bench.zipf_c()
    n_qsets = max(1, (bench.QUERY_FILE // 3) // 256)
    ranks, strata = bench.make_queries(c, n_qsets * 256)
    probs = [min(0.5, c / r) for r in ranks]
    n_fields = 2
    hi = m.synth_index(args.docs, probs, seed=bench.CORPUS_SEED, skiplist_block_size=128, n_threads=bench.usable_cpus())
    n_windows = (args.docs + 2047) // 2048
    cache = {}

    def postings(t):
        if t not in cache:
            if len(cache) > 48:
                cache.clear()
            cache[t] = decode(hi.spd, hi.dict[t])
            r = cache[t][0]
            assert r.size == int(hi.dict["docs"][t]) and r[-1] < args.docs and (np.diff(r) > 0).all() and cache[t][1].min() >= 1, t
        return cache[t]

    rows = []
    tot = {"bitmap": 0, "plane": 0, "lines_all": 0, "lines_kept": 0, "words": 0, "kept": 0, "kept_by_weight": 0, "kept_with_fields": 0}
    for a, b in strata["cc"][:args.pairs]:
        if hi.dict["docs"][a] > hi.dict["docs"][b]:
            a, b = b, a  # ExtMultiAnd_T node order
        ra, tfa, fa = postings(a)
        rb, tfb, fb = postings(b)
        idf_a, idf_b = (m.idf(int(hi.dict["docs"][t]), args.docs, n_qwords=2) for t in (a, b))
        _, ia, ib = np.intersect1d(ra, rb, assume_unique=True, return_indices=True)
        rank = np.array([bin(x).count("1") for x in range(256)], np.int64)[(fa[ia] | fb[ib]) & 255]
        w = weight(tfidf(tfa[ia], idf_a), tfidf(tfb[ib], idf_b), rank)
        kth = int(np.partition(w, w.size - K)[w.size - K]) if w.size >= K else None
        mw = ra[ia] >> 5
        words = np.unique(mw)
        # the classes and field unions of the match words, over ALL postings of the keyword in the word
        wa, ca = word_max(ra >> 5, np.minimum(tfa, 15), np.maximum)
        wb, cb = word_max(rb >> 5, np.minimum(tfb, 15), np.maximum)
        _, ua = word_max(ra >> 5, fa, np.bitwise_or)
        _, ub = word_max(rb >> 5, fb, np.bitwise_or)
        sa, sb = np.searchsorted(wa, words), np.searchsorted(wb, words)
        ta, tb = bound(ca[sa], idf_a), bound(cb[sb], idf_b)
        up = weight(ta, tb, np.full(words.size, n_fields, np.int64))
        up_f = weight(ta, tb, np.array([bin(x).count("1") for x in range(256)], np.int64)[(ua[sa] | ub[sb]) & 255])
        lo, sh = bins_of(idf_a, idf_b, n_fields)
        if kth is None:
            keep = keep_w = keep_f = np.ones(words.size, bool)
        else:
            keep = ((np.maximum(up - lo, 0)) >> sh) >= ((max(kth - lo, 0)) >> sh)
            keep_w = up >= kth
            keep_f = ((np.maximum(up_f - lo, 0)) >> sh) >= ((max(kth - lo, 0)) >> sh)
        kept_match = keep[np.searchsorted(words, mw)]
        lines_all = np.unique(ia >> 6).size + np.unique(ib >> 6).size
        lines_kept = np.unique(ia[kept_match] >> 6).size + np.unique(ib[kept_match] >> 6).size
        rows.append({"a": int(a), "b": int(b), "matches": int(w.size), "kth_weight": kth, "bin_shift": sh, "words": int(words.size),
                     "survive": round(float(keep.mean()), 5), "survive_by_weight": round(float(keep_w.mean()), 5),
                     "survive_with_word_fields": round(float(keep_f.mean()), 5), "lines_all": int(lines_all), "lines_kept": int(lines_kept)})
        tot["bitmap"] += 2 * n_windows * 256
        tot["plane"] += 2 * n_windows * 32
        tot["lines_all"] += lines_all
        tot["lines_kept"] += lines_kept
        tot["words"] += int(words.size)
        tot["kept"] += int(keep.sum())
        tot["kept_by_weight"] += int(keep_w.sum())
        tot["kept_with_fields"] += int(keep_f.sum())
    before = tot["bitmap"] + tot["lines_all"] * 128
    after = tot["bitmap"] + tot["plane"] + tot["lines_kept"] * 128
    out = {"docs": args.docs, "pairs": len(rows), "k": K,
           "survive": round(tot["kept"] / max(1, tot["words"]), 5),
           "survive_by_weight_not_bin": round(tot["kept_by_weight"] / max(1, tot["words"]), 5),
           "survive_with_word_fields_instead_of_rmax": round(tot["kept_with_fields"] / max(1, tot["words"]), 5),
           "survive_per_pair_min_max": [min(r["survive"] for r in rows), max(r["survive"] for r in rows)],
           "lines_kept_over_lines_all": round(tot["lines_kept"] / max(1, tot["lines_all"]), 5),
           "bytes_before": before, "bytes_after": after, "bytes_after_over_before": round(after / before, 4),
           "bytes": {"bitmaps": tot["bitmap"], "class_plane": tot["plane"], "plane_lines_before": tot["lines_all"] * 128, "plane_lines_after": tot["lines_kept"] * 128},
           "threshold": "the exact K-th weight of the whole pair, applied from the first word on", "per_pair": rows}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "per_pair"}))


if __name__ == "__main__":
    main()
