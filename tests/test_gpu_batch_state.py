"""GPU: state that outlives one submit, bit-exact against the oracle and against fresh batches.

A Batch keeps buffers, flags and lazily created sub-batches (the cutoff probe, the retry batch of mrk_batch_wait) from one
submit to the next, and bench.py drives long-lived batches two at a time with prepared query sets.  Here: match-queue
overflows and their reruns (ctx key mq_max_chunks; the rerun's device-side rows too), the generic evaluator's arena limits,
one batch fed a sequence of different submits forwards and backwards, overlapped submits the way bench.step() makes them,
bench's own corpus and settings at parity size, and the rows bench.py --dump-outputs writes.  Every comparison is bit-exact
on status, total_found, rowids and weights.

MRK_BENCH_DOCS sets the docs of the bench-sized corpora (default 2 M)."""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import synth_postings
from test_gpu_parity import kw, orc_index_of, to_orc
from test_gpu_wide_fields import query_mix, wide_corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_DOCS = int(os.environ.get("MRK_BENCH_DOCS", 2_000_000))
KCAP, RW = 1024, 1026  # MRK_MAX_K, MRK_ROW_WORDS
ROW_DECLINED = 1 << 62
# the context defaults (mrk_host_int.h) of the keys these tests change
DEFAULTS = {"mq_max_chunks": 1 << 22, "gen_spill_mb": 1024, "gen_lane_hits": 256, "prox_prune": 1, "bt_cover_inv": 1024,
            "prox_bound_keywords": 0}
PROBS = [0.9, 0.7, 0.5, 0.3, 0.15, 0.05]


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    hip = C.CDLL("libamdhip64.so")
    rows = C.c_void_p()
    assert hip.hipMalloc(C.byref(rows), C.c_size_t(256 * RW * 8)) == 0
    yield m, ctx, hip, rows
    hip.hipFree(rows)
    ctx.close()


class Settings:
    """ctx.set() for the block, the defaults back afterwards whatever happens."""

    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set(k, DEFAULTS[k])


def oracle_all(orc, hi, queries, oi=None):
    """The oracle's answer to every query (C calls on a thread pool: ctypes releases the GIL)."""
    oi = oi or orc_index_of(orc, hi)
    cidx = oi.c_struct()
    flat = [to_orc(orc, q) for q in queries]
    with ThreadPoolExecutor(max(1, min(16, orc.usable_cpus()))) as ex:
        return list(ex.map(lambda f: f.run(oi, cidx), flat))


def same(a, b, what=""):
    assert a.status == b.status, (what, a.status, b.status)
    assert a.total_found == b.total_found, (what, a.total_found, b.total_found)
    assert np.array_equal(a.rowid, b.rowid), (what, a.rowid[:8], b.rowid[:8])
    assert np.array_equal(a.weight, b.weight), (what, a.weight[:8], b.weight[:8])


def same_all(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, (what, i))


def vs_oracle(got, want, what="", allow_declined=False):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if allow_declined and g.status != 0:
            continue
        assert g.status == 0, (what, i, g.status)
        assert g.total_found == w.total_found, (what, i, g.total_found, w.total_found)
        assert np.array_equal(g.rowid, w.rowid), (what, i, g.rowid[:8], w.rowid[:8])
        assert np.array_equal(g.weight, w.weight), (what, i, g.weight[:8], w.weight[:8])


def check_device_rows(dev, batch, got, rowid_base=0):
    """The batch's device-side results (mrk_batch_device_results, and the rows mrk_batch_export_rows writes) hold what
    results() handed back: a rerun query's repaired row, no stale flag or declined mark of an earlier submit."""
    m, ctx, hip, buf = dev
    from manticoresearch_amd import _lib

    n = len(got)
    kp, cp, tp = batch.device_results()
    keys, cnt, tot = np.zeros((n, KCAP), np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    for host, ptr in ((keys, kp), (cnt, cp), (tot, tp)):
        assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(host.nbytes), 2) == 0
    _lib.check(_lib.lib().mrk_batch_export_rows(batch._h, buf))
    rows = np.zeros((n, RW), np.uint64)
    assert hip.hipMemcpy(C.c_void_p(rows.ctypes.data), buf, C.c_size_t(rows.nbytes), 2) == 0
    for i, g in enumerate(got):
        if g.status != 0:
            assert int(rows[i, RW - 1]) & ROW_DECLINED, i
            continue
        k = len(g.rowid)
        want = ((g.weight.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64) << np.uint64(32)) | \
            (~(g.rowid + np.uint32(rowid_base))).astype(np.uint64)
        assert int(cnt[i]) == k and int(tot[i]) == g.total_found, (i, int(cnt[i]), k, int(tot[i]), g.total_found)
        assert np.array_equal(keys[i, :k], want), i
        assert int(rows[i, KCAP]) == k and int(rows[i, KCAP + 1]) == g.total_found, (i, int(rows[i, KCAP]), hex(int(rows[i, KCAP + 1])))
        assert np.array_equal(rows[i, :k], want) and not rows[i, k:KCAP].any(), i


def fresh_search(m, ctx, seg, queries, n_max=64):
    b = m.Batch(ctx, max(n_max, len(queries)))
    try:
        return b.search(seg, queries)
    finally:
        b.close()


# ------------------------------------------------------------------ corpora and query mixes
_CORPORA = {}


def narrow_corpus(m):
    """3 fields, end flags on each word's last hit in a field (end_markers=1), short fields: phrases and NEAR match often."""
    if "narrow" not in _CORPORA:
        _CORPORA["narrow"] = m.synth_index(500_000, PROBS, seed=0x5EED0101, n_fields=3, max_pos=24, end_markers=1)
    return _CORPORA["narrow"]


def wide_synth_corpus(m):
    """20 fields (the WIDE kernel instances), end flags where the reference's indexer puts them (end_markers=2)."""
    if "wide" not in _CORPORA:
        _CORPORA["wide"] = m.synth_index(300_000, PROBS, seed=0x5EED0102, n_fields=20, max_pos=24, end_markers=2)
    return _CORPORA["wide"]


def bench_corpus(m, docs):
    """bench.py's main corpus (synth_index defaults: two fields, no end flags) and its query strata, one set of 256 per stratum."""
    key = ("bench", docs)
    if key not in _CORPORA:
        import bench

        c = bench.zipf_c()
        ranks, strata = bench.make_queries(c, 256)
        probs = [min(0.5, c / r) for r in ranks]
        hi = m.synth_index(docs, probs, seed=bench.CORPUS_SEED)
        _CORPORA[key] = (hi, strata, c)
    return _CORPORA[key]


def bench_mkq(m, hi, docs, K=1000):
    gd = hi.dict["docs"].astype(np.int64)

    def mkq(a, b):  # bench.main's mkq
        return m.Query(m.XQNode.AND(kw(m, a, 1), kw(m, b, 2)), ranker=m.SPH_RANK_BM25, max_matches=K, total_docs=int(docs),
                       local_docs={a: int(gd[a]), b: int(gd[b])})

    return mkq, gd


def hit_mix(m, rng, nt, n_fields, with_cutoff=True):
    """Hit-ranked queries for all three match queues: [0] AND / OR / ANDNOT trees, [1] root PHRASE, "a b"~N, BEFORE, NEAR,
    [2] the generic evaluator (a 5-word phrase, a NOTNEAR over a phrase, a NEAR over 3 operands: the probe launch);
    attribute filters, weight filters and a cutoff ride along."""
    top = n_fields - 1
    masks = [0xFFFFFFFF] * 6 + [0b110, 1 << top]
    P = m.SPH_RANK_PROXIMITY_BM25
    qs = []

    def k(t, pos):
        return kw(m, t, pos, int(rng.choice(masks)))

    for rk in (P, m.SPH_RANK_SPH04, m.SPH_RANK_MATCHANY):
        for _ in range(2):
            a, b, c = (int(x) for x in rng.choice(nt, 3, replace=False))
            qs.append(m.Query(m.XQNode.AND(k(a, 1), k(b, 2)), ranker=rk))
            qs.append(m.Query(m.XQNode.AND(m.XQNode(m.SPH_QUERY_OR, [k(a, 1), k(b, 2)]), k(c, 3)), ranker=rk))
            qs.append(m.Query(m.XQNode(m.SPH_QUERY_ANDNOT, [m.XQNode.AND(k(a, 1), k(b, 2)), kw(m, c, 3)]), ranker=rk))
    for rk in (P, m.SPH_RANK_SPH04):
        a, b = (int(x) for x in rng.choice(nt, 2, replace=False))
        qs.append(m.Query(m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, a, 1), kw(m, b, 2)]), ranker=rk))
        qs.append(m.Query(m.XQNode(m.SPH_QUERY_PROXIMITY, [kw(m, a, 1), kw(m, b, 2)], opt=3), ranker=rk))
        qs.append(m.Query(m.XQNode(m.SPH_QUERY_BEFORE, [kw(m, a, 1), kw(m, b, 2)]), ranker=rk))
        qs.append(m.Query(m.XQNode(m.SPH_QUERY_NEAR, [kw(m, a, 1), kw(m, b, 2)], opt=3), ranker=rk))
    for rk in (P, m.SPH_RANK_MATCHANY):
        a, b, c = (int(x) for x in rng.choice(nt, 3, replace=False))
        qs.append(m.Query(m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, int(t), i + 1) for i, t in enumerate(rng.permutation(nt)[:5])]), ranker=rk))
        qs.append(m.Query(m.XQNode(m.SPH_QUERY_NOTNEAR, [kw(m, a, 1), m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, b, 2), kw(m, c, 3)])], opt=3), ranker=rk))
        qs.append(m.Query(m.XQNode(m.SPH_QUERY_NEAR, [kw(m, a, 1), kw(m, b, 2), kw(m, c, 3)], opt=4), ranker=rk))
    for i, q in enumerate(qs):
        q.max_matches = [1000, 20, 300][i % 3]
        if i % 4 == 1:
            q.filters = [m.Filter(0, 32, values=[0, 2, 3])]
        if i % 5 == 2:
            q.weight_filters = [m.Filter(0, 32, min=1500, max=1 << 30)]
        q.field_weights = [int(x) for x in rng.integers(1, 30, n_fields)] if i % 2 else None
    if with_cutoff:  # (not on the NEAR over 3 operands: the device declines a cutoff there)
        for j, cut in ((0, 50), (13, 7), (len(qs) - 2, 300)):
            qs[j].weight_filters, qs[j].cutoff = None, cut
    return qs


def attrs_of(hi):
    return (np.arange(hi.total_docs, dtype=np.uint32) % 5).reshape(-1, 1)


def segment(m, ctx, hi, rowid_base=0, oi=None):
    seg = m.Segment(ctx, hi, rowid_base=rowid_base)
    a = attrs_of(hi)
    seg.set_attrs(a)
    if oi is not None:
        oi.attrs = a
    return seg


# ------------------------------------------------------------------ 1. match-queue overflow reruns
@pytest.mark.parametrize("corpus", ["narrow", "wide"])
def test_match_queue_overflow_reruns(orc, dev, corpus):
    m, ctx, hip, buf = dev
    hi = narrow_corpus(m) if corpus == "narrow" else wide_synth_corpus(m)
    oi = orc_index_of(orc, hi)
    qs = hit_mix(m, np.random.default_rng(31 if corpus == "narrow" else 32), len(PROBS), hi.n_fields)
    seg = segment(m, ctx, hi, oi=oi)
    want = oracle_all(orc, hi, qs, oi)
    batch = m.Batch(ctx, len(qs))
    try:
        for prune in (0, 1):
            for cover in (1024, 0):  # bitmap-word trees / block trees
                with Settings(ctx, prox_prune=prune, bt_cover_inv=cover):
                    base = batch.search(seg, qs)
                    assert batch.stats()["n_rerun"] == 0
                    vs_oracle(base, want, ("default cap", prune, cover))
                    for cap in (1, 3, 64):
                        with Settings(ctx, mq_max_chunks=cap):
                            got = batch.search(seg, qs)
                            n_rerun = batch.stats()["n_rerun"]
                        same_all(got, base, ("cap", cap, prune, cover))
                        vs_oracle(got, want, ("cap", cap, prune, cover))
                        check_device_rows(dev, batch, got)
                        print(f"{corpus} prune={prune} cover={cover} cap={cap}: {n_rerun} of {len(qs)} queries rerun")
                        if cap == 1:  # (not every query: those whose work items ran before the queue filled up fit)
                            assert n_rerun >= 1
                    # and the default cap again on the same batch
                    same_all(batch.search(seg, qs), base, ("default cap again", prune, cover))
                    assert batch.stats()["n_rerun"] == 0
                    check_device_rows(dev, batch, base)
    finally:
        batch.close()
        seg.close()


# ------------------------------------------------------------------ 2. the generic evaluator's arena limits
def test_gen_arena_limits_fail_loudly_then_recover(orc, dev):
    """The smallest arena (gen_lane_hits=16, gen_spill_mb=1) against docs whose keywords hold ~100 hits each: a 5-word phrase and
    a 5-keyword AND either come back right or fail with the gen_spill_mb message -- never a wrong answer with status 0; with the
    defaults back, the same batch answers them right."""
    m, ctx, hip, buf = dev
    from manticoresearch_amd import _lib

    n_docs, n_terms, per = 6000, 5, 100
    rows = np.repeat(np.arange(n_docs, dtype=np.uint32), per)
    W, R, H = [], [], []
    for t in range(n_terms):  # term t at positions t+1, t+6, ...: "t0 t1 t2 t3 t4" is a phrase 100 times per doc
        W.append(np.full(n_docs * per, t + 1, np.uint64))
        R.append(rows)
        H.append(np.tile((np.uint32(1) << 24) | (np.arange(per, dtype=np.uint32) * n_terms + t + 1), n_docs))
    hi = m.index_from_hits(np.concatenate(W), np.concatenate(R), np.concatenate(H), n_terms=n_terms, total_docs=n_docs, n_fields=2)
    qs = [m.Query(m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, t, t + 1) for t in range(n_terms)]), ranker=m.SPH_RANK_PROXIMITY_BM25),
          m.Query(m.XQNode.AND(*[kw(m, t, t + 1) for t in range(n_terms)]), ranker=m.SPH_RANK_PROXIMITY_BM25, max_matches=50)]
    want = oracle_all(orc, hi, qs)
    seg = m.Segment(ctx, hi)
    batch = m.Batch(ctx, 8)
    try:
        n_failed = 0
        for q, w in zip(qs, want):
            with Settings(ctx, gen_lane_hits=16, gen_spill_mb=1):
                batch.submit(seg, [q])
                batch.wait()
                err = _lib.lib().mrk_last_error().decode(errors="replace")
                g = batch.results()[0]
            if g.status != 0:
                assert "gen_spill_mb" in err, err
                n_failed += 1
            else:
                vs_oracle([g], [w], "small arena")
            vs_oracle(batch.search(seg, [q]), [w], "defaults again")
        assert n_failed >= 1  # (6000 docs x 500 hits do not fit in 1 MB: the limit was met)
        vs_oracle(batch.search(seg, qs), want, "both, defaults")
    finally:
        batch.close()
        seg.close()


# ------------------------------------------------------------------ 3. one batch, many different submits
def test_batch_reuse_sequence_forwards_and_backwards(orc, dev):
    m, ctx, hip, buf = dev
    rng = np.random.default_rng(33)
    nt = len(PROBS)
    P, B = m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_BM25
    narrow = narrow_corpus(m)
    wide, nt_wide = wide_corpus(m, 20, 128, 1, True, seed=36)
    W, R, H = synth_postings(rng, 50_000, PROBS, n_fields=3, max_pos=20, end_markers=True)
    based = m.index_from_hits(W, R, H, n_terms=nt, total_docs=50_000, n_fields=3)
    segs = {"narrow": (narrow, 0), "wide": (wide, 0), "based": (based, 500_000)}  # (a shard that holds rows 500000 ..)

    def pair():
        return (int(x) for x in rng.choice(nt, 2, replace=False))

    def triple():
        return (int(x) for x in rng.choice(nt, 3, replace=False))

    def c3(i):
        a, b, c = triple()
        ka, kb, kc = kw(m, a, 1), kw(m, b, 2), kw(m, c, 3)
        return [m.XQNode.AND(ka, kb, kc), m.XQNode.AND(m.XQNode(m.SPH_QUERY_OR, [ka, kb]), kc), m.XQNode.AND(ka, m.XQNode(m.SPH_QUERY_OR, [kb, kc])),
                m.XQNode(m.SPH_QUERY_ANDNOT, [m.XQNode.AND(ka, kb), kc])][i % 4]

    headline = [m.Query(m.XQNode.AND(*(kw(m, t, j + 1) for j, t in enumerate(pair()))), ranker=B) for _ in range(64)]
    config3 = [m.Query(c3(i), ranker=P) for i in range(64)]
    phrases = []
    for i in range(40):
        a, b, c = triple()
        words = [kw(m, a, 1), kw(m, b, 2)] + ([kw(m, c, 3)] if i % 3 == 0 else [])
        phrases.append(m.Query(m.XQNode(m.SPH_QUERY_PHRASE if i % 2 else m.SPH_QUERY_PROXIMITY, words, opt=0 if i % 2 else 4),
                               ranker=[P, m.SPH_RANK_SPH04, B][i % 3], max_matches=[1000, 30][i % 2]))
    gen = []
    for i in range(24):
        a, b, c = triple()
        perm = [int(t) for t in rng.permutation(nt)]
        root = [m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, t, j + 1) for j, t in enumerate(perm[:5])]),
                m.XQNode(m.SPH_QUERY_NEAR, [kw(m, a, 1), kw(m, b, 2), kw(m, c, 3)], opt=int(rng.integers(2, 8))),
                m.XQNode.AND(*[kw(m, t, j + 1) for j, t in enumerate(perm[:5])]),
                m.XQNode(m.SPH_QUERY_NOTNEAR, [kw(m, a, 1), m.XQNode(m.SPH_QUERY_PHRASE, [kw(m, b, 2), kw(m, c, 3)])], opt=3)][i % 4]
        gen.append(m.Query(root, ranker=[P, m.SPH_RANK_MATCHANY, m.SPH_RANK_WORDCOUNT][i % 3], max_matches=[100, 1000][i % 2]))
    declined = []
    for i in range(32):
        q = m.Query(c3(i) if i % 2 else m.XQNode.AND(*(kw(m, t, j + 1) for j, t in enumerate(pair()))), ranker=[P, B][i % 2])
        if i % 5 == 1:
            q.cutoff = 1025  # past the device's top-K: declined
        elif i % 7 == 3:
            q.cutoff, q.weight_filters = 5, [m.Filter(0, 32, min=0, max=1 << 30)]  # a cutoff next to a weight filter: declined
        declined.append(q)
    clean = [m.Query(q.root, ranker=q.ranker) for q in declined]
    cutoffs = [m.Query(q.root, ranker=q.ranker, max_matches=[20, 1000][i % 2], cutoff=[1, 7, 100, 1000][i % 4],
                       filters=[m.Filter(0, 32, values=[1, 4])] if i % 3 == 0 else None) for i, q in enumerate(config3[:12] + [g for j, g in enumerate(gen[:12]) if j % 4 != 1] + headline[:4])]
    overflow = hit_mix(m, np.random.default_rng(34), nt, 3)
    wide_q = query_mix(m, np.random.default_rng(35), nt_wide, 20, with_filters=True)[::5][:64]
    based_q = headline[:24] + config3[:24]

    seq = [("narrow", headline, {}), ("narrow", config3, {}), ("narrow", phrases, {}), ("narrow", gen, {}), ("narrow", declined, {}),
           ("narrow", clean, {}), ("narrow", cutoffs, {}), ("narrow", overflow, {"mq_max_chunks": 1}), ("wide", wide_q, {}),
           ("based", based_q, {}), ("narrow", config3[:8], {}), ("narrow", headline, {})]
    seg_objs, ois = {}, {}
    batch = m.Batch(ctx, 64)
    try:
        for k, (hi, base) in segs.items():
            ois[k] = orc_index_of(orc, hi)
            seg_objs[k] = segment(m, ctx, hi, base, ois[k])
        expect = []
        for k, qs, kv in seq:
            want = oracle_all(orc, segs[k][0], qs, ois[k])
            with Settings(ctx, **kv):
                ref = fresh_search(m, ctx, seg_objs[k], qs)
            vs_oracle(ref, want, ("fresh", k, len(qs)), allow_declined=True)
            expect.append(ref)
        assert sum(r.status != 0 for r in expect[4]) >= 6 and all(r.status == 0 for r in expect[5])
        for order in (range(len(seq)), reversed(range(len(seq)))):
            for i in order:
                k, qs, kv = seq[i]
                with Settings(ctx, **kv):
                    got = batch.search(seg_objs[k], qs)
                    if kv:
                        assert batch.stats()["n_rerun"] >= 1
                same_all(got, expect[i], ("reused", i))
                check_device_rows(dev, batch, got, segs[k][1])
    finally:
        batch.close()
        for s in seg_objs.values():
            s.close()


# ------------------------------------------------------------------ 4. overlapped submits, bench-style
def test_overlapped_prepared_submits(orc, dev):
    """Kinds side by side, each cycling through four prepared query sets: headline BM25 ANDs and config-3 trees on bench's
    corpus, a query mix on a 20-field segment.  2, then 4 sets of batches in flight: a step submits its batches and then
    collects the set n_sets steps back (bench.step()).  Every collected result equals the synchronous one; three cycles give
    the same bytes."""
    m, ctx, hip, buf = dev
    import bench

    docs = BENCH_DOCS
    hi, strata, _ = bench_corpus(m, docs)
    mkq, gd = bench_mkq(m, hi, docs)
    wide = wide_synth_corpus(m)
    pairs = [p for trip in zip(strata["cc"], strata["sc"], strata["ss"]) for p in trip]
    queries = {"bm25": [[mkq(a, b) for a, b in pairs[k * 64:(k + 1) * 64]] for k in range(4)],
               "c3": [bench.config3_queries(m, strata, 256, 1000, docs, gd)[k * 64:(k + 1) * 64] for k in range(4)],
               "wide": [query_mix(m, np.random.default_rng(40), len(PROBS), 20, with_filters=False)[k * 64:(k + 1) * 64] for k in range(4)]}
    his = {"bm25": hi, "c3": hi, "wide": wide}
    seg_main, seg_wide = m.Segment(ctx, hi), m.Segment(ctx, wide)
    segs = {"bm25": seg_main, "c3": seg_main, "wide": seg_wide}
    kinds = list(queries)
    prepared = {k: [m.prepare(qs) for qs in queries[k]] for k in kinds}
    batches = {}
    try:
        with Settings(ctx, prox_bound_keywords=1):  # bench's setting (neither corpus carries a per-word end flag)
            sync = {}
            for k in kinds:
                oi = orc_index_of(orc, his[k])
                sync[k] = []
                for qk in range(4):
                    ref = fresh_search(m, ctx, segs[k], queries[k][qk])
                    vs_oracle(ref, oracle_all(orc, his[k], queries[k][qk], oi), ("sync", k, qk))
                    sync[k].append(ref)
            batches = {n_sets: [{k: m.Batch(ctx, 64) for k in kinds} for _ in range(n_sets)] for n_sets in (2, 4)}
            cycles = []
            for cycle in range(3):
                out = []
                for n_sets, sets in batches.items():
                    pending = []

                    def collect(idx, qk):
                        for k in kinds:
                            sets[idx][k].wait()
                            got = sets[idx][k].results()
                            same_all(got, sync[k][qk], ("overlapped", cycle, n_sets, k, qk))
                            out.extend(r.rowid.tobytes() + r.weight.tobytes() + np.int64([r.total_found, r.status]).tobytes() for r in got)

                    for step in range(10):
                        idx, qk = step % n_sets, step % 4
                        for k in kinds:
                            sets[idx][k].submit_prepared(segs[k], prepared[k][qk], 64)
                        pending.append((idx, qk))
                        while len(pending) >= n_sets:
                            collect(*pending.pop(0))
                    while pending:
                        collect(*pending.pop(0))
                cycles.append(b"".join(out))
            assert cycles[0] == cycles[1] == cycles[2]
    finally:
        for sets in batches.values():
            for s in sets:
                for b in s.values():
                    b.close()
        seg_main.close()
        seg_wide.close()


# ------------------------------------------------------------------ 5. bench's settings at parity size
def alternating(m, ctx, seg, cq, n, reps=4):
    """bench's config-3 / config-5 loop: two batches, one waits while the other is in flight; every collected result set."""
    bs = [m.Batch(ctx, n), m.Batch(ctx, n)]
    out, busy = [], [False, False]
    try:
        for i in range(reps):
            b = bs[i % 2]
            if busy[i % 2]:
                b.wait()
                out.append(b.results())
            b.submit_prepared(seg, cq, n)
            busy[i % 2] = True
        for j, b in enumerate(bs):
            if busy[j]:
                b.wait()
                out.append(b.results())
    finally:
        for b in bs:
            b.close()
    return out


def test_bench_settings_at_parity_size(orc, dev):
    m, ctx, hip, buf = dev
    import bench

    docs = BENCH_DOCS
    hi, strata, c = bench_corpus(m, docs)
    mkq, gd = bench_mkq(m, hi, docs)
    K = 1000
    oi = orc_index_of(orc, hi)
    seg = m.Segment(ctx, hi)
    try:
        with Settings(ctx, prox_bound_keywords=1):
            for s in ("cc", "sc", "ss"):
                qs = [mkq(a, b) for a, b in strata[s]]
                want = oracle_all(orc, hi, qs, oi)
                for got in alternating(m, ctx, seg, m.prepare(qs), len(qs)):
                    vs_oracle(got, want, s)
            c3 = bench.config3_queries(m, strata, 256, K, docs, gd)
            want = oracle_all(orc, hi, c3, oi)
            runs = alternating(m, ctx, seg, m.prepare(c3), len(c3))
            for got in runs:
                vs_oracle(got, want, "config3")
            with Settings(ctx, prox_prune=0):
                same_all(fresh_search(m, ctx, seg, c3, 256), runs[0], "config3 unpruned")
        same_all(fresh_search(m, ctx, seg, c3, 256), runs[0], "config3 bound by hits")
    finally:
        seg.close()
    # config 5 as bench.config5_leg builds it (its own corpus: 4 fields, end flags where the reference's indexer puts them)
    ranks5, strata5 = bench.make_queries(c, 342)
    hi5 = m.synth_index(docs, [min(0.5, c / r) for r in ranks5], seed=bench.CORPUS_SEED + 5, n_fields=4, end_markers=2)
    gd5 = hi5.dict["docs"].astype(np.int64)
    qs5 = bench.config5_queries(m, strata5, 1024, K, docs, gd5, (10, 5, 2, 1))
    seg5 = m.Segment(ctx, hi5)
    try:
        with Settings(ctx, prox_bound_keywords=1):
            runs = alternating(m, ctx, seg5, m.prepare(qs5), 1024)
        for got in runs[1:]:
            same_all(got, runs[0], "config5 repeat")
        assert all(r.status == 0 for r in runs[0])
        same_all(fresh_search(m, ctx, seg5, qs5, 1024), runs[0], "config5 bound by hits")
        with Settings(ctx, prox_prune=0):
            same_all(fresh_search(m, ctx, seg5, qs5, 1024), runs[0], "config5 unpruned")
        vs_oracle(runs[0][::4], oracle_all(orc, hi5, qs5[::4]), "config5")
    finally:
        seg5.close()


# ------------------------------------------------------------------ 6. what the timed path returns
def test_bench_dump_outputs_match_oracle(orc, dev, tmp_path):
    m = dev[0]
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--docs", "2000000", "--queries", "256", "--query-file", "768", "--warmup", "1",
           "--steps", "2", "--no-config3", "--no-config5", "--no-cpu-baseline", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    hi, strata, _ = bench_corpus(m, 2_000_000)
    mkq, _ = bench_mkq(m, hi, 2_000_000)
    oi = orc_index_of(orc, hi)
    n_checked = 0
    for s in ("cc", "sc", "ss"):
        arr = {k: np.load(out_dir / f"{s}_{k}.npy") for k in ("rowid", "weight", "count", "total_found", "status", "query")}
        sel = arr["query"].astype(np.int64)
        assert len(sel) == len(arr["count"]) and len(sel) > 0
        want = oracle_all(orc, hi, [mkq(*strata[s][i]) for i in sel], oi)  # --query-file 768: one set, every step runs set 0
        ends = np.cumsum(arr["count"].astype(np.int64))
        assert ends[-1] == len(arr["rowid"]) == len(arr["weight"])
        for j, w in enumerate(want):
            lo, hi_ = ends[j] - int(arr["count"][j]), ends[j]
            assert arr["status"][j] == 0, (s, j)
            assert int(arr["total_found"][j]) == w.total_found, (s, j, arr["total_found"][j], w.total_found)
            assert np.array_equal(arr["rowid"][lo:hi_], w.rowid.astype(np.float64)), (s, j)
            assert np.array_equal(arr["weight"][lo:hi_], w.weight.astype(np.float64)), (s, j)
            n_checked += 1
    assert n_checked == 3 * 256
