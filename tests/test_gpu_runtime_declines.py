"""GPU: what the device path only finds out while a query runs -- a doc with more live phrase states than a kernel keeps (QF_FSM),
the generic evaluator out of hit-list memory (QF_ARENA) -- at and around the caps, bit-exact against the oracle where the query is
answered, loud where it is not, and never a flagless or a stale exchange row: "never hand back a silently truncated result"
(mrk_batch_wait), "MRK_ROW_DECLINED: ... the merged row is not an answer" (include/mrk.h).

Every corpus is hand-made (runtime_declines_common.py: a few hundred docs), every query a hand-made tree with explicit query
positions; rowids, weights and total_found come from the CPU oracle, merged rows from the numpy models of dist.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import runtime_declines_common as rd
from runtime_declines_common import ARENA, LIVE_STATES, Settings
from test_gpu_batch_state import oracle_all
from test_gpu_order_merge import Hip
from test_gpu_parity import kw, orc_index_of
from test_gpu_sort_merge import L

pytestmark = pytest.mark.gpu

K1 = 1024
UNSUPPORTED = -2


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    hip = Hip()
    yield m, ctx, hip
    hip.free()
    ctx.close()


def last_error():
    return L()[0].mrk_last_error().decode(errors="replace")


def exact(g, w, what):
    """True = answered.  An answer (status 0) that differs from the oracle fails here, first and with its own message, whatever else
    the caller allows for the query."""
    if g.status == 0:
        assert g.total_found == w.total_found, (what, "status 0, total_found differs", g.total_found, w.total_found)
        assert np.array_equal(g.rowid, w.rowid), (what, "status 0, rowids differ", g.rowid[:8], w.rowid[:8])
        assert np.array_equal(g.weight, w.weight), (what, "status 0, weights differ", g.weight[:8], w.weight[:8])
    return g.status == 0


def loud(g, what):
    assert g.status == UNSUPPORTED and len(g.rowid) == 0 and g.total_found == 0, (what, g.status, len(g.rowid), g.total_found)


def one(batch, seg, q):
    """One query alone: (result, the message behind its status)"""
    batch.submit(seg, [q])
    batch.wait()
    err = last_error()
    return batch.results()[0], err


# ------------------------------------------------------------------ 1. the specialised phrase path at PHRASE_STATES
SMALL_CONFIGS = [{}, {"bt_phrase": 0}, {"bitmap_inv": 0}, {"bt_cover_inv": 0}]


@pytest.mark.parametrize("block,fmt", [(128, 1), (32, 0)])
def test_phrases_up_to_span_7_are_answered_whatever_the_runs(orc, dev, block, fmt):
    """The planner takes a phrase for the specialised kernels while its atoms span < PHRASE_STATES = 8 positions (mrk_plan.cpp,
    build_tree) -- a promise that 8 slots suffice.  A run of the first word at r consecutive positions keeps min(r, span) + 1 states
    busy when the slot of a state that cannot match any more is taken first, one more when it is not: span 7 behind a run of 9
    is the cap.  Every gap 1..7 and both 3-word phrases of span 7, under BM25 and PROXIMITY_BM25, at the root and under an AND,
    on the bitmap-word and the block-walk kernels, with and without dead rows: status 0 and the oracle's rowids, weights and
    total_found.

    With more live states than slots the kernel raises QF_FSM (mrk_khits.h, hit_pass).  Below span 8 that cannot happen, so this
    site is not reachable through a query the planner hands to these kernels, and no input is made up for it.  What stands in:
    span 8 never reaches them.  Where the generic evaluator is at hand (the packed path) it answers the query, exactly; where it
    is not (ctx path = 1) the planner's own decline stands, with its message."""
    m, ctx, hip = dev
    H, n_docs = rd.small_gap_corpus()
    assert n_docs < 400 and len(H) < 5000
    hi = H.index(m, 4, n_docs, block=block, fmt=fmt)
    qs, spans = rd.small_gap_queries(m)
    assert max(spans) == 7 and spans.count(7) == 12
    span8 = [m.Query(rd.PHRASE(m, kw(m, rd.A, 1), kw(m, rd.B, 9)), ranker=rk) for rk in (m.SPH_RANK_BM25, m.SPH_RANK_PROXIMITY_BM25)]
    oi = orc_index_of(orc, hi)
    dead = rd.dead_map(n_docs, range(3, n_docs, 7))
    want = {False: oracle_all(orc, hi, qs + span8, oi)}
    oi.dead_rows = dead
    want[True] = oracle_all(orc, hi, qs + span8, oi)
    assert sum(w.total_found for w in want[False][:len(qs)]) > sum(w.total_found for w in want[True][:len(qs)]) > 100  # the phrases do occur
    batch = m.Batch(ctx, len(qs) + 2)
    try:
        for cfg in SMALL_CONFIGS:
            with Settings(ctx, **cfg):
                seg = m.Segment(ctx, hi)  # (bitmap_inv is read when the segment loads)
                try:
                    for with_dead in (False, True):
                        seg.set_dead_rows(dead if with_dead else None)
                        batch.submit(seg, qs + span8)
                        batch.wait()
                        err = last_error()
                        got = batch.results()
                        assert batch.stats()["packed"] == 1
                        for i, (g, w) in enumerate(zip(got, want[with_dead])):
                            what = (cfg, "dead rows" if with_dead else "", i, "span", (spans + [8, 8])[i])
                            answered = exact(g, w, what)
                            assert answered, (what, g.status, err)
                finally:
                    seg.close()
        with Settings(ctx, path=1):  # the VLB path: no generic evaluator behind the specialised planner
            seg = m.Segment(ctx, hi)
            try:
                for q, w in zip(span8, want[False][len(qs):]):
                    g, err = one(batch, seg, q)
                    loud(g, "span 8, path 1")
                    assert "phrase spans 8 positions (device path: < 8)" in err, err
                for i in (24, 26):  # the span-7 phrases there: whatever that path does with a phrase, not a state overflow and not a wrong answer
                    g, err = one(batch, seg, qs[i])
                    if not exact(g, want[False][i], ("span 7, path 1", i)):
                        loud(g, "span 7, path 1")
                        assert LIVE_STATES not in err, err
            finally:
                seg.close()
    finally:
        batch.close()


# ------------------------------------------------------------------ 2. the generic evaluator at GEN_FSM_STATES
def test_generic_phrases_at_the_state_cap(orc, dev):
    """Phrases of five words, and two phrases under an OR, run through the generic per-doc evaluator (mrk_keval.h), whose phrase node
    keeps GEN_FSM_STATES = 32 live states.  build_gen (mrk_plan.cpp) sets no limit on a phrase's span -- only ascending positions
    and 2..8 words -- so the cap is met at run time: w0 at r consecutive positions under a first gap g keeps min(r - 1, g) states
    live when the next w0 arrives.  That is 32 for g >= 32 and r >= 33, and for nothing else: every g < 32 must be answered whatever
    the run, g = 32 behind a run of 32 too; (g, r) = (40, 64) must be declined by the cap alone.  A declined query says "more live
    phrase states", has no rows and total_found 0; an answered one equals the oracle.

    QF_FSM's raising sites in mrk_keval.h: the phrase node (these queries); the proximity node for query positions spanning more
    than 32, a property of the query alone -- '"w0 .. w4"~3' over 33 positions is declined, over 32 answered; the NEAR chain's
    insert, which fails at 16 operands, and a NEAR takes 8 (MRK_MAX_AND_TERMS): not reachable, no input is made up for it.

    The healthy queries in front of and behind a declining one are answered exactly, and with the tripping docs dead the same
    batch answers all of them exactly on its next submit."""
    m, ctx, hip = dev
    H, n_docs, cases, healthy = rd.wide_gap_corpus()
    assert n_docs < 400 and len(H) < 5000
    hi = H.index(m, 7, n_docs)
    oi = orc_index_of(orc, hi)
    P = m.SPH_RANK_PROXIMITY_BM25
    all_trip = [r for rows in cases.values() for r in rows]
    seg = m.Segment(ctx, hi)
    batch = m.Batch(ctx, 8)
    n_declined, n_answered = 0, 0
    try:
        for (g, r), rows in cases.items():
            qs = [rd.healthy_and(m), m.Query(rd.phrase5(m, 30), ranker=P), m.Query(rd.phrase5(m, g), ranker=P), m.Query(rd.or_phrases(m, g), ranker=m.SPH_RANK_BM25),
                  m.Query(rd.phrase5(m, g), ranker=m.SPH_RANK_BM25, max_matches=3), rd.healthy_and(m, max_matches=5)]
            under_test = (2, 3, 4)
            dead = rd.dead_map(n_docs, [x for x in all_trip if x not in rows])
            oi.dead_rows = dead
            want = oracle_all(orc, hi, qs, oi)
            seg.set_dead_rows(dead)
            batch.submit(seg, qs)
            batch.wait()
            err = last_error()
            got = batch.results()
            must_answer = g < 32 or r <= 32
            for i, (gq, w) in enumerate(zip(got, want)):
                what = ("g", g, "r", r, "query", i)
                answered = exact(gq, w, what)
                if i not in under_test or must_answer:
                    assert answered, (what, gq.status, err)
                elif not answered:
                    loud(gq, what)
                    assert LIVE_STATES in err, (what, err)
                    n_declined += 1
                n_answered += answered and i in under_test
            if (g, r) == (40, 64):
                assert [got[i].status for i in under_test] == [UNSUPPORTED] * 3, ("33 first words in a row under a gap of 40: 32 live states", [x.status for x in got])
            if any(got[i].status != 0 for i in under_test):  # the same batch, the tripping docs dead: every query exact
                oi.dead_rows = rd.dead_map(n_docs, all_trip)
                seg.set_dead_rows(oi.dead_rows)
                again = batch.search(seg, qs)
                for i, (gq, w) in enumerate(zip(again, oracle_all(orc, hi, qs, oi))):
                    assert exact(gq, w, ("tripping docs dead", g, r, i)), (g, r, i, gq.status)
        assert want[1].total_found > 0 and n_answered >= 3 * 9 and n_declined >= 3
        # the proximity node: 32 slots for the query positions
        oi.dead_rows = None
        seg.set_dead_rows(None)
        for qlen, must in ((31, True), (32, False), (44, False)):
            q = m.Query(rd.prox5(m, qlen), ranker=P)
            g_, err = one(batch, seg, q)
            w = oracle_all(orc, hi, [q], oi)[0]
            assert w.total_found > 0 or qlen != 31
            if not exact(g_, w, ("proximity over", qlen + 1, "positions")):
                assert not must, (qlen, g_.status, err)
                loud(g_, ("proximity", qlen))
                assert LIVE_STATES in err, err
            elif qlen == 44:
                raise AssertionError("query positions 1..45 do not fit 32 slots: the proximity node must decline")
            # ... and the batch is whole again on the next submit
            assert exact(batch.search(seg, [rd.healthy_and(m)])[0], oracle_all(orc, hi, [rd.healthy_and(m)], oi)[0], "behind a proximity decline")
    finally:
        batch.close()
        seg.close()


# ------------------------------------------------------------------ 3. run-time declines in the three exchange-row formats
class Rows:
    """The three formats' entry points and a device buffer per use"""

    def __init__(self, m, hip, fmt, nq):
        from manticoresearch_amd import dist as mdist

        lib, self.chk = L()
        kind = {"narrow": "rows", "wide": "srows", "order": "orows"}[fmt]
        self.fmt, self.nq, self.hip, self.mdist = fmt, nq, hip, mdist
        self.W = rd.words_of(mdist, fmt)
        self.set_dst = getattr(lib, f"mrk_batch_set_{kind}_dst")
        self.export_fn = getattr(lib, f"mrk_batch_export_{kind}")
        self.merge_fn = getattr(lib, f"mrk_topk_merge_{kind}")

    def buffer(self, n_lists=1):
        p = self.hip.malloc(n_lists * self.nq * self.W * 8)
        self.hip.fill(p, 0xEE, n_lists * self.nq * self.W * 8)
        return p

    def host(self, p, n_lists=None):
        return self.hip.to_host(p, (self.nq, self.W) if n_lists is None else (n_lists, self.nq, self.W))

    def export(self, batch):
        p = self.buffer()
        self.chk(self.export_fn(batch._h, p))
        return self.host(p)

    def merge(self, ctx, lists, k):
        src, out = self.buffer(len(lists)), self.buffer()
        self.hip.to_dev(src, np.stack(lists))
        self.chk(self.merge_fn(ctx._h, src, len(lists), self.nq, k, out))
        return self.host(out)


@pytest.fixture(scope="module")
def row_expectations(orc):
    """Per trigger: the corpus, the queries, and every format's rows from the oracle -- each segment's, the unsplit corpus', and the
    healthy batch's (the declining queries replaced).  Computed once, read by every test below."""
    import manticoresearch_amd as m
    from manticoresearch_amd import dist as mdist

    out = {}
    for trigger in ("fsm", "arena"):
        c = rd.row_corpus(m, trigger)
        assert c.n_docs < 500 and (trigger == "arena" or sum(int(h.dict["hits"].sum()) for h in c.his) < 5000)
        qs, declining = rd.row_queries(m, c)
        healthy_qs, _ = rd.row_queries(m, c, with_declining=False)
        exp = {}
        for fmt in rd.FORMATS:
            per_seg = [rd.expected_rows(mdist, orc, fmt, c.his[s], qs, declining, c.seg_rows(s), c.bases[s]) for s in (0, 1)]
            per_seg[1] = rd.expected_rows(mdist, orc, fmt, c.his[1], qs, [], c.seg_rows(1), c.bases[1])  # (nothing trips in segment 1)
            exp[fmt] = {"seg": per_seg, "whole": rd.expected_rows(mdist, orc, fmt, c.whole, qs, declining, c.rows, 0),
                        "healthy": rd.expected_rows(mdist, orc, fmt, c.his[0], healthy_qs, [], c.seg_rows(0), 0)}
        out[trigger] = (c, qs, declining, healthy_qs, exp)
    return out


def trigger_settings(ctx, trigger):
    return Settings(ctx, gen_lane_hits=16, gen_spill_mb=1) if trigger == "arena" else Settings(ctx)


@pytest.mark.parametrize("fmt", rd.FORMATS)
@pytest.mark.parametrize("trigger", ["fsm", "arena"])
def test_declined_rows_standing_exported_merged_and_resubmitted(dev, row_expectations, trigger, fmt):
    """A query that met QF_FSM / QF_ARENA, by relevance, sorted and ordered, between healthy queries, in one format:
    - the standing row, read once the stream has drained and before the host has looked, is flagged (MRK_ROW_RERUN or
      MRK_ROW_DECLINED), holds no keys, count 0 and a zero plane;
    - after mrk_batch_wait the query's status is MRK_E_UNSUPPORTED with the trigger's message, and the exported rows -- all of them,
      every word -- are the rows the oracle's answers make, the declining queries' MRK_ROW_DECLINED without keys;
    - merged with the rows of a healthy second segment the result is the numpy model's of the oracle's rows: the declining
      queries' rows carry MRK_ROW_DECLINED (without keys where the query is sorted or ordered; a relevance query's merged row keeps
      the answering segment's keys under the flag, as dist.merge_srows_np / merge_orows_np state the merge), the others are the
      unsplit corpus' answer;
    - the healthy batch on the same Batch afterwards leaves rows without a stale flag, standing and exported."""
    m, ctx, hip = dev
    from manticoresearch_amd import dist as mdist

    c, qs, declining, healthy_qs, exp = row_expectations[trigger]
    exp = exp[fmt]
    R = Rows(m, hip, fmt, len(qs))
    segs = [m.Segment(ctx, c.his[s], rowid_base=c.bases[s]) for s in (0, 1)]
    batch = m.Batch(ctx, len(qs))
    try:
        for s in (0, 1):
            segs[s].set_attrs(c.seg_rows(s))
        with trigger_settings(ctx, trigger):
            dst = R.buffer()
            R.chk(R.set_dst(batch._h, dst))
            batch.submit(segs[0], qs)
            hip.sync()  # the stream has drained; the host has not looked
            standing = R.host(dst)
            for i in declining:
                rd.assert_declined_row(mdist, standing[i], ("standing, before the wait", trigger, fmt, i), (mdist.ROW_RERUN, mdist.ROW_DECLINED))
            batch.wait()
            err = last_error()
            R.chk(R.set_dst(batch._h, None))
            got = batch.results()
            assert [g.status for g in got] == [UNSUPPORTED if i in declining else 0 for i in range(len(qs))], ([g.status for g in got], err)
            assert (LIVE_STATES if trigger == "fsm" else ARENA) in err, err  # the limit was met, and by this trigger
            exported = R.export(batch)
        for i in declining:
            rd.assert_declined_row(mdist, exported[i], ("exported after the wait", trigger, fmt, i))
        rd.assert_rows_equal(mdist, exported, exp["seg"][0], ("exported", trigger, fmt))
        keep = [i for i in range(len(qs)) if i not in declining]
        rd.assert_rows_equal(mdist, R.host(dst)[keep], exp["seg"][0][keep], ("standing", trigger, fmt))
        # the healthy second segment, and the merge of the two
        batch.submit(segs[1], qs)
        batch.wait()
        assert [g.status for g in batch.results()] == [0] * len(qs)
        second = R.export(batch)
        rd.assert_rows_equal(mdist, second, exp["seg"][1], ("segment 1", trigger, fmt))
        merged = R.merge(ctx, [exported, second], rd.KROWS)
        model = rd.merge_model(mdist, fmt, np.stack([exp["seg"][0], exp["seg"][1]]), rd.KROWS)
        for i in declining:  # (a sorted / ordered query's merged row has no keys; a relevance query's keeps the answering lists' under the flag: the models' rule)
            assert int(merged[i, K1 + 1]) & mdist.ROW_DECLINED, ("merged: a declined list's flag is lost", trigger, fmt, i, hex(int(merged[i, K1 + 1])), int(merged[i, K1]))
            assert int(model[i, K1 + 1]) & mdist.ROW_DECLINED and (int(model[i, K1]) == 0 or not rd.spec_word(mdist, fmt, qs[i]))
        rd.assert_rows_equal(mdist, merged, model, ("merged vs the model", trigger, fmt))
        rd.assert_rows_equal(mdist, merged[keep], exp["whole"][keep], ("merged vs the unsplit corpus", trigger, fmt))
        # a later submit of the same batch without the declining queries: nothing of them is left, standing or exported
        dst2 = R.buffer()
        R.chk(R.set_dst(batch._h, dst2))
        batch.submit(segs[0], healthy_qs)
        batch.wait()
        R.chk(R.set_dst(batch._h, None))
        assert [g.status for g in batch.results()] == [0] * len(qs)
        rd.assert_rows_equal(mdist, R.host(dst2), exp["healthy"], ("healthy batch, standing", trigger, fmt))
        rd.assert_rows_equal(mdist, R.export(batch), exp["healthy"], ("healthy batch, exported", trigger, fmt))
    finally:
        L()[0].mrk_batch_set_rows_dst(batch._h, None), L()[0].mrk_batch_set_srows_dst(batch._h, None), L()[0].mrk_batch_set_orows_dst(batch._h, None)
        batch.close()
        for s in segs:
            s.close()
        hip.free()


def test_shard_merger_reports_a_run_time_decline_as_one_declined_query():
    """ShardMerger on one rank with an attached batch, the three formats, both triggers (own process: torch has to load its HIP
    runtime before libmrk.so pulls in the system one): finish() returns -- no "overflowed again" for a query no rerun can repair --,
    results(allow_declined=True) has None for the declining queries and the oracle's answer for the rest, and the healthy batch
    behind it on the same attached Batch comes back whole."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(here, "runtime_declines_worker.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime declines chain ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
