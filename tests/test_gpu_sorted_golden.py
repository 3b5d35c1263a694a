"""GPU: every expressible case of tests/golden/sorted_vectors.json -- results the reference recorded for queries sorted by an
attribute (test_106, test_140), ordered by the 64-bit id (test_146), filtered by an attribute and ranked under SPH_MATCH_ANY
(test_016) -- answered on the device and compared with the recorded list itself: ids in the recorded order, weights, attribute
values, total_found.  No oracle runs here and nothing of the reference is read.  Each case is asked from the hand-built tree and
from its query text, in every spelling of its order (Query.sort, a one-part Query.order, the id as SORTKEY_INT64), at every K, alone
in a batch and mixed into one batch with relevance queries and the other cases, on a segment with rowid_base != 0; then the corpus
is cut into two and three rowid-range segments at every cut position, the segments' wide rows and order rows are merged on the
device (mrk_topk_merge_srows / mrk_topk_merge_orows) and unmapped.  No case may be declined, and the number of cases run is asserted."""
import dataclasses

import numpy as np
import pytest

import order_merge_common as omc
import sort_merge_common as smc
import sorted_golden_common as sg
from test_gpu_order_merge import Hip
from test_gpu_sort_merge import L

pytestmark = pytest.mark.gpu

K1 = 1024


@pytest.fixture(scope="module")
def dev():
    import manticoresearch_amd as m

    ctx = m.Context(0)
    batch = m.Batch(ctx, 256)
    hip = Hip()
    yield m, ctx, batch, hip
    hip.free()
    batch.close()
    ctx.close()


def check(corpus, case, what, q, g, K):
    assert g.status == 0, (what, "no recorded case may be declined", g.status)
    want = sg.recorded(corpus, case, K)
    sg.assert_answer(case, what, g.rowid, g.weight, g.total_found, want)
    if q.sort is not None:
        assert g.order_key is None and np.array_equal(g.sort_key, sg.recorded_key(corpus, q, want[0])), what
    elif q.order is not None:
        assert g.sort_key is None and np.array_equal(g.order_key, sg.recorded_key(corpus, q, want[0])), what
    else:
        assert g.sort_key is None and g.order_key is None, what


def variations(m, corpus, cases):
    """[(case, what, query, K)]: tree / query text x every spelling of the order x every K"""
    out = []
    for case in cases:
        ks = [corpus.n] if case.get("unordered") else sorted(set(range(1, case["total_found"] + 1)) | {corpus.n})
        for from_text in (False, True) if sg.parses(case) else (False,):
            for K in ks:
                for label, q in sg.spellings(m, corpus, case, sg.base_query(m, corpus, case, from_text, K)):
                    out.append((case, (case["name"], "text" if from_text else "tree", label, K), q, K))
    return out


def test_recorded_cases_on_device(dev):
    m, ctx, batch, hip = dev
    ran = set()
    n_text = 0
    for name in sg.G["corpora"]:
        corpus = sg.Corpus(name)
        cases = [c for c in sg.EXPRESSIBLE if c["corpus"] == name]
        host = corpus.index(m)
        V = variations(m, corpus, cases)
        # relevance queries to sit between the recorded cases: every case's own tree without its order
        rel = [dataclasses.replace(sg.base_query(m, corpus, c), filters=None) for c in cases]
        for base in (0, 1000):
            seg = m.Segment(ctx, host, rowid_base=base)
            try:
                seg.set_attrs(corpus.rows)
                rel_alone = batch.search(seg, rel)
                assert [g.status for g in rel_alone] == [0] * len(rel)
                if base == 0:  # alone in a batch
                    for case, what, q, K in V:
                        check(corpus, case, what + ("alone",), q, batch.search(seg, [q])[0], K)
                # mixed: recorded cases of every kind and relevance queries in one batch, 255 at a time
                mixed = []
                for i, v in enumerate(V):
                    mixed.append(v)
                    if i % 4 == 0:
                        mixed.append(rel[(i // 4) % len(rel)])
                for at in range(0, len(mixed), 255):
                    chunk = mixed[at:at + 255]
                    got = batch.search(seg, [x[2] if isinstance(x, tuple) else x for x in chunk])
                    assert batch.stats()["packed"] == 1 and batch.stats()["n_rerun"] == 0
                    for x, g in zip(chunk, got):
                        if isinstance(x, tuple):
                            check(corpus, x[0], x[1] + ("mixed", base), x[2], g, x[3])
                            ran.add(x[0]["name"])
                            n_text += x[1][1] == "text"
                        else:  # a relevance query next to them answers as in a batch of its own
                            w = rel_alone[rel.index(x)]
                            assert g.status == 0 and g.total_found == w.total_found and np.array_equal(g.rowid, w.rowid) and np.array_equal(g.weight, w.weight)
            finally:
                seg.close()
    assert len(ran) == len(sg.EXPRESSIBLE) == 18, sorted(ran)
    assert n_text >= 2 * sum(sg.parses(c) for c in sg.EXPRESSIBLE)  # (every case the parser covers, on both segments)


def test_recorded_cases_across_segments(dev):
    """Every cut of each corpus into two and three rowid-range segments: exported srows and orows, merged on the device, unmapped."""
    m, ctx, batch, hip = dev
    from manticoresearch_amd import dist as mdist

    lib, chk = L()
    ran = set()
    for name in sg.G["corpora"]:
        corpus = sg.Corpus(name)
        cases = [c for c in sg.EXPRESSIBLE if c["corpus"] == name]
        Q = [(c, l, corpus.globalize(q)) for c in cases for l, q in sg.spellings(m, corpus, c, sg.base_query(m, corpus, c))]
        qs = [q for _, _, q in Q]
        nq, SW, OW = len(qs), m.SROW_WORDS, m.OROW_WORDS
        assert nq <= 256
        srows_all, orows_all = hip.malloc(3 * nq * SW * 8), hip.malloc(3 * nq * OW * 8)
        s_out, o_out = hip.malloc(nq * SW * 8), hip.malloc(nq * OW * 8)
        n_cuts = 0
        for shards in (2, 3):
            for cuts in corpus.cuts(shards):
                hip.fill(srows_all, 0xEE, 3 * nq * SW * 8)
                hip.fill(orows_all, 0xEE, 3 * nq * OW * 8)
                for s in range(shards):
                    seg = m.Segment(ctx, corpus.index(m, cuts[s], cuts[s + 1]), rowid_base=cuts[s])
                    try:
                        seg.set_attrs(np.ascontiguousarray(corpus.rows[cuts[s]:cuts[s + 1]]))
                        batch.submit(seg, qs)
                        batch.wait()
                        assert [r.status for r in batch.results()] == [0] * nq, (name, cuts, s, "no recorded case may be declined on a shard")
                        assert batch.stats()["n_rerun"] == 0
                        batch.export_srows(srows_all.value + s * nq * SW * 8)
                        batch.export_orows(orows_all.value + s * nq * OW * 8)
                    finally:
                        seg.close()
                hip.fill(s_out, 0xEE, nq * SW * 8)
                hip.fill(o_out, 0xEE, nq * OW * 8)
                chk(lib.mrk_topk_merge_srows(ctx._h, srows_all, shards, nq, 1024, s_out))
                chk(lib.mrk_topk_merge_orows(ctx._h, orows_all, shards, nq, 1024, o_out))
                ms, mo = hip.to_host(s_out, (nq, SW)), hip.to_host(o_out, (nq, OW))
                for qi, (case, label, q) in enumerate(Q):
                    what = (case["name"], label, cuts)
                    want = sg.recorded(corpus, case)
                    row = mo[qi]
                    assert not int(row[K1 + 1]) & (mdist.ROW_RERUN | mdist.ROW_DECLINED), (what, "orow flagged")
                    omc.assert_padding(mdist, row)
                    assert int(row[mdist.OROW_SPEC]) == omc.spec_of(mdist, q), what
                    docid, weight, total = omc.decode_orow(row, q.max_matches)
                    sg.assert_answer(case, what + ("orows",), docid, weight, total, want)
                    vals = mdist.unmap_order_keys(int(row[mdist.OROW_SPEC]), mdist.orow_mkeys(row)[:len(docid)])
                    if q.order is not None:
                        assert np.array_equal(vals, sg.recorded_key(corpus, q, want[0])), what
                    elif q.sort is not None:
                        assert np.array_equal(vals, sg.recorded_key(corpus, q, want[0]).astype(np.uint64) << np.uint64(32)), what
                    if q.order is None:  # (a wide row carries no 64-bit key: Order queries travel in order rows alone)
                        row = ms[qi]
                        assert not int(row[K1 + 1]) & (mdist.ROW_RERUN | mdist.ROW_DECLINED), (what, "srow flagged")
                        smc.assert_padding(mdist, row)
                        docid, weight, sk, total = smc.decode_srow(mdist, row, q.max_matches)
                        sg.assert_answer(case, what + ("srows",), docid, weight, total, want)
                        assert (sk is None) == (q.sort is None) and (sk is None or np.array_equal(sk, sg.recorded_key(corpus, q, want[0]))), what
                    ran.add(case["name"])
                n_cuts += 1
        assert n_cuts == (corpus.n - 1) + (corpus.n - 1) * (corpus.n - 2) // 2  # every cut position, with two and with three segments
    hip.free()
    assert len(ran) == len(sg.EXPRESSIBLE) == 18, sorted(ran)
