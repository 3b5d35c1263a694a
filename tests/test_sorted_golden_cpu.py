"""CPU: the expectation the sorted / ordered GPU tests compare against -- the oracle's matches reordered by numpy
(sorted_expect.expected_sort / expected_order) -- against what the REFERENCE recorded (tests/golden/sorted_vectors.json: the
`matches` arrays of test_106, test_146, test_016 and test_140's model.bin, in the order the daemon returned them).  Until these
results were written down, the reading of the reference's sorter in sorted_expect.py (unsigned compare, the weight tie rule, rowid
ascending last whatever the attribute's direction) was checked against nothing but itself; so were the oracle's MATCHANY ranker
and its attribute filters.  Also: dist.merge_srows_np / merge_orows_np over every rowid-range cut of each corpus into two and three
shards, and every K.  Every comparison is exact; no case is skipped (the count is asserted).

What the recorded results can NOT tell (none of them holds such rows): a 64-bit key with the sign bit set (every recorded id is a
small positive number: reading the high dword unsigned changes no recorded order -- test_gpu_order.py's random bigint columns of both
signs cover that against numpy's int64 view only), float keys and -0.0, then_weight 0 against 1 / 2 (test_106's tied rows carry
equal weights)."""
import numpy as np
import pytest

import order_merge_common as omc
import sort_merge_common as smc
import sorted_golden_common as sg
from sorted_expect import expected_order, expected_sort
from test_query_parser import as_golden, strip_op_masks


def _m():
    import manticoresearch_amd as m

    return m


def _oracle_index(orc, m, corpus, lo=0, hi=None):
    from test_gpu_parity import orc_index_of

    host = corpus.index(m, lo, hi)
    oi = orc_index_of(orc, host)
    oi.host = host  # (the oracle's arrays are views into the host index: it must outlive them)
    oi.attrs = np.ascontiguousarray(corpus.rows[lo:hi])
    return oi


def _answer(orc, oi, q, rows, n):
    """(rowid, weight, key or None, total) through the shared expectation"""
    from test_gpu_parity import to_orc

    if q.sort is not None:
        return expected_sort(orc, oi, q, rows, n)
    if q.order is not None:
        return expected_order(orc, oi, q, rows, n)
    r = to_orc(orc, q).run(oi)
    return r.rowid, r.weight, None, int(r.total_found)


def test_fixture_holds_the_required_cases():
    src = [c["source"] for c in sg.CASES]
    assert "test/test_106/test.xml:58" in src and "test/test_016/test.xml:37" in src and "test/test_016/test.xml:38" in src
    assert [s for s in src if s.startswith("test/test_146/")] == ["test/test_146/test.xml:%d" % n for n in range(134, 146)]
    assert [c["source"] for c in sg.CASES if c["device"] == "not expressible"] == ["test/test_106/test.xml:59", "test/test_106/test.xml:60"]
    assert len(sg.CASES) == 20 and len(sg.EXPRESSIBLE) == 18
    for c in sg.CASES:
        assert c["total_found"] == len(c["expect"])  # (no recorded list is cut by a limit)


@pytest.mark.parametrize("case", [c for c in sg.CASES if sg.parses(c)], ids=lambda c: c["name"])
def test_parsed_text_equals_the_recorded_tree(case):
    m = _m()
    t = m.parse_query(case["text"], [], sg.G["corpora"][case["corpus"]]["min_word_len"])
    assert as_golden(t) == strip_op_masks(case["query"])


@pytest.mark.parametrize("case", sg.CASES, ids=lambda c: c["name"])
def test_oracle_weights_and_total(orc, case):
    """1. the oracle's weights and total_found are the recorded ones (MATCHANY and the filter included); a sorter that spells its
    whole order out (test_106's third query) is also replayed by numpy over the oracle's matches."""
    from test_gpu_parity import to_orc

    m = _m()
    corpus = sg.Corpus(case["corpus"])
    oi = _oracle_index(orc, m, corpus)
    r = to_orc(orc, sg.base_query(m, corpus, case)).run(oi)
    print(case["name"], [(corpus.ids[int(i)], int(w)) for i, w in zip(r.rowid, r.weight)], r.total_found)
    assert r.total_found == case["total_found"] == len(r.rowid)
    want = {i: w for i, w in case["expect"]}
    assert sorted(corpus.ids[int(i)] for i in r.rowid) == sorted(want)
    if "weights" not in case:
        assert {corpus.ids[int(i)]: int(w) for i, w in zip(r.rowid, r.weight)} == want
    if case["sorter"].get("sortby") == "@weight DESC, date_added DESC, id DESC":
        date = corpus.rows[r.rowid, corpus.loc["date_added"][0] >> 5].astype(np.int64)
        ids = np.array(corpus.ids)[r.rowid]
        order = np.lexsort((-ids, -date, -r.weight.astype(np.int64)))
        assert [[int(ids[i]), int(r.weight[i])] for i in order] == case["expect"]


@pytest.mark.parametrize("case", sg.EXPRESSIBLE, ids=lambda c: c["name"])
def test_shared_expectation_gives_the_recorded_order(orc, case):
    """2. + 4. oracle + lexsort == the recorded list, under every spelling of the order and at every K (the recorded list's prefix,
    total_found unchanged)."""
    m = _m()
    corpus = sg.Corpus(case["corpus"])
    oi = _oracle_index(orc, m, corpus)
    n_match = case["total_found"]
    ran = 0
    for from_text in (False, True) if sg.parses(case) else (False,):
        for K in [corpus.n] if case.get("unordered") else sorted(set(range(1, n_match + 1)) | {corpus.n}):
            for label, q in sg.spellings(m, corpus, case, sg.base_query(m, corpus, case, from_text, K)):
                rid, w, key, total = _answer(orc, oi, q, corpus.rows, corpus.n)
                want = sg.recorded(corpus, case, K)
                sg.assert_answer(case, (case["name"], label, K, from_text), rid, w, total, want)
                if key is not None:
                    assert np.array_equal(key, sg.recorded_key(corpus, q, want[0]))
                ran += 1
    assert ran >= (1 if case.get("unordered") else max(n_match, 1))


@pytest.mark.parametrize("case", sg.EXPRESSIBLE, ids=lambda c: c["name"])
def test_numpy_merges_reproduce_the_recorded_list_at_every_cut(orc, case):
    """3. every cut of the corpus into two and into three rowid ranges: each shard's answer (oracle + the shared expectation over the
    shard's own rows, ranked with the corpus-wide statistics) packed into wide rows and order rows, merged by dist.merge_srows_np /
    merge_orows_np, decoded and unmapped -> the recorded ids, weights and attribute values."""
    from manticoresearch_amd import dist
    from test_gpu_parity import to_orc

    m = _m()
    corpus = sg.Corpus(case["corpus"])
    want = sg.recorded(corpus, case)
    qs = [(l, corpus.globalize(q)) for l, q in sg.spellings(m, corpus, case, sg.base_query(m, corpus, case))]
    n_cuts = 0
    for shards in (2, 3):
        if corpus.n < shards:
            continue
        for cuts in corpus.cuts(shards):
            ois = [_oracle_index(orc, m, corpus, cuts[s], cuts[s + 1]) for s in range(shards)]
            srows = np.zeros((shards, len(qs), dist.SROW_WORDS), np.uint64)
            orows = np.zeros((shards, len(qs), dist.OROW_WORDS), np.uint64)
            for s in range(shards):
                rows_s, n_s = np.ascontiguousarray(corpus.rows[cuts[s]:cuts[s + 1]]), cuts[s + 1] - cuts[s]
                for qi, (_, q) in enumerate(qs):
                    orows[s, qi] = omc.shard_answer_orow(dist, orc, to_orc, expected_order, expected_sort, ois[s], q, rows_s, n_s, cuts[s])
                    if q.order is None:  # (a wide row carries no 64-bit key)
                        srows[s, qi] = smc.shard_answer_row(dist, orc, expected_sort, to_orc, ois[s], q, rows_s, n_s, cuts[s])
            mo, ms = dist.merge_orows_np(orows, 1024), dist.merge_srows_np(srows, 1024)
            for qi, (label, q) in enumerate(qs):
                what = (case["name"], label, cuts)
                omc.assert_padding(dist, mo[qi])
                assert int(mo[qi, dist.OROW_SPEC]) == omc.spec_of(dist, q)
                docid, weight, total = omc.decode_orow(mo[qi], q.max_matches)
                sg.assert_answer(case, what + ("orows",), docid, weight, total, want)
                vals = dist.unmap_order_keys(int(mo[qi, dist.OROW_SPEC]), dist.orow_mkeys(mo[qi])[:len(docid)])
                if q.order is not None:
                    assert np.array_equal(vals, sg.recorded_key(corpus, q, want[0])), what
                elif q.sort is not None:
                    assert np.array_equal(vals, sg.recorded_key(corpus, q, want[0]).astype(np.uint64) << np.uint64(32)), what
                if q.order is None:
                    smc.assert_padding(dist, ms[qi])
                    docid, weight, sk, total = smc.decode_srow(dist, ms[qi], q.max_matches)
                    sg.assert_answer(case, what + ("srows",), docid, weight, total, want)
                    assert (sk is None) == (q.sort is None) and (sk is None or np.array_equal(sk, sg.recorded_key(corpus, q, want[0]))), what
            n_cuts += 1
    n = corpus.n
    assert n_cuts == (n - 1) + (n - 1) * (n - 2) // 2  # every cut position, with two and with three shards
