"""CPU: the corpora of the hit-stream decoders' suite (hit_edges_common.py) reach every edge they are built for -- asserted from the
bytes index_from_hits wrote, through a restatement of the window discipline -- and the oracle agrees with a Python model of the
weights that works from the hit arrays.  The coverage assertions are conditions on the builder: if one fails, the builder changes."""
import numpy as np
import pytest

import hit_edges_common as C
from test_gpu_parity import orc_index_of, to_orc


@pytest.fixture(scope="module")
def m():
    import manticoresearch_amd

    return manticoresearch_amd


def test_window_trace_on_a_hand_made_stream():
    # dummy byte; 1 | 0x81 0x00 (128) | 5 bytes (2^28 + 3) | seven 2s | 3 bytes | terminator
    spp = np.array([1, 0x01, 0x81, 0x00, 0x81, 0x80, 0x80, 0x80, 0x03] + [2] * 7 + [0x81, 0x80, 0x05, 0] + [0] * 64, np.uint8)
    trace, hits, refills, end = C.window_trace(spp, 1)
    assert trace[:3] == [(1, 1), (2, 2), (5, 4)] and trace[3:10] == [(1, o) for o in range(9, 12)] + [(1, o) for o in range(0, 4)]
    assert trace[10:] == [(3, 4), (1, 7)] and refills == [1] and end == 19
    assert hits[:3] == [1, 129, 129 + (1 << 28) + 3] and hits[-1] == hits[2] + 14 + (1 << 14) + 5
    assert [C.vlb_len(v) for v in (1, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, 0xFFFFFFFF)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5]


def test_crafted_lists_are_what_they_claim():
    for nf in (8, 32):
        for k, v, t in C.grid(nf):
            h = C.craft(k, v, t, nf, salt=k + t)
            d = np.diff([0] + h)
            lens = [C.vlb_len(int(x)) for x in d]
            want = 4 if v in ("4p", "4f") else 5 if v == "5" else v
            assert lens == [1] * k + [want] + [1] * t and len(h) == k + 1 + t
            assert ((h[k] >> 24) != 0) == (v in ("4f", "5")) and (v != "5" or h[k] >> 24 >= 16)
        assert len(C.grid(nf)) == (320 if nf == 8 else 384)
    # the end flag in front of a field change and on the last hit: the deltas next to it cross bit 23
    h = C.craft(6, "5", 2, 32, salt=1, flag=2)
    assert h[5] & C.END and C.vlb_len(h[5] - h[4]) == 4 and C.vlb_len(h[6] - h[5]) == 5
    h = C.craft(6, 2, 1, 32, salt=1, flag=1)
    assert h[-1] & C.END and C.vlb_len(h[-1] - h[-2]) == 4


@pytest.mark.parametrize("name", C.SEGMENT_IDS)
def test_every_length_at_every_window_offset(m, orc, name):
    hi, docs = C.segment(name)
    oi = orc_index_of(orc, hi)
    spp = np.concatenate([hi.spp, np.zeros(64, np.uint8)])
    max_len = 5 if hi.n_fields > 16 else 4
    last_end = 0
    for term in (C.T_A, C.T_B):  # each crafted keyword on its own reaches everything
        pairs, term_at, aligns, refill_before = set(), set(), set(), set()
        lists = C.stored_lists(oi, term)
        n_refills = 0
        for rowid, p in lists:
            trace, hits, refills, end = C.window_trace(spp, p)
            assert hits == docs[rowid].hits[term], (name, term, rowid)  # the bytes hold the crafted hits
            pairs.update(trace[:-1])
            term_at.add(trace[-1][1])
            aligns.add(p & 3)
            refill_before.update(refills)
            n_refills += len(refills)
            last_end = max(last_end, end)
        # a multi-hit list lives in .spp in both formats, a lone hit in the plain one only
        assert len(lists) == sum(1 for d in docs if len(d.hits[term]) > 1 or not hi.hit_format)
        assert pairs == {(n, o) for n in range(1, max_len + 1) for o in range(12)}, (name, term, sorted(pairs))
        assert term_at == set(range(12)), (name, term, sorted(term_at))
        assert aligns == {0, 1, 2, 3}
        assert refill_before == set(range(1, max_len + 1)), (name, term, refill_before)
        assert n_refills >= 150, (name, term, n_refills)
    # B is the last keyword and the highest rowid holds a crafted list on it: that list ends on the last byte of .spp
    assert docs[-1].slot == C.T_B and docs[-1].kind == "grid" and C.stored_lists(oi, C.T_B)[-1][0] == len(docs) - 1
    assert last_end == len(hi.spp) - 1 and hi.spp[-1] == 0
    tail = C.window_trace(spp, C.stored_lists(oi, C.T_B)[-1][1])[0]
    assert tail[-2][0] == max_len  # ... behind its longest varint
    if hi.hit_format:  # a lone hit travels in the doclist
        assert sum(1 for r, _, _, hp in zip(*oi.decode_doclist(C.T_A)) if int(hp) >> 63) == sum(1 for d in docs if len(d.hits[C.T_A]) == 1)


def test_corpus_shape():
    for nf in (8, 32):
        docs = C.corpus_docs(nf)
        kinds = [d.kind for d in docs]
        assert len(docs) <= 1000 and kinds.count("control") == C.N_CONTROLS
        assert kinds.count("grid") == 2 * len(C.grid(nf)) and kinds.count("long") == 2
        assert all(set(d.hits) == {0, 1, 2, 3, 4} for d in docs)
        assert all(len(d.hits[d.slot]) > 300 for d in docs if d.kind == "long")
        assert any(d.hits[d.slot][-1] & C.POS_MASK == C.MAX_POS for d in docs if d.kind == "max_pos_last")
        assert any(d.hits[d.slot] == [((nf - 1) << 24) | C.END | 9] for d in docs)
        if nf == 32:  # a list whose first delta is itself 5 bytes
            assert any(C.vlb_len(d.hits[d.slot][0]) == 5 and len(d.hits[d.slot]) > 1 for d in docs)
        # neighbouring rowids differ: no run of the grid's order survives the permutation
        cells = [getattr(d, "cell", None) for d in docs]
        assert sum(1 for a, b in zip(cells, cells[1:]) if a and b and a[:2] == b[:2]) < len(docs) // 20


@pytest.mark.parametrize("name", ["N-inline-128", "W-plain-128"])
def test_index_from_hits_writes_the_oracle_writers_bytes(m, orc, name):
    hi, docs = C.segment(name)
    W, R, H = C.hits_of(docs)
    oi = orc.build_index(W, R, H, total_docs=len(docs), skiplist_block_size=hi.skiplist_block_size, inline_hits=hi.hit_format,
                         n_fields=hi.n_fields, n_terms=C.N_TERMS)
    assert np.array_equal(oi.spp, hi.spp) and np.array_equal(oi.spd, hi.spd)


@pytest.mark.parametrize("n_fields,fmt", [(8, 1), (32, 0)])
def test_oracle_equals_model(m, orc, n_fields, fmt):
    """PROXIMITY, WORDCOUNT, FIELDMASK and the docs of PHRASE(A, B), on an index the oracle's own writer built from the same hits."""
    docs = C.corpus_docs(n_fields)
    W, R, H = C.hits_of(docs)
    oi = orc.build_index(W, R, H, total_docs=len(docs), skiplist_block_size=128, inline_hits=fmt, n_fields=n_fields, n_terms=C.N_TERMS)
    fw = C.PRIMES[:n_fields]
    model_of = {m.SPH_RANK_PROXIMITY: C.proximity_weight, m.SPH_RANK_WORDCOUNT: C.wordcount_weight, m.SPH_RANK_FIELDMASK: C.fieldmask_weight}
    R_ = C.routes(m, n_fields)
    n_checked = 0
    for q in R_["P"] + R_["L"] + R_["G"]:
        if q.ranker not in model_of or q.root.op not in (m.SPH_QUERY_AND, m.SPH_QUERY_OR):
            continue
        kws = C.keywords_of(q.root)
        if len({t for t, _, _ in kws}) < len(kws):
            continue  # (a repeated keyword: the other Update)
        if len(kws) == 3 and any(mask != 0xFFFFFFFF for _, _, mask in kws) and q.ranker == m.SPH_RANK_PROXIMITY:
            continue  # (the MergeHits3 field test: the oracle's and the device's business)
        got = to_orc(orc, q).run(oi)
        rowid, weight = C.ranked(docs, kws, model_of[q.ranker], fw, match_all=q.root.op == m.SPH_QUERY_AND)
        assert got.total_found == rowid.size == got.rowid.size <= q.max_matches
        assert np.array_equal(got.rowid, rowid) and np.array_equal(got.weight, weight), (q.ranker, kws, got.weight[:6], weight[:6])
        n_checked += 1
    assert n_checked >= 12
    ph = to_orc(orc, m.Query(m.XQNode(m.SPH_QUERY_PHRASE, [C.kw(m, C.T_A), C.kw(m, C.T_B)]), ranker=m.SPH_RANK_NONE, max_matches=1000)).run(oi)
    want = C.phrase_docs(docs)
    assert ph.total_found == len(want) and sorted(ph.rowid.tolist()) == want
    controls = [r for r, d in enumerate(docs) if d.kind == "control"]
    assert not set(controls) & set(want) and len(want) > len(docs) // 2
    # an "always adjacent" answer fails: the controls' LCS is 1 in the last hit's field
    a, b = C.keywords_of(R_["P"][1].root)[:2]
    for r in controls:
        assert C.proximity_weight(docs[r], [a, b], [1] * 32) <= len({h >> 24 for h in docs[r].hits[docs[r].slot]})


@pytest.mark.parametrize("name", C.SEGMENT_IDS)
def test_every_query_stays_within_max_matches(m, orc, name):
    hi, docs = C.segment(name)
    oi = orc_index_of(orc, hi)
    for route, qs in C.routes(m, hi.n_fields).items():
        for q in qs:
            r = to_orc(orc, q).run(oi)
            assert r.total_found <= q.max_matches and r.rowid.size == r.total_found == r.weight.size, (route, r.total_found)
