"""CPU: the weight in front of the sorter's order (Order.weight_first; mrk_order::then_weight = MRK_ORDER_WEIGHT_FIRST_DESC / _ASC -- 'ORDER BY weight() DESC, attr', '@weight DESC,
date_added DESC', 'ORDER BY weight() ASC').  The candidate layout and the weight's pruning bin (csrc/mrk_sortkey.h) and the planner's
answers (csrc/mrk_plan.cpp) are checked by host-only programs under AddressSanitizer + UBSan (tests/cpp/weight_first_key.cpp,
weight_first_plan.cpp, built like order_plan.cpp); the Python marshalling on the flattened C structs; and the expectation the GPU
tests compare against (weight_first_expect.py) on what the REFERENCE recorded for its own weight-first sorters
(tests/golden/sorted_vectors.json, read and not edited: the Order translations are this file's)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sorted_golden_common as sg
from weight_first_expect import expected_weight_first

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]


def _m():
    import manticoresearch_amd as m

    return m


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_key_order_inverse_and_bins_under_sanitizers(tmp_path):
    exe = str(tmp_path / "weight_first_key")
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(HERE, "cpp", "weight_first_key.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    # both weight directions x (no parts, one part x 2 directions x int / float, two parts x 4 directions x 3 kinds, INT64 x 2 directions)
    assert out.stdout.startswith("ok variants %d" % (2 * (1 + 4 + 12 + 2))), out.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only objects")
def test_planner_under_sanitizers(tmp_path):
    objs = []
    for src in (os.path.join(ROOT, "manticoresearch_amd", "csrc", "mrk_plan.cpp"), os.path.join(HERE, "cpp", "weight_first_plan.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([HIPCC] + FLAGS + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "weight_first_plan")
    subprocess.check_call([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    # 5 query shapes x 4 rankers x (2 weight directions x (5 single parts + 3 pairs) + weight ASC alone, the latter without attribute rows too)
    assert out.stdout.startswith("ok accepted %d declined 11 hostile 18" % (5 * 4 * (2 * 8 + 1 + 1))), out.stdout


def test_order_weight_first_round_trips_through_cqueries():
    m = _m()
    from manticoresearch_amd import _lib
    from manticoresearch_amd.api import _CQueries

    kw = m.XQNode.keyword
    qs = [m.Query(kw(1, 1), order=m.Order([m.OrderPart(0, 32)], weight_first=1)),
          m.Query(kw(1, 1), order=m.Order([m.OrderPart(128, 64, desc=False, kind=m.SORTKEY_INT64)], weight_first=2)),
          m.Query(kw(1, 1), order=m.Order(parts=[], weight_first=2)),
          m.Query(kw(1, 1), order=m.Order([m.OrderPart(35, 5), m.OrderPart(64, 32, kind=m.SORTKEY_FLOAT)], then_weight=2)),
          m.Query(kw(1, 1), order=m.Order([m.OrderPart(35, 5)]))]
    cq = _CQueries(qs)
    got = [(c.order.contents.n_parts, c.order.contents.then_weight) for c in cq.arr]
    # include/mrk.h: then_weight says where the weight stands -- MRK_ORDER_WEIGHT_FIRST | 1 / 2 in front, 0 / 1 / 2 behind (left alone: 1)
    assert got == [(1, 0x101), (1, 0x102), (0, 0x102), (2, 2), (1, 1)]
    assert [q.order.then_weight for q in qs] == [0, 0, 0, 2, 1]
    with pytest.raises(ValueError):  # in front AND behind: one word cannot say it
        _CQueries([m.Query(kw(1, 1), order=m.Order([m.OrderPart(0, 32)], weight_first=1, then_weight=1))])
    assert C.sizeof(_lib.Order) == 4 + 2 * 16 + 4  # mrk_order keeps its size and layout


def _oracle_index(orc, m, corpus):
    from test_gpu_parity import orc_index_of

    host = corpus.index(m)
    oi = orc_index_of(orc, host)
    oi.host = host  # (the oracle's arrays are views into the host index: it must outlive them)
    oi.attrs = np.ascontiguousarray(corpus.rows)
    return oi


def _case(source):
    return next(c for c in sg.CASES if c["source"] == source)


def test_recorded_weight_ascending_is_the_expectation_in_order(orc):
    """test_016:38, sortby="-@weight": the recorded list IS weight ascending, rowid ascending -- Order(parts=[], weight_first=2) -- in
    ORDER (the fixture compares it as a set, since no mrk_query said it), at every K."""
    m = _m()
    case = _case("test/test_016/test.xml:38")
    assert case["sorter"]["sortby"] == "-@weight"
    corpus = sg.Corpus(case["corpus"])
    oi = _oracle_index(orc, m, corpus)
    for from_text in (False, True) if sg.parses(case) else (False,):
        for K in sorted(set(range(1, case["total_found"] + 1)) | {corpus.n}):
            import dataclasses

            q = dataclasses.replace(sg.base_query(m, corpus, case, from_text, K), order=m.Order(parts=[], weight_first=2))
            rid, w, key, total = expected_weight_first(orc, oi, q, corpus.rows, corpus.n)
            assert key is None and total == case["total_found"]
            assert [[corpus.ids[int(r)], int(x)] for r, x in zip(rid, w)] == case["expect"][:K], (K, from_text)


def test_recorded_weight_then_date_is_the_expectation_up_to_full_ties(orc):
    """test_106:59, sortby="@weight DESC, date_added DESC": the recorded list equals the expectation under
    Order([date_added DESC], weight_first=1) up to the order INSIDE groups whose weight AND date are equal.  Those three pairs are
    recorded 6 before 3, 5 before 2, 4 before 1 (ids; higher rowid first), where MatchGeneric2_fn as read ends on rowid ascending:
    unexplained (tests/golden/README_weight_first.md), so the group structure is asserted and the inner order is not -- no rule is made up for it."""
    import dataclasses

    m = _m()
    case = _case("test/test_106/test.xml:59")
    assert case["sorter"]["sortby"] == "@weight DESC, date_added DESC"
    corpus = sg.Corpus(case["corpus"])
    oi = _oracle_index(orc, m, corpus)
    off, bits, kind = corpus.loc["date_added"]
    q = dataclasses.replace(sg.base_query(m, corpus, case), order=m.Order([m.OrderPart(off, bits, desc=True, kind=kind)], weight_first=1))
    rid, w, key, total = expected_weight_first(orc, oi, q, corpus.rows, corpus.n)
    assert total == case["total_found"] == len(rid)
    date_of = lambda r: int(corpus.rows[int(r), off >> 5])

    def groups(rows_w):  # [(weight, date, set of ids)] in list order: maximal runs of equal (weight, date)
        out = []
        for r, x in rows_w:
            k = (int(x), date_of(r))
            if out and out[-1][:2] == k:
                out[-1][2].add(corpus.ids[int(r)])
            else:
                out.append((k[0], k[1], {corpus.ids[int(r)]}))
        return out

    want_rows = [(corpus.rowid_of[i], x) for i, x in case["expect"]]
    got, want = groups(zip(rid, w)), groups(want_rows)
    assert got == want
    assert [len(g[2]) for g in want] == [1, 2, 1, 2, 1, 2]  # (three fully tied pairs: the rest of the list is decided by the two parts)
    assert (key >> np.uint64(32)).tolist() == [date_of(r) for r in rid] and not (key & np.uint64(0xFFFFFFFF)).any()
    # strictly ordered across groups: weight descending, then date descending
    for a, b in zip(want, want[1:]):
        assert (a[0], a[1]) > (b[0], b[1])


def test_third_part_stays_not_expressible():
    """test_106:60 (@weight DESC, date_added DESC, id DESC) needs a third part behind the weight: mrk_order holds two, and a 64-bit
    part stands alone (weight_first_plan.cpp: MRK_E_INVAL).  The fixture keeps the case as not expressible."""
    from manticoresearch_amd import _lib

    assert _lib.MRK_MAX_ORDER_PARTS == 2
    case = _case("test/test_106/test.xml:60")
    assert case["device"] == "not expressible" and case["sorter"]["sortby"].count(",") == 2
