"""Writes tests/golden/sorted_vectors.json: results the reference recorded for queries that are SORTED by an attribute, FILTERED by
one, or ranked under SPH_MATCH_ANY -- the order of the rows as the reference's sorter left it, with each row's weight.

The values below were copied by hand, as data, from the reference's own test directories while reading them (nothing of the
reference is imported or executed): corpora = the <db_insert> rows of test/test_NNN/test.xml, expected ordered (id, weight) lists
and total_found = the `matches` arrays of the tests' model.bin (PHP-serialised text; a PHP array keeps insertion order, which is
the order the daemon returned the rows in).  Queries are written as the parsed tree, in make_vectors.py's T / OP form.
Run:  python tests/golden/make_sorted_vectors.py
"""
import json
import os

ALL = 0xFFFFFFFF


def T(word, pos, mask=ALL):
    return {"word": word, "pos": pos, "mask": mask}


def OP(op, *kids, mask=ALL, opt=0):
    return {"op": op, "kids": list(kids), "mask": mask, "opt": opt}


def D(s):
    """'2008-10-01' under SET time_zone='+0:00' -> UNIX_TIMESTAMP, as model.bin lists the attribute"""
    return {"2008-10-01": 1222819200, "2008-10-02": 1222905600, "2008-10-03": 1222992000, "2008-10-07": 1223337600,
            "2008-10-08": 1223424000, "2008-10-09": 1223510400}[s]


# The sorter as the test spelled it -> what the device is asked.  Every attribute row starts with the document id as a bigint (two
# dwords, low first), the declared attributes follow in the order of the source; "attr" names the column.
BY_ID_ASC = {"order": {"parts": [{"attr": "id", "desc": False}], "then_weight": 0}}
BY_ID_DESC = {"order": {"parts": [{"attr": "id", "desc": True}], "then_weight": 0}}

CORPORA = {
    # test_106 "extended sort with more than 1 sorter": three pairs of rows share a date (1 / 4, 2 / 5, 3 / 6)
    "test_106": {"source": "test/test_106/test.xml:44-55 + model.bin", "min_word_len": 1, "fields": ["text"], "ids": list(range(1, 10)),
                 "docs": [["one"], ["one two"], ["one two three"], ["one"], ["one two"], ["one two three"], ["one"], ["one two"], ["one two three"]],
                 "attrs": [{"name": "date_added", "type": "timestamp",
                            "values": [D("2008-10-01"), D("2008-10-02"), D("2008-10-03"), D("2008-10-01"), D("2008-10-02"), D("2008-10-03"),
                                       D("2008-10-07"), D("2008-10-08"), D("2008-10-09")]}]},
    # test_146 "joined fields indexing", index test: field 0 = the `text` column, field 1 = the joined field (the rows of test_joined
    # with the document's id, in table order, one after the other: positions run on from row to row).  The index sets
    # phrase_boundary = '.' with phrase_boundary_step = 2 ('zzz. my': my sits 1 + 2 positions behind zzz) and a stopword file
    # holding "not" and "as" (none of the rows contains either; in a QUERY a stopword is dropped and keeps its position).
    "test_146": {"source": "test/test_146/test.xml:115-131 (index test: :37-55) + model.bin", "min_word_len": 1, "fields": ["text", "text"],
                 "phrase_boundary": ".", "phrase_boundary_step": 2, "stopwords": ["not", "as"], "ids": [1, 2, 3],
                 "docs": [["aaa", "jjj kkk zzz. my cool"], ["aaa bbb", "yyy ttt"], ["bbb ccc", "ccc do. dog sleepy"]],
                 "attrs": [{"name": "idd", "type": "uint", "values": [1, 2, 3]}]},
    # test_016 "expr sorting vs filters"; 'test-ing' indexes as test + ing
    "test_016": {"source": "test/test_016/test.xml:54-60 + model.bin", "min_word_len": 1, "fields": ["body"], "ids": [111, 222, 333, 444],
                 "docs": [["this is test"], ["just a test"], ["for test-ing purposes"], ["lets test it"]],
                 "attrs": [{"name": "group_id", "type": "uint", "values": [1, 1, 2, 1]}]},
    # test_140 "MVA and string via MySQL", index main: the body column is the one full-text field; idd and tag are the uint attributes
    # (the MVA and string attributes live in the blob pool and are not asked for here)
    "test_140": {"source": "test/test_140/test.xml:127-140 (index main) + model.bin", "min_word_len": 1, "fields": ["body"], "ids": list(range(1, 12)),
                 "docs": [["main and delta"], ["main and delta"], ["main and delta"], ["delta"], ["delta"], ["delta"], ["main"], ["main"], ["delta"],
                          ["delta"], ["delta"]],
                 "attrs": [{"name": "idd", "type": "uint", "values": list(range(1, 12))},
                           {"name": "tag", "type": "uint", "values": [1, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0]}]},
}

ONE_TWO_THREE = OP("or", T("one", 1), T("two", 2), T("three", 3))
W106 = {1: 1427, 2: 2414, 3: 3442, 4: 1427, 5: 2414, 6: 3442, 7: 1427, 8: 2414, 9: 3442}


def t146(line, name, text, query, expect, parse=True):
    c = {"name": "146 " + name, "corpus": "test_146", "source": "test/test_146/test.xml:%d" % line, "text": text, "query": query,
         "ranker": "proximity_bm25", "filters": [], "index_weight": 1, "sorter": {"sortmode": "extended", "sortby": "id asc"},
         "device": dict(BY_ID_ASC), "expect": expect, "total_found": len(expect)}
    if not parse:
        c["text_parse"] = "the query holds stopwords of the index (not, as): the parser knows no stopword list"
    return c


def t140(line, text, query, ids):
    return {"name": "140 " + text, "corpus": "test_140", "source": "test/test_140/test.xml:%d" % line, "text": text, "query": query,
            "ranker": "proximity_bm25", "filters": [], "index_weight": 1, "sorter": {"sphinxql": "order by idd asc"},
            "device": {"sort": {"attr": "idd", "desc": False, "then_weight": 0}},
            "weights": "not recorded (select * lists no weight())", "expect": [[i, None] for i in ids], "total_found": len(ids)}


CASES = [
    # ---- test_106: the one recorded result that shows rowid ascending last under a DESCENDING attribute (3 before 6, 2 before 5,
    # 1 before 4).  The rows of each pair carry equal weights, so this case does not tell then_weight 0 from 1 or 2: it is asked
    # with all three and must answer the same.
    {"name": "106 date_added DESC", "corpus": "test_106", "source": "test/test_106/test.xml:58", "text": "one|two|three", "query": ONE_TWO_THREE,
     "ranker": "proximity_bm25", "filters": [], "index_weight": 1, "sorter": {"sortmode": "extended", "sortby": "date_added DESC"},
     "device": {"sort": {"attr": "date_added", "desc": True, "then_weight": 0}}, "then_weight_any": True,
     "expect": [[i, W106[i]] for i in (9, 8, 7, 3, 6, 2, 5, 1, 4)], "total_found": 9},
    # the weight comes FIRST in these two: no mrk_query can say that (Sort / Order start with an attribute), and serving them as
    # plain relevance would be wrong (relevance ties on rowid ascending; here row 6 precedes row 3).  They pin the oracle's weights
    # and total_found only; README.md says why their tie order is not asserted.
    {"name": "106 @weight DESC, date_added DESC", "corpus": "test_106", "source": "test/test_106/test.xml:59", "text": "one|two|three",
     "query": ONE_TWO_THREE, "ranker": "proximity_bm25", "filters": [], "index_weight": 1,
     "sorter": {"sortmode": "extended", "sortby": "@weight DESC, date_added DESC"}, "device": "not expressible",
     "expect": [[i, W106[i]] for i in (9, 6, 3, 8, 5, 2, 7, 4, 1)], "total_found": 9},
    {"name": "106 @weight DESC, date_added DESC, id DESC", "corpus": "test_106", "source": "test/test_106/test.xml:60", "text": "one|two|three",
     "query": ONE_TWO_THREE, "ranker": "proximity_bm25", "filters": [], "index_weight": 1,
     "sorter": {"sortmode": "extended", "sortby": "@weight DESC, date_added DESC, id DESC"}, "device": "not expressible",
     "expect": [[i, W106[i]] for i in (9, 6, 3, 8, 5, 2, 7, 4, 1)], "total_found": 9},
    # ---- test_146, index test: twelve queries under sortby="id asc" -- ORDER BY id through Query.order with SORTKEY_INT64
    t146(134, "aaa", "aaa", T("aaa", 1), [[1, 1500], [2, 1500]]),
    t146(135, "bbb", "bbb", T("bbb", 1), [[2, 1500], [3, 1500]]),
    t146(136, "aaa | bbb", "aaa | bbb", OP("or", T("aaa", 1), T("bbb", 2)), [[1, 1500], [2, 2500], [3, 1500]]),
    t146(137, '"aaa bbb"', '"aaa bbb"', OP("phrase", T("aaa", 1), T("bbb", 2)), [[2, 2500]]),
    t146(138, '( kkk zzz ) | "do dog"', '( kkk zzz ) | "do dog"',
         OP("or", OP("and", T("kkk", 1), T("zzz", 2)), OP("phrase", T("do", 3), T("dog", 4))), [[1, 2590]]),
    t146(139, '( kkk zzz ) | "do not as dog"', '( kkk zzz ) | "do not as dog"',
         OP("or", OP("and", T("kkk", 1), T("zzz", 2)), OP("phrase", T("do", 3), T("dog", 6))), [[1, 2590], [3, 2590]], parse=False),
    t146(140, '"kkk zzz"', '"kkk zzz"', OP("phrase", T("kkk", 1), T("zzz", 2)), [[1, 2680]]),
    t146(141, '"zzz not as not cool"', '"zzz not as not cool"', OP("phrase", T("zzz", 1), T("cool", 5)), [[1, 2680]], parse=False),
    t146(142, '"zzz do dog look cool"/2', '"zzz do dog look cool"/2',
         OP("quorum", T("zzz", 1), T("do", 2), T("dog", 3), T("look", 4), T("cool", 5), opt=2), [[1, 2572], [3, 1572]]),
    t146(143, "dog not as do sleepy", "dog not as do sleepy", OP("and", T("dog", 1), T("do", 4), T("sleepy", 5)), [[3, 1680]], parse=False),
    t146(144, '"dog not as do sleepy"', '"dog not as do sleepy"', OP("phrase", T("dog", 1), T("do", 4), T("sleepy", 5)), [], parse=False),
    t146(145, '"do not as dog sleepy"', '"do not as dog sleepy"', OP("phrase", T("do", 1), T("dog", 4), T("sleepy", 5)), [[3, 3680]], parse=False),
    # ---- test_016: mode="any" = SPH_MATCH_ANY: the words as a quorum of 1 under the MATCHANY ranker ("text" is that rewrite, the
    # test's own text is `test it`).  sortmode="expr" sortby="@weight" is the relevance order.
    {"name": "016 any: test it, group_id = 1", "corpus": "test_016", "source": "test/test_016/test.xml:37", "text": '"test it"/1',
     "query": OP("quorum", T("test", 1), T("it", 2), opt=1), "ranker": "matchany", "filters": [{"attr": "group_id", "values": [1]}],
     "index_weight": 1, "sorter": {"sortmode": "expr", "sortby": "@weight"}, "device": {"relevance": True},
     "expect": [[444, 4], [111, 1], [222, 1]], "total_found": 3},
    # the same without the filter, under sortby="-@weight": the weight ASCENDING, ties by id ascending.  No mrk_query says "weight
    # first, ascending"; the rows and their weights are compared as a set (relevance order is asked of the device).
    {"name": "016 any: test it", "corpus": "test_016", "source": "test/test_016/test.xml:38", "text": '"test it"/1',
     "query": OP("quorum", T("test", 1), T("it", 2), opt=1), "ranker": "matchany", "filters": [], "index_weight": 1,
     "sorter": {"sortmode": "expr", "sortby": "-@weight"}, "device": {"relevance": True}, "unordered": True,
     "expect": [[111, 1], [222, 1], [333, 1], [444, 4]], "total_found": 4},
    # ---- test_140, index main: ORDER BY a uint attribute ascending (every idd is distinct; rows only, no weights)
    t140(85, "main", T("main", 1), [1, 2, 3, 7, 8]),
    t140(86, "delta", T("delta", 1), [1, 2, 3, 4, 5, 6, 9, 10, 11]),
    t140(87, "main | delta", OP("or", T("main", 1), T("delta", 2)), list(range(1, 12))),
]

G = {"_about": "Results the reference recorded for sorted, filtered and SPH_MATCH_ANY queries; data only, see README.md", "corpora": CORPORA, "cases": CASES}

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sorted_vectors.json")
    with open(out, "w", encoding="utf-8") as f:
        json.dump(G, f, ensure_ascii=False, indent=1)
        f.write("\n")
    print("wrote", out, len(CASES), "cases")
