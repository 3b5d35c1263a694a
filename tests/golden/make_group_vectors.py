"""Writes tests/golden/group_vectors.json: results the reference recorded for GROUP BY queries over one integer attribute.

The values below were copied by hand, as data, from the reference's own test directory while reading it (nothing of the reference
is imported or executed): the corpus = the (document_id, tag) columns of the <db_insert> rows of test/test_020/test.xml:182-193;
the queries = test.xml:112-116 -- full scans (empty query text: every row matches with weight 1) with groupattr = tag, groupfunc =
attr and the five groupsort clauses; expected = the `matches` arrays of test_020's model.bin for those five queries, in the order
the daemon returned them (a PHP array keeps insertion order): (id, weight, @groupby, @count), and total_found.  Both index variants
of the test (uint / bigint MVA) recorded the same rows.

'groupsort = tag desc' orders the groups by the head's own tag attribute, which IS the group key: it is recorded as sort_by "key".

Not taken: test.xml:117-122 group by day / week / month / year or by an MVA; :124-129 use groupdistinct; :130-131 are GROUP BY tag
over the keyword 'test*', which needs prefix expansion (min_prefix_len = 1) and a within-group order other than relevance
(sortby = time asc / id desc).  None of the recorded grouped cases of this test can be written as a full-text mrk_query over
keywords, so none runs on the device from here.
Run:  python tests/golden/make_group_vectors.py
"""
import json
import os

CORPUS = {"source": "test/test_020/test.xml:182-193", "rows": [[1, 1], [2, 2], [3, 2], [4, 3], [5, 3], [6, 3], [7, 4], [8, 4], [9, 4], [10, 4]]}  # (id, tag)

DESC = [[7, 1, 4, 4], [4, 1, 3, 3], [2, 1, 2, 2], [1, 1, 1, 1]]
ASC = [[1, 1, 1, 1], [2, 1, 2, 2], [4, 1, 3, 3], [7, 1, 4, 4]]
CASES = [
    {"source": "test/test_020/test.xml:112 + model.bin", "groupsort": "@group desc", "sort_by": "key", "desc": True, "total_found": 4, "matches": DESC},
    {"source": "test/test_020/test.xml:113 + model.bin", "groupsort": "@group asc", "sort_by": "key", "desc": False, "total_found": 4, "matches": ASC},
    {"source": "test/test_020/test.xml:114 + model.bin", "groupsort": "@count desc", "sort_by": "count", "desc": True, "total_found": 4, "matches": DESC},
    {"source": "test/test_020/test.xml:115 + model.bin", "groupsort": "@count asc", "sort_by": "count", "desc": False, "total_found": 4, "matches": ASC},
    {"source": "test/test_020/test.xml:116 + model.bin", "groupsort": "tag desc", "sort_by": "key", "desc": True, "total_found": 4, "matches": DESC},
]

if __name__ == "__main__":
    out = {"about": "recorded by the reference (test/test_020): full-scan GROUP BY tag; matches = (id, weight, @groupby, @count) in returned order",
           "max_matches": 1000, "corpus": CORPUS, "cases": CASES}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "group_vectors.json")
    with open(path, "w") as fp:
        json.dump(out, fp, indent=1)
        fp.write("\n")
    print("wrote", path, len(CASES), "cases")
