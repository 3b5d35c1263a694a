"""Writes tests/golden/group_mva_vectors.json: results the reference recorded for GROUP BY a multi-value attribute.

The values below were copied by hand, as data, from the reference's own test directory while reading it (nothing of the reference
is imported or executed): the corpus = the (document_id, mva) columns of the <db_insert> rows of test/test_020/test.xml:167-176
(the uint variant of the index: 'sql_attr_multi = uint mva from field'; the MVA's stored values are the listed ones, sorted); the
queries = test.xml:121-122 -- the keyword 'test*' (min_prefix_len = 1: it matches all ten rows), groupattr = mva, groupfunc = attr,
groupsort = '@group desc' / '@group asc'; expected = the `matches` arrays of test_020's model.bin for those two queries, in the
order the daemon returned them: (id, weight, @groupby, @count), and total_found.  Both index variants of the test recorded the same
rows.

Every recorded weight is 1281, so inside a group all matches tie on the weight and the head is the group's smallest id: the recorded
head ids are determined by the recorded weights, and the model must reproduce them.  The queries order by the group key, so no two
groups tie.  'test*' needs prefix expansion, so the query does not run on the device from here: the fixture pins the numpy model
(tests/group_mva_expect.py), fed with the ten matches at the recorded weight.
Run:  python tests/golden/make_group_mva_vectors.py
"""
import json
import os

CORPUS = {"source": "test/test_020/test.xml:167-176",
          "rows": [[1, [1, 2, 3]], [2, [3, 4, 5]], [3, [4, 5, 6]], [4, [1, 2, 3]], [5, [3, 5]], [6, [3, 5]], [7, [4, 5]], [8, [4, 5, 6]], [9, [4]], [10, [3, 4, 5]]]}  # (id, mva)
WEIGHT = 1281

DESC = [[3, 1281, 6, 2], [2, 1281, 5, 7], [2, 1281, 4, 6], [1, 1281, 3, 6], [1, 1281, 2, 2], [1, 1281, 1, 2]]
ASC = DESC[::-1]
CASES = [
    {"source": "test/test_020/test.xml:121 + model.bin", "groupsort": "@group desc", "sort_by": "key", "desc": True, "total_found": 6, "matches": DESC},
    {"source": "test/test_020/test.xml:122 + model.bin", "groupsort": "@group asc", "sort_by": "key", "desc": False, "total_found": 6, "matches": ASC},
]

if __name__ == "__main__":
    out = {"about": "recorded by the reference (test/test_020): 'test*' GROUP BY mva; matches = (id, weight, @groupby, @count) in returned order",
           "max_matches": 1000, "weight": WEIGHT, "corpus": CORPUS, "cases": CASES}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "group_mva_vectors.json")
    with open(path, "w") as fp:
        json.dump(out, fp, indent=1)
        fp.write("\n")
    print("wrote", path, len(CASES), "cases")
