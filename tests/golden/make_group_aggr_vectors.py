"""Writes tests/golden/group_aggr_vectors.json: results the reference recorded for GROUP BY queries with SUM / MIN / MAX.

The values below were copied by hand, as data, from the reference's own test directory while reading it (nothing of the reference
is imported or executed).  The corpus = the (id, tag, gr) columns of the three rows the index dist_no holds in both tests (sql_query
... WHERE id<4 over the <db_insert> rows of test/test_153/test.xml:496-499 and test/test_171/test.xml:565-568); both attributes are
sql_attr_uint, i.e. SPH_ATTR_INTEGER sources: AggrSum_t<DWORD> / AggrMin_t<DWORD> / AggrMax_t<DWORD>.  The queries are full scans (no
MATCH: every row matches with weight 1); expected = the `rows` arrays of the tests' model.bin for those statements, in the order the
daemon returned them:

    test_153/test.xml:361   select gr, sum(tag) as t from dist_no group by gr                      -> (gr, t)
    test_171/test.xml:513-518 (the dist_no statement of each pair)
                            SELECT id, MIN(gr) aa, COUNT(*) cc, GROUPBY() gg FROM dist_no GROUP BY tag HAVING aa=2
                            SELECT id, MAX(gr) aa, ...                                       HAVING aa=3
                            SELECT id, SUM(gr) aa, ...                                       HAVING aa>5   -> (id, aa, cc, gg)

Each case restates its statement as columns of (rowid, weight, group value, source value) per row -- the id stands for the rowid (the
indexer numbers rows in document order) -- and the recorded groups as (head id or null where the statement does not select it, group
value, @count or null, aggregate).  SphinxQL's default order of the groups is weight DESC, id ASC over the heads, which is sort_by
"weight" descending here.  The HAVING clauses keep every group of these statements, so they change nothing.

Not taken: the dist0 .. dist3 / dist2 twins of these statements run over distributed indexes (agents, several local indexes), whose
merge is not the single sorter the model describes; test_171:519-520 use GROUP 8 BY (several rows per group).  No recorded case has
a sum that wraps, a BIGINT source or a negative value: the typing rules for those rest on the cited source lines alone
(sphinxsort.cpp:1902-1979, :2608-2693).
Run:  python tests/golden/make_group_aggr_vectors.py
"""
import json
import os

ROWS = [[1, 2, 3], [2, 2, 2], [3, 2, 3]]  # (id, tag, gr)
TAG, GR = 1, 2


def case(source, statement, func, group_col, source_col, groups):
    return {"source": source, "statement": statement, "func": func, "sort_by": "weight", "desc": True,
            "rows": [[r[0], 1, r[group_col], r[source_col]] for r in ROWS],  # (rowid, weight, group value, source value)
            "groups": groups}  # (head id | null, group value, @count | null, aggregate), in returned order


CASES = [
    case("test/test_153/test.xml:361 + model.bin", "select gr, sum(tag) as t from dist_no group by gr", "sum", GR, TAG, [[None, 3, None, 4], [None, 2, None, 2]]),
    case("test/test_171/test.xml:514 + model.bin", "SELECT id, MIN(gr) aa, COUNT(*) cc, GROUPBY() gg FROM dist_no GROUP BY tag HAVING aa=2", "min", TAG, GR, [[1, 2, 3, 2]]),
    case("test/test_171/test.xml:516 + model.bin", "SELECT id, MAX(gr) aa, COUNT(*) cc, GROUPBY() gg FROM dist_no GROUP BY tag HAVING aa=3", "max", TAG, GR, [[1, 2, 3, 3]]),
    case("test/test_171/test.xml:518 + model.bin", "SELECT id, SUM(gr) aa, COUNT(*) cc, GROUPBY() gg FROM dist_no GROUP BY tag HAVING aa>5", "sum", TAG, GR, [[1, 2, 3, 8]]),
]

if __name__ == "__main__":
    out = {"about": "recorded by the reference (test/test_153, test/test_171): full-scan GROUP BY with SUM / MIN / MAX of a uint attribute over the index dist_no",
           "max_matches": 1000, "cases": CASES}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "group_aggr_vectors.json")
    with open(path, "w") as fp:
        json.dump(out, fp, indent=1)
        fp.write("\n")
    print("wrote", path, len(CASES), "cases")
