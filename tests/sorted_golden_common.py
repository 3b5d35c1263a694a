"""Shared by tests/test_sorted_golden_cpu.py and tests/test_gpu_sorted_golden.py: tests/golden/sorted_vectors.json (results the
reference recorded for sorted, filtered and SPH_MATCH_ANY queries) turned into postings, attribute rows and Query objects, whole and
cut into rowid-range shards.  Nothing here knows an answer: the recorded lists are only translated from document ids to rowids."""
import dataclasses
import itertools
import json
import os

import numpy as np

from helpers import make_hits

G = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sorted_vectors.json"), encoding="utf-8"))
CASES = G["cases"]
EXPRESSIBLE = [c for c in CASES if c["device"] != "not expressible"]
FIELDS_OF_TEXT = {}  # corpus -> field names for the parser (none of the fixture's queries names a field)


class Corpus:
    """One corpus of the fixture: hits, vocabulary, attribute rows (the id as a bigint in dwords 0..1, low dword first; then every
    declared attribute: a uint / timestamp takes one dword, a bigint two) and the locator of every column."""

    def __init__(self, name):
        c = G["corpora"][name]
        self.name, self.c, self.ids, self.n = name, c, c["ids"], len(c["ids"])
        self.W, self.R, self.H, self.v = make_hits(c["docs"], c["min_word_len"], False, c.get("phrase_boundary", ""), c.get("phrase_boundary_step", 0))
        self.n_fields = max(len(d) for d in c["docs"])
        assert self.n_fields == len(c["fields"]) and not set(c.get("stopwords", [])) & set(self.v)  # (no row holds a stopword)
        cols = [("id", "bigint", self.ids)] + [(a["name"], a["type"], a["values"]) for a in c["attrs"]]
        self.loc, words = {}, []
        for nm, ty, vals in cols:
            assert len(vals) == self.n and ty in ("uint", "timestamp", "bigint")
            self.loc[nm] = (len(words) * 32, 64 if ty == "bigint" else 32, 2 if ty == "bigint" else 0)  # bit offset, bits, SORTKEY_*
            a = np.array(vals, np.int64)
            words.append((a & 0xFFFFFFFF).astype(np.uint32))
            if ty == "bigint":
                words.append(((a >> 32) & 0xFFFFFFFF).astype(np.uint32))
        self.rows = np.ascontiguousarray(np.stack(words, axis=1))
        self.rowid_of = {i: r for r, i in enumerate(self.ids)}
        hit_rows = np.unique(self.R)
        self.gdocs = {t: int(np.unique(self.R[self.W == t + 1]).size) for t in range(len(self.v))}
        assert hit_rows.size <= self.n

    def index(self, m, lo=0, hi=None):
        """the rows [lo, hi) as a segment of their own (local rowids from 0; the vocabulary is the whole corpus')"""
        hi = self.n if hi is None else hi
        keep = (self.R >= lo) & (self.R < hi)
        return m.index_from_hits(self.W[keep], self.R[keep] - np.uint32(lo), self.H[keep], n_terms=len(self.v), total_docs=hi - lo, n_fields=self.n_fields)

    def globalize(self, q):
        """the query with the corpus-wide document frequencies (local_df), so that every shard ranks as the whole does"""
        return dataclasses.replace(q, total_docs=self.n, local_docs=dict(self.gdocs))

    def cuts(self, shards):
        """every way to cut the rows into `shards` non-empty rowid ranges"""
        return [[0] + list(c) + [self.n] for c in itertools.combinations(range(1, self.n), shards - 1)]


def tree(m, v, q):
    ops = {"and": m.SPH_QUERY_AND, "or": m.SPH_QUERY_OR, "phrase": m.SPH_QUERY_PHRASE, "quorum": m.SPH_QUERY_QUORUM}
    if "word" in q:
        return m.XQNode.keyword(v.get(q["word"], -1), q["pos"], q["mask"])  # -1: not in the dictionary
    return m.XQNode(ops[q["op"]], [tree(m, v, k) for k in q["kids"]], None, q["mask"], q.get("opt", 0))


def parses(case):
    return "text_parse" not in case


def root_of(m, corpus, case, from_text):
    if not from_text:
        return tree(m, corpus.v, case["query"])
    assert parses(case)
    # (transform: what every query goes through between the parser and the ranker)
    return m.parse_query(case["text"], FIELDS_OF_TEXT.get(corpus.name, []), corpus.c["min_word_len"], lookup=lambda w: corpus.v.get(w, -1), transform=True)


def base_query(m, corpus, case, from_text=False, K=None):
    rankers = {"proximity_bm25": m.SPH_RANK_PROXIMITY_BM25, "matchany": m.SPH_RANK_MATCHANY}
    fl = []
    for f in case["filters"]:
        off, bits, _ = corpus.loc[f["attr"]]
        fl.append(m.Filter(off, bits, values=f["values"]))
    return m.Query(root_of(m, corpus, case, from_text), ranker=rankers[case["ranker"]], max_matches=K or corpus.n, index_weight=case["index_weight"], filters=fl or None)


def spellings(m, corpus, case, q):
    """[(label, query)]: the case's order in every way the device can be asked for it -- a one-attribute sort as Query.sort and as
    a one-part Query.order; the id as SORTKEY_INT64; a case that does not tell the tie rules apart under all three of them."""
    d = case["device"]
    ties = (0, 1, 2) if case.get("then_weight_any") else None
    out = []
    if "relevance" in d:
        return [("relevance", q)]
    if "sort" in d:
        s = d["sort"]
        off, bits, kind = corpus.loc[s["attr"]]
        assert bits == 32
        for t in ties or (s["then_weight"],):
            out.append((f"sort tw{t}", dataclasses.replace(q, sort=m.Sort(off, bits, desc=s["desc"], then_weight=t, kind=kind))))
            out.append((f"order tw{t}", dataclasses.replace(q, order=m.Order([m.OrderPart(off, bits, desc=s["desc"], kind=kind)], then_weight=t))))
        return out
    o = d["order"]
    parts = [m.OrderPart(corpus.loc[p["attr"]][0], corpus.loc[p["attr"]][1], desc=p["desc"], kind=corpus.loc[p["attr"]][2]) for p in o["parts"]]
    for t in ties or (o["then_weight"],):
        out.append((f"order tw{t}", dataclasses.replace(q, order=m.Order(parts, then_weight=t))))
    return out


def recorded(corpus, case, K=None):
    """(rowids, weights or None, total_found) of the recorded list, cut to K"""
    exp = case["expect"][:K]
    rid = np.array([corpus.rowid_of[i] for i, _ in exp], np.uint32)
    w = None if any(x is None for _, x in exp) else np.array([x for _, x in exp], np.int32)
    return rid, w, case["total_found"]


def recorded_key(corpus, q, rid):
    """the attribute values the recorded rows carry, in Matches.sort_key's / order_key's format"""
    if q.sort is not None:
        return corpus.rows[rid, q.sort.bit_offset >> 5]
    p = q.order.parts
    if p[0].kind == 2:
        it = p[0].bit_offset >> 5
        return np.ascontiguousarray(corpus.rows[rid, it:it + 2]).view(np.uint64).reshape(-1)
    k = corpus.rows[rid, p[0].bit_offset >> 5].astype(np.uint64) << np.uint64(32)
    return k | corpus.rows[rid, p[1].bit_offset >> 5].astype(np.uint64) if len(p) > 1 else k


def assert_answer(case, what, rid, weight, total, want):
    """an answer (rowids in order, weights, total_found) against the recorded list"""
    wr, ww, wt = want
    assert total == wt, (what, total, wt)
    if case.get("unordered"):
        got = sorted(zip(rid.tolist(), weight.tolist()))
        assert got == sorted(zip(wr.tolist(), ww.tolist())), (what, got)
        return
    assert rid.tolist() == wr.tolist(), (what, rid.tolist(), wr.tolist())
    if ww is not None:
        assert weight.tolist() == ww.tolist(), (what, weight.tolist(), ww.tolist())
