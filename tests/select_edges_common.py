"""Corpora and the expectation of the relevance top-K selection's edge tests (csrc/mrk_select.hip), shared by test_select_edges_cpu.py
(which asserts that every corpus has the structure its case names) and test_gpu_select_edges.py (which runs them on the device).
Everything is built through m.index_from_hits from explicit, deterministic hits: a doc's weight class is its tf of one keyword.

The sorter's order is weight descending, then rowid ascending (MatchRelevanceLt_fn).  The expectation is that definition applied to
the oracle's FULL match list -- never the oracle's own K-sized queue, which the CPU test holds against it instead."""
import dataclasses

import numpy as np

FIELD = 1  # every hit lies in field 1 of 2: field 0's weight never reaches a match (case E puts an absurd one there)

# ---- the shared corpus of cases A, B, D, E: 240 000 rowids, every fourth holds both keywords a (term 0, tf 1) and b (term 1)
SHARED_DOCS, SHARED_MATCHES = 240_000, 60_000
LADDERS = {"L1": (300, 500, 59_200), "L2": (300, 6_000, 53_700), "ONE": (0, 0, 60_000)}  # docs with b's tf = 3 (best) / 2 / 1
PLACEMENTS = ("low", "high", "even")
LADDER_KS = {"L1": (1, 299, 300, 301, 799, 800, 801, 1000, 1024), "L2": (301, 1000, 1024), "ONE": (1, 2, 1000, 1024)}
BASES = (0, 1 << 24, (1 << 32) - SHARED_DOCS)  # case D: rowid bins of a small shift, of 15, and the clamped bin 0 of shift 22
FALLBACK_FIELD_WEIGHTS = (2_200_000, 1)  # case E: bins_by_weight's estimate leaves int32 (field 0 x 1000); no match has a hit in field 0

# ---- the corpus of cases C and G: nine rare keywords (terms 0..8) of exactly these many docs, and a dense one (term 9)
SLICE_DOCS = 65_536
SLICE_COUNTS = (1, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6145)
SLICE_DENSE = 9
SLICE_TOP = 10  # the highest rowids of each rare keyword have tf 2: a class on top that the scan finds last

# ---- case F: more candidates than one chunk of SCH = 1024 slices holds.  The keyword's docs are rowids 0 .. 2 199 999 of a rowid space four
# times as large (in every doc its idf would be negative and the tf-2 class the WORSE one)
CHUNK_DOCS, CHUNK_TOP, CHUNK_ROWIDS = 2_200_000, 700, 8_800_000


def _hits_of(term, rows, tf, first_pos):
    """hits of one keyword: rows ascending, tf[i] hits in doc rows[i] at positions first_pos.."""
    rows = np.asarray(rows, np.uint32)
    tf = np.asarray(tf, np.int64)
    R = np.repeat(rows, tf)
    start = np.repeat(np.cumsum(tf) - tf, tf)
    pos = np.arange(R.size, dtype=np.int64) - start + first_pos
    return np.full(R.size, term + 1, np.uint64), R, ((FIELD << 24) | pos).astype(np.uint32)


def _index(m, parts, n_terms, total_docs):
    W, R, H = (np.concatenate([p[i] for p in parts]) for i in range(3))
    return m.index_from_hits(W, R, H, n_terms=n_terms, total_docs=total_docs, n_fields=2)


def ladder_tf(ladder, placement):
    """b's tf of the shared corpus's matches, in rowid order"""
    best, second, rest = LADDERS[ladder]
    n = SHARED_MATCHES
    assert best + second + rest == n
    tf = np.ones(n, np.int64)
    if placement == "low":
        tf[:best], tf[best:best + second] = 3, 2
    elif placement == "high":
        tf[n - best:], tf[n - best - second:n - best] = 3, 2
    else:
        if best:
            tf[(np.arange(best, dtype=np.int64) * n) // best] = 3
        left = np.flatnonzero(tf == 1)
        if second:
            tf[left[(np.arange(second, dtype=np.int64) * left.size) // second]] = 2
    assert (np.bincount(tf, minlength=4)[1:] == (rest, second, best)).all()
    return tf


def shared_index(m, ladder, placement):
    rows = np.arange(SHARED_MATCHES, dtype=np.uint32) * 4
    return _index(m, [_hits_of(0, rows, np.ones(rows.size, np.int64), 1), _hits_of(1, rows, ladder_tf(ladder, placement), 2)], 2, SHARED_DOCS)


def slice_rows(t):
    """the docs of rare keyword t (or of the dense one): a fixed pseudo-random draw"""
    if t == SLICE_DENSE:
        return np.arange(SLICE_DOCS // 4, dtype=np.uint32) * 4 + 1
    return np.sort(np.random.default_rng(1000 + t).choice(SLICE_DOCS, SLICE_COUNTS[t], replace=False)).astype(np.uint32)


def slice_index(m):
    parts = []
    for t, n in enumerate(SLICE_COUNTS):
        tf = np.ones(n, np.int64)
        tf[-SLICE_TOP:] = 2
        parts.append(_hits_of(t, slice_rows(t), tf, 1))
    rows = slice_rows(SLICE_DENSE)
    parts.append(_hits_of(SLICE_DENSE, rows, np.ones(rows.size, np.int64), 20))
    return _index(m, parts, len(SLICE_COUNTS) + 1, SLICE_DOCS)


def chunk_index(m):
    tf = np.ones(CHUNK_DOCS, np.int64)
    tf[-CHUNK_TOP:] = 2
    return _index(m, [_hits_of(0, np.arange(CHUNK_DOCS, dtype=np.uint32), tf, 1)], 1, CHUNK_ROWIDS)


# ---- queries
def q_and(m, K, ranker=None, **kw):
    k = m.XQNode.keyword
    return m.Query(m.XQNode.AND(k(0, 1), k(1, 2)), ranker=m.SPH_RANK_BM25 if ranker is None else ranker, max_matches=K, **kw)


def q_one(m, t, K):
    return m.Query(m.XQNode.keyword(t, 1), ranker=m.SPH_RANK_BM25, max_matches=K)


def q_with_dense(m, t, K=1000):
    k = m.XQNode.keyword
    return m.Query(m.XQNode.AND(k(t, 1), k(SLICE_DENSE, 2)), ranker=m.SPH_RANK_BM25, max_matches=K)


def slice_batch(m):
    """case C's batch, in keyword order: the candidate lists' offsets are no multiples of 2048 and consecutive queries' slice counters
    are neighbours"""
    ts = range(len(SLICE_COUNTS))
    return [q_one(m, t, 1000) for t in ts] + [q_one(m, t, 1024) for t in ts] + [q_with_dense(m, t) for t in ts]


GROUP_QUERIES = 4100


def group_batch(m):
    """case G: (keyword, K) per query, cycling; queries 4093..4099 are the 4097-, 6143- and 6145-doc keywords (terms 6..8), the first
    of them the last ones of the first filter group (SEL_MAXQ = 4096), the rest the second group"""
    ks = (1, 1000, 1024)
    out = [(i % 9, ks[(i // 9) % 3]) for i in range(GROUP_QUERIES)]
    for i in range(4093, GROUP_QUERIES):
        out[i] = (6 + (i - 4093) % 3, ks[(i - 4093) % 3])
    return out


# ---- the expectation
def oracle_index(orc, hi):
    oi = orc.Index(hi.spd, hi.spp, hi.spe, hi.dict.view(orc.DICT_DTYPE), hi.total_docs, hi.skiplist_block_size, hi.hit_format, hi.n_fields)
    oi.host = hi  # (the oracle's arrays are views into the host index: it must outlive them)
    return oi


def full_list(orc, oi, q):
    """every match of q with its weight, as the oracle returns them with a queue that holds them all"""
    from test_gpu_parity import to_orc

    r = to_orc(orc, dataclasses.replace(q, max_matches=int(oi.total_docs))).run(oi)
    assert len(r.rowid) == r.total_found
    return r


def cut(full, K):
    """the definition: weight descending, then rowid ascending, cut to K -> (rowids, weights, total)"""
    order = np.lexsort((full.rowid, -full.weight.astype(np.int64)))[:K]
    return full.rowid[order], full.weight[order], int(full.total_found)


def expected_topk(orc, oi, q):
    return cut(full_list(orc, oi, q), q.max_matches)


def classes(full):
    """[(weight, docs)] of a full list, best class first"""
    w, n = np.unique(full.weight, return_counts=True)
    return [(int(a), int(b)) for a, b in zip(w[::-1], n[::-1])]


def rank_class(cls, K):
    """(index, docs above it) of the class that holds rank K (the last class if the list is shorter)"""
    above = 0
    for i, (_, n) in enumerate(cls):
        if above + n >= K or i == len(cls) - 1:
            return i, above
        above += n


class Corpora:
    """the corpora by name, each built once (a module-scoped fixture of either test file holds one of these):
    ("shared", ladder, placement), ("slices",), ("chunks",)  ->  (host index, oracle index)"""

    def __init__(self, m, orc):
        self.m, self.orc, self._built, self._full = m, orc, {}, {}

    def get(self, *name):
        if name not in self._built:
            hi = shared_index(self.m, *name[1:]) if name[0] == "shared" else slice_index(self.m) if name[0] == "slices" else chunk_index(self.m)
            self._built[name] = (hi, oracle_index(self.orc, hi))
        return self._built[name]

    def full(self, name, key, q):
        """the full list of query q on corpus `name`, computed once per `key` (the query without its K) and left unchanged"""
        if (name, key) not in self._full:
            r = full_list(self.orc, self.get(*name)[1], q)
            r.rowid.setflags(write=False), r.weight.setflags(write=False)
            self._full[(name, key)] = r
        return self._full[(name, key)]

    def want(self, name, key, q):
        return cut(self.full(name, key, q), q.max_matches)
