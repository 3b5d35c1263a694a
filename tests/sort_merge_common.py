"""Shared by the tests of the wide exchange rows (sorted queries across shards): an independent numpy statement of the sort key
map, packing of per-shard results into wide rows, decoding of merged rows.  Nothing here calls the library's map or merge."""
import dataclasses

import numpy as np

K1 = 1024  # MRK_MAX_K


def map_keys_np(raw, kind, desc):
    """Order-preserving 32-bit key of raw attribute values, larger = better -- written from the order's definition (unsigned
    compare for integers; float32 compare with -0.0 == +0.0 for floats), not from the library's code."""
    raw = np.asarray(raw, dtype=np.uint32)
    if kind == 1:
        v = np.where((raw << np.uint32(1)) == 0, np.uint32(0), raw)
        neg = (v >> np.uint32(31)) == 1
        m = np.where(neg, ~v, v | np.uint32(0x80000000)).astype(np.uint32)
    else:
        m = raw
    return m if desc else ~m


def fold_zero(raw, kind):
    """A float key of -0.0 folded onto +0.0 (the map does not keep the sign of zero)."""
    raw = np.asarray(raw, dtype=np.uint32)
    return np.where(raw == np.uint32(0x80000000), np.uint32(0), raw) if kind == 1 else raw


def make_keys(weight, docid):
    w = (np.asarray(weight).astype(np.int64).astype(np.uint64) ^ np.uint64(0x80000000)) & np.uint64(0xFFFFFFFF)
    return (w << np.uint64(32)) | ((~np.asarray(docid).astype(np.uint64)) & np.uint64(0xFFFFFFFF))


def pack_srow(mdist, docid, weight, total, sort=None, raw=None):
    """One wide row from a shard's answer (global docids, in the sorter's order)."""
    row = np.zeros(mdist.SROW_WORDS, np.uint64)
    n = len(docid)
    row[:n] = make_keys(weight, docid)
    row[K1] = n
    row[K1 + 1] = total
    if sort is not None:
        plane = np.zeros(K1, "<u4")
        plane[:n] = map_keys_np(raw, sort.kind, sort.desc)
        row[mdist.SROW_MKEYS:mdist.SROW_SPEC] = plane.view("<u8")
        row[mdist.SROW_SPEC] = mdist.sort_spec_word(sort.kind, sort.desc, sort.then_weight, sort.bit_count)
    return row


def decode_srow(mdist, row, k):
    """(docid, weight, raw sort key or None, total_found word) of a wide row, cut to k."""
    n = min(int(row[K1]), k)
    keys = row[:n]
    weight = ((keys >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)
    docid = ~keys.astype(np.uint32)
    spec = int(row[mdist.SROW_SPEC])
    sk = mdist.unmap_keys(spec, mdist.srow_mkeys(row)[:n]) if spec else None
    return docid, weight, sk, int(row[K1 + 1])


def assert_padding(mdist, row):
    """Zero past count: keys and mapped keys."""
    n = int(row[K1])
    assert not row[n:K1].any() and not mdist.srow_mkeys(row)[n:].any()
    if not int(row[mdist.SROW_SPEC]):
        assert not row[mdist.SROW_MKEYS:mdist.SROW_SPEC].any()


def shard_answer_row(mdist, orc, expected, to_orc, oi, q, rows, n_docs, base):
    """A shard's wide row for query q from the oracle (+ numpy for the order, as test_gpu_sort.expected builds it)."""
    if q.sort is None:
        r = to_orc(orc, q).run(oi)
        return pack_srow(mdist, r.rowid.astype(np.int64) + base, r.weight, r.total_found)
    rid, w, raw, total = expected(orc, oi, q, rows, n_docs)
    return pack_srow(mdist, rid.astype(np.int64) + base, w, total, q.sort, raw)


def check_merged_row(mdist, orc, expected, to_orc, oi, q, rows, n_docs, row, what=""):
    """A merged wide row against the unsharded expectation (oracle + numpy)."""
    assert not int(row[K1 + 1]) & (mdist.ROW_RERUN | mdist.ROW_DECLINED), (what, "flagged")
    assert_padding(mdist, row)
    docid, weight, sk, total = decode_srow(mdist, row, q.max_matches)
    if q.sort is None:
        r = to_orc(orc, q).run(oi)
        assert sk is None and total == r.total_found and np.array_equal(docid, r.rowid) and np.array_equal(weight, r.weight), what
        return
    rid, w, raw, tot = expected(orc, oi, q, rows, n_docs)
    assert total == tot, (what, total, tot)
    assert np.array_equal(docid, rid), (what, q.sort, q.max_matches, docid[:8], rid[:8])
    assert np.array_equal(weight, w), (what, weight[:8], w[:8])
    assert np.array_equal(sk, fold_zero(raw, q.sort.kind)), (what, sk[:8], raw[:8])


class Corpus:
    """One synthetic corpus, whole and cut into rowid-range shards, with attribute rows sliced at the same cuts."""

    def __init__(self, m, make_rows, n_docs, cuts, probs, seed, rows_seed, max_pos=64):
        self.n_docs, self.cuts, self.nt = n_docs, list(cuts), len(probs)
        self.whole = m.synth_index(n_docs, probs, seed=seed, max_pos=max_pos)
        self.shards = [m.synth_index(cuts[i + 1] - cuts[i], probs, seed=seed, max_pos=max_pos, rowid_base=cuts[i]) for i in range(len(cuts) - 1)]
        self.gdocs = {t: int(self.whole.dict[t]["docs"]) for t in range(self.nt)}
        assert all(self.gdocs[t] == sum(int(sh.dict[t]["docs"]) for sh in self.shards) for t in range(self.nt))
        self.rows = make_rows(np.random.default_rng(rows_seed), n_docs)
        self.shard_rows = [np.ascontiguousarray(self.rows[cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1)]

    def globalize(self, q):
        """The query with the corpus-wide document frequencies (local_df), so that every shard ranks as the whole does."""
        return dataclasses.replace(q, total_docs=self.n_docs, local_docs=dict(self.gdocs))


def grid_queries(m, sorts, kw, corpus):
    """Every sort column x asc / desc x then_weight 0 / 1 / 2 x K in {1, 10, 1000, 1024}, over three query shapes, with relevance
    queries mixed in."""
    roots = [(kw(m, 0, 1), m.SPH_RANK_BM25), (m.XQNode.AND(kw(m, 0, 1), kw(m, 1, 2)), m.SPH_RANK_PROXIMITY_BM25),
             (m.XQNode.AND(kw(m, 1, 1), kw(m, 2, 2)), m.SPH_RANK_NONE)]
    qs, i = [], 0
    for name, (off, cnt, kind) in sorts(m).items():
        for desc in (False, True):
            for tw in (0, 1, 2):
                for K in (1, 10, 1000, 1024):
                    root, rk = roots[i % 3]
                    qs.append(corpus.globalize(m.Query(root, ranker=rk, max_matches=K, sort=m.Sort(off, cnt, desc=desc, then_weight=tw, kind=kind))))
                    if i % 20 == 0:
                        qs.append(corpus.globalize(m.Query(root, ranker=rk, max_matches=K)))
                    i += 1
    return qs
