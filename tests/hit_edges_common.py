"""Corpora, a model of the read-ahead window and a model of the weights for the hit-stream decoders' edge suite
(test_hit_edges_cpu.py, test_gpu_hit_edges.py).

The device holds three hand-written decoders of the .spp byte stream (delta VLB, 7-bit groups most significant first, 0-terminated):
read_vlb32 / hit_advance (two aligned dwords and a funnel shift), hs_fill / hs_advance (a 16-byte window, refilled when the offset
passes 11) and the `next` lambda of hit_rank_prox (the same window with its own base / offset bookkeeping).  What can go wrong in them
depends on a varint's LENGTH and on its OFFSET in the window, so the corpora are built from crafted hitlists:

    k one-byte deltas (k = 0..15), one probe delta of encoded length L, a tail of 0..3 one-byte deltas

A list starts at position 1 of field 0 and steps by 2, which leaves the odd / even neighbour free.  L = 2 and 3 are position jumps inside
the field, L = 4 is a position jump of >= 2^21 ('4p') or a field change of 1..15 ('4f'), L = 5 a field change of >= 16 (32-field
corpus only).  The probe's 7-bit groups are all different from each other, from the one-byte deltas and from 0, so a byte taken from the
wrong place shows.  Some more lists carry the end flag (bit 23) on their last hit or on the hit in front of a field change: the deltas
next to it cross the flag.

Five keywords: C, D, E (dictionary slots 0-2), A and B (3, 4).  A's and B's lists are the last of .spp, and the highest rowid holds a
crafted list on B, which therefore ends on the file's last byte.  Every doc holds all five.  In the `A` range the crafted list is A's and
B, C, D, E have one hit each right behind its last position (last + 1 .. last + 4, same field); in the `B` range the list is B's, A sits
at last - 1 and C, D, E at last + 1 .. last + 3.  LCS, phrase, NEAR and BEFORE outcomes thus hang on the CUMULATIVE position of the
list: one wrong delta anywhere breaks the adjacency.  In 40 control docs the neighbours stand two positions apart.  The rowids are a
fixed permutation of the docs, so neighbouring lanes differ in k, L and alignment.

Extremes: a lone hit in the highest field with and without the end flag; position 2^23 - 1 as a lone hit and as a list's last hit (the
neighbours stand in front of it there); a list whose first delta is 5 bytes; lists of more than 300 hits.
"""
import functools

import numpy as np

T_C, T_D, T_E, T_A, T_B = 0, 1, 2, 3, 4
N_TERMS = 5
QPOS = {T_A: 1, T_B: 2, T_C: 3, T_D: 4, T_E: 5}
END = 1 << 23
POS_MASK = END - 1
MAX_POS = END - 1
PRIMES = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131]
HI_FIELDS = 0xFFFF0000  # a field limit that names fields 16-31 only
N_CONTROLS = 40
PERM_SEED = {8: 1, 32: 2}  # the docs' order: test_hit_edges_cpu.py asserts that every edge is reached under it, in every segment


# --------------------------------------------------------------------------- the byte stream
def vlb_len(v):
    return 1 if v < 1 << 7 else 2 if v < 1 << 14 else 3 if v < 1 << 21 else 4 if v < 1 << 28 else 5


def read_vlb(spp, p):
    """-> (value, length) of the varint at byte p"""
    v = 0
    for n in range(1, 6):
        b = int(spp[p + n - 1])
        v = (v << 7) | (b & 0x7F)
        if not b & 0x80:
            return v, n
    raise AssertionError(f"a varint of more than 5 bytes at {p}")


def window_trace(spp, p):
    """The window discipline hs_advance and hit_rank_prox's `next` share, restated: the window starts at p rounded down to a dword,
    off = p & 3; before a varint is decoded, off > 11 (fewer than 5 bytes left) makes a refill, which leaves off & 3.
    -> ([(length, off) per varint, the terminator last], hits decoded, refills as [(length of the varint behind the refill)], end)
    where end = the position of the terminator byte.  read_vlb32 needs (length, p & 3) only, which is (length, off & 3)."""
    off = p & 3
    trace, hits, refills, cur = [], [], [], 0
    while True:
        fresh = off > 11
        if fresh:
            off &= 3
        v, n = read_vlb(spp, p)
        assert off + n <= 16
        trace.append((n, off))
        if fresh:
            refills.append(n)
        if v == 0:
            assert n == 1
            return trace, hits, refills, p
        cur += v
        hits.append(cur)
        p += n
        off += n


# --------------------------------------------------------------------------- crafted hitlists
def probe_groups(n, salt):
    """n different 7-bit groups in 3..127 (never 0, 1 or 2: the terminator and the one-byte deltas)"""
    return [(37 + 29 * salt + 41 * i) % 125 + 3 for i in range(n)]


def groups_value(gs):
    v = 0
    for g in gs:
        v = (v << 7) | g
    return v


def craft(k, variant, tail, n_fields, salt, flag=0):
    """One crafted hitlist as raw Hitpos_t values.  flag: 1 = the end flag on the last hit, 2 = on the hit in front of the probe (k >= 1,
    a probe that changes the field)."""
    f, pos, hits = 0, 0, []
    for i in range(k):
        pos += 1 if i == 0 else 2
        hits.append(pos)
    if flag == 2:
        assert k >= 1 and variant in ("4f", "5")
        hits[-1] |= END
    if variant in (1, 2, 3):
        pos += groups_value(probe_groups(variant, salt))
    elif variant == "4p":
        pos += ((1 + salt % 2) << 21) | groups_value(probe_groups(3, salt))
    else:
        lo, hi = (1, min(15, n_fields - 1)) if variant == "4f" else (16 + (flag == 2), n_fields - 1)
        f = lo + salt % (hi - lo + 1)
        pos += groups_value(probe_groups(3, salt))
    want = 4 if variant in ("4p", "4f") else variant if isinstance(variant, int) else 5
    hits.append((f << 24) | pos)
    assert vlb_len(hits[-1] - (hits[-2] if k else 0)) == want, (k, variant, salt, flag)
    for _ in range(tail):
        pos += 2
        hits.append((f << 24) | pos)
    if flag == 1:
        hits[-1] |= END
    assert all(1 <= (h & POS_MASK) for h in hits) and (hits[-1] & POS_MASK) + 8 < MAX_POS
    return hits


def variants_of(n_fields):
    return [1, 2, 3, "4p", "4f"] + (["5"] if n_fields > 16 else [])


def grid(n_fields):
    """(k, variant, tail) of the full grid: 16 x 5 x 4 = 320 lists for 8 fields, 16 x 6 x 4 = 384 for 32"""
    return [(k, v, t) for k in range(16) for v in variants_of(n_fields) for t in range(4)]


class Doc:
    """One doc: term -> raw hits, and what it was made for"""

    def __init__(self, kind, slot, hits):
        self.kind, self.slot, self.hits = kind, slot, hits


def with_neighbours(kind, slot, lst, step=1, nb_flag=False, before=False):
    """The crafted list on keyword `slot`, the other four keywords with one hit each around its last position."""
    last = lst[-1]
    base, lp, fl = last & ~POS_MASK & ~END, last & POS_MASK, END if nb_flag else 0
    if before:  # (the last position is the highest there is: everybody else stands in front of it)
        others = [T_B if slot == T_A else T_A, T_C, T_D, T_E]
        hits = {t: [base | (lp - 1 - i)] for i, t in enumerate(others)}
    elif slot == T_A:
        hits = {t: [base | fl | (lp + step * (i + 1))] for i, t in enumerate((T_B, T_C, T_D, T_E))}
    else:
        back = 1 if step == 1 else 2  # (a control's list has no tail: last - 2 is free)
        assert lp - back >= 1 and base | (lp - back) not in lst
        hits = {T_A: [base | (lp - back)]}
        hits.update({t: [base | fl | (lp + step * (i + 1))] for i, t in enumerate((T_C, T_D, T_E))})
    hits[slot] = list(lst)
    return Doc(kind, slot, hits)


def long_list(n_fields, slot_salt):
    """more than 300 hits in one doc: 150 one-byte deltas, a 3-byte jump, 120 more, a field change, 40 more"""
    hits, pos = [], 0
    for i in range(150):
        pos += 1 if i == 0 else 2
        hits.append(pos)
    pos += groups_value(probe_groups(3, slot_salt))
    for _ in range(120):
        hits.append(pos)
        pos += 2
    f = n_fields - 1 - slot_salt
    for _ in range(40):
        hits.append((f << 24) | pos)
        pos += 2
    return hits


@functools.lru_cache(maxsize=None)
def corpus_docs(n_fields):
    """-> the docs in rowid order.  8 fields: the corpus N, 32 fields: W."""
    top = n_fields - 1
    docs, pinned = [], None
    for slot in (T_A, T_B):
        for i, (k, v, t) in enumerate(grid(n_fields)):
            d = with_neighbours("grid", slot, craft(k, v, t, n_fields, salt=i + 7 * (slot == T_B)))
            d.cell = (k, v, t)
            if slot == T_B and (k, v, t) == (6, variants_of(n_fields)[-1], 0):
                pinned = d  # the longest probe, then the terminator: .spp's last two varints
            else:
                docs.append(d)
    # the end flag on the last hit (A's lists: 'A$' accepts that hit alone) and in front of a field change (B's lists)
    for i, (k, v, t) in enumerate((k, v, t) for k in (2, 7, 12) for v in variants_of(n_fields) for t in (0, 1, 3)):
        docs.append(with_neighbours("flag_last", T_A, craft(k, v, t, n_fields, salt=3 * i + 1, flag=1), nb_flag=True))
    for i, (k, v, t) in enumerate((k, v, t) for k in (1, 6, 11, 15) for v in variants_of(n_fields)[4:] for t in (0, 2)):
        docs.append(with_neighbours("flag_mid", T_B, craft(k, v, t, n_fields, salt=5 * i + 2, flag=2)))
    # controls: the neighbours two positions apart
    vs = variants_of(n_fields)
    for i in range(N_CONTROLS):
        slot = T_A if i % 2 == 0 else T_B
        docs.append(with_neighbours("control", slot, craft(3 + i % 10, vs[i % len(vs)], i % 4 if slot == T_A else 0, n_fields, salt=11 * i + 3), step=2))
    # extremes
    for slot in (T_A, T_B):
        docs.append(with_neighbours("lone_top", slot, [(top << 24) | 5]))
        docs.append(with_neighbours("lone_top_end", slot, [(top << 24) | END | 9], nb_flag=True))
        docs.append(with_neighbours("max_pos_lone", slot, [((top // 2) << 24) | MAX_POS], before=True))
        docs.append(with_neighbours("max_pos_last", slot, [1, 3, 5, MAX_POS], before=True))
        docs.append(with_neighbours("max_pos_last_end", slot, [1, 3, (top << 24) | 7, (top << 24) | END | MAX_POS], before=True))
        docs.append(with_neighbours("first_delta_long", slot, [(top << 24) | 1, (top << 24) | 3, (top << 24) | 5]))
        docs.append(with_neighbours("long", slot, long_list(n_fields, int(slot == T_B))))
    n = len(docs)
    perm = np.random.default_rng(PERM_SEED[n_fields]).permutation(n)
    out = [docs[i] for i in perm] + [pinned]
    assert len(out) <= 1000
    return out


def hits_of(docs):
    """-> index_from_hits' arrays, sorted by (wordid, rowid, hitpos)"""
    rows = [(t + 1, r, h) for r, d in enumerate(docs) for t, hs in d.hits.items() for h in hs]
    a = np.array(sorted(rows), np.uint64)
    return a[:, 0].copy(), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32)


SEGMENTS = [("N-inline-128", 8, 1, 128), ("N-plain-128", 8, 0, 128), ("W-inline-128", 32, 1, 128), ("W-plain-128", 32, 0, 128),
            ("W-inline-32", 32, 1, 32)]
SEGMENT_IDS = [s[0] for s in SEGMENTS]


@functools.lru_cache(maxsize=None)
def segment(name):
    """-> (HostIndex, docs) of one of SEGMENTS"""
    import manticoresearch_amd as m

    _, n_fields, fmt, block = next(s for s in SEGMENTS if s[0] == name)
    docs = corpus_docs(n_fields)
    W, R, H = hits_of(docs)
    hi = m.index_from_hits(W, R, H, n_terms=N_TERMS, total_docs=len(docs), skiplist_block_size=block, hit_format=fmt, n_fields=n_fields)
    return hi, docs


def stored_lists(oi, term):
    """-> [(rowid, .spp position)] of the hitlists of `term` that live in .spp (an inlined lone hit does not), from the doclist bytes"""
    rowid, _, _, hp = oi.decode_doclist(term)
    return [(int(r), int(p)) for r, p in zip(rowid, hp) if not int(p) >> 63]


# --------------------------------------------------------------------------- queries
def kw(m, t, mask=0xFFFFFFFF, pos=None, **mods):
    return m.XQNode.keyword(t, QPOS[t] if pos is None else pos, mask, **mods)


def routes(m, n_fields):
    """-> {route: [Query]}: every batch holds the queries of ONE rank pass, so that mrk_batch_stats.mq_chunks can be asserted.
    P = lean, hit_rank_prox<2/3/4>; L = lean, hit_rank_plain; F = queue 1, hit_pass (+ termpos_any / notnear_any in the scan);
    S_bm25 / S_prox = a phrase leaf decided in the scan; G = queue 2, the generic evaluator."""
    wide = n_fields > 16
    fw = PRIMES[:n_fields]
    A, B, C, D, E = T_A, T_B, T_C, T_D, T_E
    some = HI_FIELDS if wide else 0xFC  # fields behind a field change only

    def q(root, ranker):
        return m.Query(root, ranker=ranker, max_matches=1000, field_weights=fw)

    def node(op, kids, opt=0):
        return m.XQNode(op, kids, None, m.ALL_FIELDS, opt)

    AND = m.XQNode.AND
    ands = [AND(kw(m, A), kw(m, B)), AND(kw(m, A), kw(m, B), kw(m, C)), AND(kw(m, A), kw(m, B), kw(m, C), kw(m, D))]
    out = {}
    prox = [m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_PROXIMITY]
    p_roots = ands + [AND(kw(m, A, some), kw(m, B)), AND(kw(m, A), kw(m, B, some), kw(m, C), kw(m, D))]
    out["P"] = [q(r, rk) for r in p_roots for rk in prox]
    plain = [m.SPH_RANK_SPH04, m.SPH_RANK_WORDCOUNT, m.SPH_RANK_MATCHANY, m.SPH_RANK_FIELDMASK]
    out["L"] = [q(r, rk) for r in ands + [node(m.SPH_QUERY_OR, [kw(m, A), kw(m, B)])] for rk in plain]
    out["L"] += [q(AND(kw(m, A, pos=1), kw(m, B, pos=2), kw(m, A, pos=3)), rk) for rk in prox]  # repeated keyword
    out["L"] += [q(AND(kw(m, B, pos=1), kw(m, A, pos=2), kw(m, B, pos=3)), m.SPH_RANK_PROXIMITY_BM25)]
    out["L"] += [q(AND(kw(m, A, some), kw(m, B), kw(m, C)), rk) for rk in prox]  # the MergeHits3 quirk
    out["L"] += [q(AND(kw(m, A), kw(m, B, some), kw(m, C)), m.SPH_RANK_WORDCOUNT)]
    f_roots = [node(m.SPH_QUERY_PHRASE, [kw(m, A), kw(m, B)]),
               node(m.SPH_QUERY_PROXIMITY, [kw(m, A), kw(m, B)], 3),
               node(m.SPH_QUERY_BEFORE, [kw(m, A), kw(m, B)]),
               node(m.SPH_QUERY_NEAR, [kw(m, A), kw(m, B)], 2),
               node(m.SPH_QUERY_NOTNEAR, [kw(m, A), kw(m, B)], 2),
               node(m.SPH_QUERY_NOTNEAR, [kw(m, B), kw(m, A)], 2),
               AND(kw(m, C, field_start=True), kw(m, A)),
               AND(kw(m, A, field_start=True), kw(m, C)),
               AND(kw(m, A, field_end=True), kw(m, B)),
               AND(kw(m, B, field_end=True), kw(m, A)),
               AND(kw(m, A, field_max_pos=24), kw(m, B)),
               AND(kw(m, B, field_max_pos=1 << 21), kw(m, A)),
               AND(kw(m, A, some, field_end=True), kw(m, B)),
               AND(kw(m, B, some, field_max_pos=1 << 20), kw(m, A))]
    out["F"] = [q(r, rk) for r in f_roots for rk in (m.SPH_RANK_PROXIMITY_BM25, m.SPH_RANK_SPH04)]
    leaf = node(m.SPH_QUERY_OR, [node(m.SPH_QUERY_PHRASE, [kw(m, A), kw(m, B)]), kw(m, E)])
    out["S_bm25"] = [q(leaf, m.SPH_RANK_BM25)]
    out["S_prox"] = [q(leaf, m.SPH_RANK_PROXIMITY_BM25)]
    five = [kw(m, t) for t in (A, B, C, D, E)]
    out["G"] = [q(AND(*five), m.SPH_RANK_PROXIMITY_BM25), q(AND(*five), m.SPH_RANK_PROXIMITY),
                q(node(m.SPH_QUERY_PHRASE, five), m.SPH_RANK_PROXIMITY_BM25),
                q(AND(kw(m, A, some), kw(m, B), kw(m, C), kw(m, D), kw(m, E)), m.SPH_RANK_PROXIMITY_BM25)]
    return out


# --------------------------------------------------------------------------- the weight model (from the hit arrays, not the bytes)
def queried(mask, hit):
    return (mask >> (hit >> 24)) & 1 != 0


def keywords_of(root):
    """[(term, qpos, field limit)] of a flat AND / OR / PHRASE of keywords"""
    return [(c.word.term_id, c.word.atom_pos, c.field_mask) for c in root.children]


def doc_matches_all(doc, kws):
    return all(any(queried(mask, h) for h in doc.hits[t]) for t, _, mask in kws)


def stream(doc, kws):
    """the merged hit stream the ranker sees: ordered by the raw hit position (end flag included), then the query position; hits
    outside their keyword's field limit never arrive"""
    return sorted((h, qp) for t, qp, mask in kws for h in doc.hits[t] if queried(mask, h))


def proximity_weight(doc, kws, fw):
    """RankerState_Proximity_fn<.., false> (sphinxsearch.cpp:1351-1367, 1414-1437): LCS per field in BYTE arithmetic, times the weights"""
    lcs = [0] * 256
    cur, exp_delta, last = 0, -1, -1
    for h, qp in stream(doc, kws):
        pwf = h & ~END
        delta = pwf - qp
        if pwf > last:
            cur = ((cur if delta == exp_delta else 0) + 1) & 0xFF
        f = pwf >> 24
        if cur > lcs[f]:
            lcs[f] = cur
        last, exp_delta = pwf, delta
    return sum(lcs[f] * w for f, w in enumerate(fw))


def wordcount_weight(doc, kws, fw):
    return sum(fw[h >> 24] for h, _ in stream(doc, kws) if h >> 24 < len(fw))


def fieldmask_weight(doc, kws, fw):
    mask = 0
    for h, _ in stream(doc, kws):
        mask |= 1 << (h >> 24)
    return int(np.uint32(mask).astype(np.int32))


def phrase_docs(docs, a=T_A, b=T_B):
    """rowids of the docs that hold '"a b"': a hit of b one position behind a hit of a, in the same field"""
    out = []
    for r, d in enumerate(docs):
        pa = {h & ~END for h in d.hits[a]}
        if any((h & ~END) - 1 in pa and (h & POS_MASK) > 1 for h in d.hits[b]):
            out.append(r)
    return out


def ranked(docs, kws, weight_fn, fw, match_all=True):
    """-> (rowids, weights) by weight descending, rowid ascending, of the docs an AND (match_all) or an OR of kws holds"""
    rows = []
    for r, d in enumerate(docs):
        ok = doc_matches_all(d, kws) if match_all else any(queried(mask, h) for t, _, mask in kws for h in d.hits[t])
        if ok:
            rows.append((-weight_fn(d, kws, fw), r))
    rows.sort()
    return np.array([r for _, r in rows], np.uint32), np.array([-w for w, _ in rows], np.int32)
