"""Corpora and a numpy model for the suite of the tree kernel over bitmap words (scan_bt_kernel, csrc/mrk_scan_bt.hip): shared by
test_bt_edges_cpu.py (the structure claimed here, oracle == model) and test_gpu_bt_edges.py (device == oracle, on and off the kernel).

Corpus A sits on the kernel's own edges.  N = 2 * 131072 + 5 * 2048 + 1 docs are 134 windows of 2048 rowids, the last one of a
single doc.  A tree-kernel work item is never shorter than 64 windows (layout_batch), so a pass is cut into [0, 64) [64, 128)
[128, 134): two items whose four waves walk 16 windows = 4 whole steps of 8192 rowids each, and a ragged one -- 2 windows per wave for
waves 0-2, none for wave 3, a window count that is no multiple of the 4-window step (load_step's `inr` clause), wave starts that are
no multiple of 4 (rank seeds off the step grid).  The keywords (ids below) put docs on steps' first and last rowids, blocks on
steps' ends, 31 blocks of one keyword into one step, a full step of 8192 docs into two keywords at once, tf >= 255 into a dense and
a sparse keyword, and a phrase pair whose candidates the lone-hit shortcut accepts, rejects and must hand on.

The model: a boolean tree's match set is set algebra over the keywords' rowid arrays (AND = intersection, OR = union, ANDNOT =
difference, MAYBE = its left side), dead rows removed; under SPH_RANK_NONE the answer is the K lowest rowids, weight index_weight.
It knows nothing of oracle/."""
import numpy as np

STEP = 8192   # rowids per step of the kernel (BT_SPAN = 4 windows)
WINDOW = 2048
N_DOCS = 2 * 131072 + 5 * 2048 + 1
N_WINDOWS = (N_DOCS + WINDOW - 1) // WINDOW
ITEM_WINDOWS = 64  # layout_batch: max(wpi, 4 * unit), unit = 4 windows x 4 waves; wpi is 0 for batches this small
DENSE_MIN = (N_DOCS + 63) // 64  # docs * 64 >= total docs: the keyword gets a doc-set bitmap
N_TERMS = 10
FULL_STEP = 3  # keywords 1 and 2 hold every rowid of this step
EDGE_ROWIDS = [0, 31, 32, 63, 64, 127, 128, 2047, 2048, STEP - 1, STEP, 131071, 131072, 262143, 262144, N_DOCS - 2, N_DOCS - 1]
FAT_EVERY = 997  # every 997th doc of keywords 1 and 3 holds 300 hits: the tf byte saturates (the 255-tf escape)
# the phrase pair (keywords 8 and 9): docs that hold both, by what the hit lists say about '"8 9"'
PH_ACCEPT = 3000      # tf 1 each, 9 right behind 8 in one field: the lone-hit shortcut accepts
PH_REJECT_FIELD = 500  # tf 1 each, 9 at position(8) + 1 of ANOTHER field: it rejects
PH_REJECT_GAP = 500    # tf 1 each, one field, 9 two positions behind 8: it rejects
PH_REVERSED = 500      # tf 1 each, one field, 9 right BEFORE 8: it rejects '"8 9"' and accepts '"9 8"'
PH_MULTI_WITH = 750    # tf 2-4 each, with an occurrence of '8 9': the hit pass decides
PH_MULTI_WITHOUT = 750  # tf 2-4 each, without one
PH_COMMON = PH_ACCEPT + PH_REJECT_FIELD + PH_REJECT_GAP + PH_REVERSED + PH_MULTI_WITH + PH_MULTI_WITHOUT
PH_ONLY = 8000  # docs that hold only one of the two


def item_ranges(n_windows=N_WINDOWS, per=ITEM_WINDOWS):
    """The window ranges a pass of the tree kernel is cut into, and per range the four waves' (first window, last window + 1)."""
    out = []
    for b in range(0, n_windows, per):
        e = min(b + per, n_windows)
        share = (e - b + 3) // 4
        out.append(((b, e), [(min(b + w * share, e), min(b + (w + 1) * share, e)) for w in range(4)]))
    return out


def _random_hits(rng, t, rows):
    """tf = 1 + min(254, geometric) random hits per doc over 3 fields x 40 positions (duplicates fall out later)"""
    tf = 1 + np.minimum(254, rng.geometric(0.5, rows.size) - 1)
    n = int(tf.sum())
    return (np.full(n, t + 1, np.uint64), np.repeat(rows, tf).astype(np.uint32),
            ((rng.integers(0, 3, n).astype(np.uint32)) << 24) | rng.integers(1, 41, n).astype(np.uint32))


def _fat_hits(t, rows):
    """300 hits in field 1"""
    return (np.full(rows.size * 300, t + 1, np.uint64), np.repeat(rows, 300).astype(np.uint32),
            np.tile((np.uint32(1) << 24) | np.arange(1, 301, dtype=np.uint32), rows.size))


def corpus_a_rows(seed=7):
    """The ten keywords' rowid arrays (sorted, unique) and the classes of the phrase pair's common docs."""
    rng = np.random.default_rng(seed)
    everything = np.arange(N_DOCS, dtype=np.uint32)
    full = np.arange(FULL_STEP * STEP, (FULL_STEP + 1) * STEP, dtype=np.uint32)

    def pick(p):
        return everything[rng.random(N_DOCS) < p]

    # (the dense keywords 0 and 1 hold the sparse ones' edge docs, so that those docs decide matches and weights, not only bits)
    seam = [17 * STEP - 1, 17 * STEP]
    rows = [np.union1d(pick(0.30), EDGE_ROWIDS + seam),
            np.union1d(np.union1d(pick(0.10), full), [N_DOCS - 1] + seam),
            np.union1d(np.union1d(pick(0.05), full), [N_DOCS - 1]),
            np.union1d(rng.choice(N_DOCS, 1500, replace=False), EDGE_ROWIDS),
            np.arange(5 * STEP + 100, 5 * STEP + 4100),
            np.arange(17 * STEP - 128, 17 * STEP + 128),
            np.array([N_DOCS - 1]),
            np.zeros(0)]
    # the phrase pair: disjoint draws for the classes of common docs and for the docs of one keyword alone
    perm = rng.permutation(N_DOCS).astype(np.uint32)
    sizes = [PH_ACCEPT, PH_REJECT_FIELD, PH_REJECT_GAP, PH_REVERSED, PH_MULTI_WITH, PH_MULTI_WITHOUT, PH_ONLY, PH_ONLY]
    cuts = np.cumsum([0] + sizes)
    parts = [np.sort(perm[cuts[i]:cuts[i + 1]]) for i in range(len(sizes))]
    classes = dict(zip(["accept", "reject_field", "reject_gap", "reversed", "multi_with", "multi_without", "only8", "only9"], parts))
    common = np.sort(np.concatenate(parts[:6]))
    rows.append(np.union1d(common, parts[6]))
    rows.append(np.union1d(common, parts[7]))
    return [np.asarray(r, np.uint32) for r in rows], classes


def _phrase_hits(rng, classes):
    """Hits of keywords 8 and 9 in their common docs, class by class (field << 24 | position)."""
    W, R, H = [], [], []

    def put(t, rows, hits):
        W.append(np.full(rows.size, t + 1, np.uint64)), R.append(rows.astype(np.uint32)), H.append(hits.astype(np.uint32))

    def lone(rows, dfield, dpos):
        f = rng.integers(0, 3, rows.size).astype(np.uint32)
        p = rng.integers(2, 30, rows.size)
        put(8, rows, (f << 24) | p.astype(np.uint32))
        put(9, rows, (((f + dfield) % 3) << 24) | (p + dpos).astype(np.uint32))

    lone(classes["accept"], 0, 1)
    lone(classes["reject_field"], 1, 1)
    lone(classes["reject_gap"], 0, 2)
    lone(classes["reversed"], 0, -1)
    # tf 2-4 each: 8 at p + 10 i, 9 at p + d + 20 j with d = 1 (an occurrence at i = j = 0) or 3 (9 never right behind 8, 8 never right behind 9)
    for name, d in (("multi_with", 1), ("multi_without", 3)):
        rows = classes[name]
        f = rng.integers(0, 3, rows.size).astype(np.uint32)
        p = rng.integers(1, 20, rows.size).astype(np.uint32)
        for t, stride, off in ((8, 10, 0), (9, 20, d)):
            tf = rng.integers(2, 5, rows.size)
            for i in range(4):
                sel = tf > i
                put(t, rows[sel], (f[sel] << 24) | (p[sel] + off + stride * i))
    return W, R, H


def corpus_a_hits(seed=7):
    """(wordid, rowid, hitpos) sorted and unique, the keywords' rowid arrays, the phrase classes."""
    rows, classes = corpus_a_rows(seed)
    rng = np.random.default_rng(seed + 1)
    W, R, H = [], [], []
    for t in range(8):
        rw = rows[t]
        if t in (1, 3):
            fat = rw[::FAT_EVERY]
            w, r, h = _fat_hits(t, fat)
            W.append(w), R.append(r), H.append(h)
            rw = np.setdiff1d(rw, fat)
        if rw.size:
            w, r, h = _random_hits(rng, t, rw)
            W.append(w), R.append(r), H.append(h)
    for t, name in ((8, "only8"), (9, "only9")):
        w, r, h = _random_hits(rng, t, classes[name])
        W.append(w), R.append(r), H.append(h)
    w, r, h = _phrase_hits(rng, classes)
    W, R, H = np.concatenate(W + w), np.concatenate(R + r), np.concatenate(H + h)
    o = np.lexsort((H, R, W))
    W, R, H = W[o], R[o], H[o]
    keep = np.ones(W.size, bool)
    keep[1:] = (W[1:] != W[:-1]) | (R[1:] != R[:-1]) | (H[1:] != H[:-1])
    return W[keep], R[keep], H[keep], rows, classes


def corpus_a(m, block=128, fmt=1, seed=7):
    W, R, H, rows, classes = corpus_a_hits(seed)
    hi = m.index_from_hits(W, R, H, n_terms=N_TERMS, total_docs=N_DOCS, skiplist_block_size=block, hit_format=fmt, n_fields=3)
    docs = [int(x) for x in hi.dict["docs"]]
    assert docs == [r.size for r in rows], (docs, [r.size for r in rows])
    assert all(docs[t] >= DENSE_MIN for t in (0, 1, 2, 8, 9)) and all(docs[t] < N_DOCS // 64 for t in (3, 4, 5, 6, 7)), docs
    return hi, rows, classes


# ---- corpus B: ties for the second level of the pruning in front of the hit pass
B_DOCS = 40001
B_AC, B_BC, B_NOISE = 18000, 800, 12000


def corpus_b(m, seed=11):
    """Three keywords over two fields, tf 1-2, positions 1-16, built so that thousands of matches share the K-th weight AND the
    weight bounds in front of the hit pass (prox_bounds) are exact for them -- only then does the pruning threshold reach the
    K-th weight itself, the place where its second level decides by rowid slice:
      AC     18000 docs: a once in field 0, c once in field 1.  One hit per field: lower bound = upper bound = weight.
      BC       800 docs: b once in field 0, c once in field 1.  b is the rarer keyword, so under BM25 these lie above AC.
      noise  12000 docs: each keyword with probability 0.7, tf 1-2, every hit in field 0, a behind b behind c: no run is longer
             than one hit, so these weigh less than AC and BC whatever their tf, while their upper bounds (up to six hits in the
             field) lie far above: the loose population the hit pass has to look at.
    K = 10 falls into BC (or AC + BC without BM25), K = 1000 into AC.  The field-end flag sits on every hit at a field's last
    position, whatever the word: what the reference's indexer writes, and what prox_bound_keywords = 1 asks for."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(B_DOCS).astype(np.uint32)
    ac, bc, noise = np.sort(perm[:B_AC]), np.sort(perm[B_AC:B_AC + B_BC]), np.sort(perm[B_AC + B_BC:B_AC + B_BC + B_NOISE])
    W, R, H = [], [], []

    def put(t, rw, field, pos):
        W.append(np.full(rw.size, t + 1, np.uint64)), R.append(rw.astype(np.uint32)), H.append((np.uint32(field) << 24) | pos.astype(np.uint32))

    put(0, ac, 0, rng.integers(1, 17, ac.size)), put(2, ac, 1, rng.integers(1, 17, ac.size))
    put(1, bc, 0, rng.integers(1, 17, bc.size)), put(2, bc, 1, rng.integers(1, 17, bc.size))
    for t, first in ((0, 11), (1, 6), (2, 1)):  # positions 11-16, 6-10, 1-5: query order runs against the positions
        rw = noise[rng.random(noise.size) < 0.7]
        for i in range(2):
            sel = rw if i == 0 else rw[rng.random(rw.size) < 0.5]
            put(t, sel, 0, rng.integers(first, first + 5, sel.size))
    W, R, H = np.concatenate(W), np.concatenate(R), np.concatenate(H)
    # the last position of each (doc, field) carries the flag
    key = (R.astype(np.int64) * 2 + (H >> 24)).astype(np.int64)
    last = np.zeros(2 * B_DOCS, np.uint32)
    np.maximum.at(last, key, H & 0xFFFF)
    H = H | (((H & 0xFFFF) == last[key]).astype(np.uint32) << 23)
    o = np.lexsort((H, R, W))
    W, R, H = W[o], R[o], H[o]
    keep = np.ones(W.size, bool)
    keep[1:] = (W[1:] != W[:-1]) | (R[1:] != R[:-1]) | (H[1:] != H[:-1])
    W, R, H = W[keep], R[keep], H[keep]
    hi = m.index_from_hits(W, R, H, n_terms=3, total_docs=B_DOCS, n_fields=2)
    return hi, [np.unique(R[W == t + 1]) for t in range(3)]


# ---- corpus C: every doc holds three keywords with one weight -- nothing prunes under BM25, the candidate list overflows
C_DOCS = 1_300_000


def corpus_c(m):
    rows = np.arange(C_DOCS, dtype=np.uint32)
    W = np.concatenate([np.full(C_DOCS, t + 1, np.uint64) for t in range(3)])
    R = np.concatenate([rows] * 3)
    H = np.concatenate([np.full(C_DOCS, (1 << 24) | (t + 1), np.uint32) for t in range(3)])
    return m.index_from_hits(W, R, H, n_terms=3, total_docs=C_DOCS, n_fields=2), [rows, rows, rows]


# ---- trees
def kw(m, t, pos):
    return m.XQNode.keyword(t, pos)


def AND(m, *k):
    return m.XQNode.AND(*k)


def OR(m, *k):
    return m.XQNode(m.SPH_QUERY_OR, list(k))


def MAYBE(m, l, r):
    return m.XQNode(m.SPH_QUERY_MAYBE, [l, r])


def ANDNOT(m, l, r):
    return m.XQNode(m.SPH_QUERY_ANDNOT, [l, r])


def PHRASE(m, *k):
    return m.XQNode(m.SPH_QUERY_PHRASE, list(k), None, 0xFFFFFFFF)


def PROXIMITY(m, dist, *k):
    return m.XQNode(m.SPH_QUERY_PROXIMITY, list(k), None, 0xFFFFFFFF, dist)


def named_trees(m):
    """The suite's list over corpus A, a..g = keywords 0..6, atom positions in traversal order."""
    def K(*ts):
        return [kw(m, t, i + 1) for i, t in enumerate(ts)]

    def or_ab_and(x):  # '(a|b) x'
        a, b, x = K(0, 1, x)
        return AND(m, OR(m, a, b), x)

    c, a, b = K(2, 0, 1)
    c_ab = AND(m, c, OR(m, a, b))
    a, d, b, e = K(0, 3, 1, 4)
    ad_be = AND(m, OR(m, a, d), OR(m, b, e))
    a, b, c = K(0, 1, 2)
    ab_not_c = ANDNOT(m, OR(m, a, b), c)
    a, a2, b = K(0, 0, 1)
    dupes = OR(m, a, AND(m, a2, b))
    return [("(a|b) c", or_ab_and(2)), ("c (a|b)", c_ab), ("a|b|c|d", OR(m, *K(0, 1, 2, 3))), ("(a|d)(b|e)", ad_be), ("a -d", ANDNOT(m, *K(0, 3))),
            ("(a|b) -c", ab_not_c), ("b MAYBE f", MAYBE(m, *K(1, 5))), ("f MAYBE b", MAYBE(m, *K(5, 1))), ("a b c", AND(m, *K(0, 1, 2))),
            ("b|g", OR(m, *K(1, 6))), ("b | <7>", OR(m, *K(1, 7))), ("b -<7>", ANDNOT(m, *K(1, 7))),
            ("(a|b) d", or_ab_and(3)), ("(a|b) e", or_ab_and(4)), ("(a|b) f", or_ab_and(5)), ("a | (a b)", dupes),
            ("<0>", kw(m, 0, 1)), ("<1>", kw(m, 1, 1)), ("<2>", kw(m, 2, 1))]


def full_step_trees(m):
    def K(*ts):
        return [kw(m, t, i + 1) for i, t in enumerate(ts)]

    b, c, a = K(1, 2, 0)
    return [("b c", AND(m, *K(1, 2))), ("b|c", OR(m, *K(1, 2))), ("(b|c) a", AND(m, OR(m, b, c), a)), ("b -c", ANDNOT(m, *K(1, 2)))]


def leaves(m, node):
    if node.word is not None:
        return [node]
    return [x for c in node.children for x in leaves(m, c)]


def unrestricted(m, node):
    return all(x.field_mask == 0xFFFFFFFF for x in leaves(m, node))


def random_trees(m, n, seed=20261019, n_terms=N_TERMS):
    """n trees of test_gpu_parity._random_tree whose keywords are all unrestricted in fields and at most four."""
    from test_gpu_parity import _random_tree

    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        root = _random_tree(m, rng, n_terms)
        if unrestricted(m, root) and len(leaves(m, root)) <= 4:
            out.append(root)
    return out


# ---- the model
def match_mask(m, node, rows, n_docs):
    if node.word is not None:
        mask = np.zeros(n_docs, bool)
        mask[rows[node.word.term_id]] = True
        return mask
    kids = [match_mask(m, c, rows, n_docs) for c in node.children]
    if node.op == m.SPH_QUERY_AND:
        return np.logical_and.reduce(kids)
    if node.op == m.SPH_QUERY_OR:
        return np.logical_or.reduce(kids)
    if node.op == m.SPH_QUERY_MAYBE:
        return kids[0]
    if node.op == m.SPH_QUERY_ANDNOT:
        return kids[0] & ~kids[1]
    raise ValueError("the model knows boolean trees only: op %d" % node.op)


def dead_mask(dead, n_docs):
    if dead is None:
        return np.zeros(n_docs, bool)
    return np.unpackbits(np.ascontiguousarray(dead, np.uint32).view(np.uint8), bitorder="little")[:n_docs].astype(bool)


def dead_words(n_docs, killed):
    dead = np.zeros((n_docs + 31) // 32, np.uint32)
    killed = np.asarray(killed, np.int64)
    np.bitwise_or.at(dead, killed >> 5, (np.uint32(1) << (killed & 31).astype(np.uint32)))
    return dead


def model(m, q, rows, n_docs, dead=None):
    """(total_found, rowids, weights) of a boolean tree under SPH_RANK_NONE; for every other ranker the first is what holds."""
    mask = match_mask(m, q.root, rows, n_docs) & ~dead_mask(dead, n_docs)
    hits = np.nonzero(mask)[0].astype(np.uint32)
    top = hits[:q.max_matches]
    return int(hits.size), top, np.full(top.size, q.index_weight, np.int32)


# ---- which queries the planner sends to the tree kernel (mrk_plan.cpp: tree_on_bitmaps, phrase_on_bitmaps), restated for the shapes
# of this suite: what n_items_bt must count.  The device tests assert the count exactly, so a planner that moves its bar shows.
def _cover(m, node, docs):
    if node.word is not None:
        return [node.word.term_id]
    if node.op == m.SPH_QUERY_OR:
        return [t for c in node.children for t in _cover(m, c, docs)]
    if node.op == m.SPH_QUERY_AND:
        best = None
        for c in node.children:  # the side with the fewest docs, the first one on a tie
            cv = _cover(m, c, docs)
            if best is None or sum(docs[t] for t in cv) < sum(docs[t] for t in best):
                best = cv
        return best
    return _cover(m, node.children[0], docs)  # MAYBE, ANDNOT: the left side carries the docs


def _required(m, node):
    if node.word is not None:
        return {node.word.term_id}
    sets = [_required(m, c) for c in node.children]
    if node.op == m.SPH_QUERY_AND:
        return set().union(*sets)
    if node.op == m.SPH_QUERY_OR:
        return set.intersection(*sets)
    return sets[0]


def _ops(m, node):
    return set() if node.word is not None else {node.op}.union(*[_ops(m, c) for c in node.children])


def on_tree_kernel(m, q, docs, n_docs, cover_inv=1024):
    """True where the default planner evaluates the query's one pass on bitmap words."""
    root = q.root
    lv = leaves(m, root)
    terms = [x.word.term_id for x in lv]
    dense_min = (n_docs + 63) // 64
    if len(terms) > 4 or not unrestricted(m, root) or not any(docs[t] >= dense_min for t in terms):
        return False
    if any(docs[t] == 0 for t in _required(m, root) if root.op not in (m.SPH_QUERY_PHRASE, m.SPH_QUERY_PROXIMITY)):
        return False  # a required keyword without postings: no work item at all
    ops = _ops(m, root)
    if root.op in (m.SPH_QUERY_PHRASE, m.SPH_QUERY_PROXIMITY):  # a root phrase of common words: its candidates
        return len(set(terms)) == len(terms) >= 2 and all(docs[t] > 0 for t in terms) and min(docs[t] for t in terms) * cover_inv >= n_docs
    if ops & {m.SPH_QUERY_PHRASE, m.SPH_QUERY_PROXIMITY}:
        return False  # a phrase below the root is the block scan's
    pure_and = ops <= {m.SPH_QUERY_AND}
    if pure_and and len(terms) == 2 and q.ranker in (m.SPH_RANK_NONE, m.SPH_RANK_BM25) and all(docs[t] >= dense_min for t in terms):
        return False  # the two-bitmap AND kernel's
    cover_docs = sum(docs[t] for t in _cover(m, root, docs))
    return cover_docs * (min(cover_inv, 32) if pure_and else cover_inv) >= n_docs
