"""CPU: grouped queries across segments and shards without a device.  (1) the new symbols and the group spec word; (2)
dist.merge_grows_np -- the numpy mirror of merge_grows_kernel -- against group_expect's model over the WHOLE match set, with every
shard's group row built by the test from the oracle's matches inside the shard's rowid range: three uneven shards, all six orders,
K in {1, 2, 4, 20}, the limit counted over all lists, staged merges; (3) the flags and the hostile rows in the mirror; (4) the merge
restated over GroupSeqOps and the kernels' row reader in a stand-alone program under ASan + UBSan (tests/cpp/group_merge.cpp); (5)
the same rows through the gloo exchange, all-gather and partitioned.  Every comparison is exact."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import group_expect as ge
import group_merge_common as gmc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"

N_DOCS, CUTS, PROBS = 6000, [0, 1500, 4001, 6000], [1.0, 0.6, 0.4, 0.3, 0.2]
GLOO_CUTS = [0, 2501, 6000]
ORDERS = [(by, desc) for by in (ge.GROUPSORT_KEY, ge.GROUPSORT_COUNT, ge.GROUPSORT_WEIGHT) for desc in (True, False)]


def test_symbols_and_spec_word():
    import re

    import manticoresearch_amd as m
    from manticoresearch_amd import _lib, dist

    assert m.GROW_GROUPS == _lib.GROW_GROUPS == dist.GROW_GROUPS == gmc.G == 4096
    assert m.GROW_WORDS == _lib.GROW_WORDS == dist.GROW_WORDS == gmc.WORDS == 8195 and hasattr(m.Batch, "export_grows")
    assert (dist.GROW_CNT, dist.GROW_TOTAL, dist.GROW_PLANE, dist.GROW_SPEC) == (gmc.CNT, gmc.TOTAL, gmc.PLANE, gmc.SPEC) == (4096, 4097, 4098, 8194)
    hdr = open(os.path.join(ROOT, "include", "mrk.h")).read()
    assert re.search(r"#define\s+MRK_GROW_GROUPS\s+\(4 \* MRK_MAX_K\)", hdr) and re.search(r"#define\s+MRK_GROW_WORDS\s+\(2 \* MRK_GROW_GROUPS \+ 3\)", hdr)
    for name in ("mrk_batch_export_grows", "mrk_topk_merge_grows", "mrk_topk_merge_grows_async", "mrk_topk_merge_grows_part", "mrk_shard_exchange_grows",
                 "mrk_group_spec_word"):
        assert hasattr(_lib.lib(), name) and name in hdr, name
    f = _lib.lib().mrk_group_spec_word
    for by in range(3):
        for desc in (0, 1):
            for bits in (1, 7, 32):
                for k in (1, 2, 20, 1024):
                    w = dist.group_spec_word(by, desc, bits, k)
                    assert w == f(by, desc, bits, k) == 1 | (by << 1) | (desc << 3) | (bits << 8) | (k << 16)
                    assert dist.group_spec_unpack(w) == (by, desc, bits, k)
    good = dist.group_spec_word(1, 1, 32, 20)
    for bad in (0, good & ~1, good | 16, good | (1 << 27), good | (1 << 63), dist.group_spec_word(3, 0, 32, 20), dist.group_spec_word(0, 0, 0, 20),
                dist.group_spec_word(0, 0, 33, 20), dist.group_spec_word(0, 0, 32, 0), dist.group_spec_word(0, 0, 32, 1025)):
        assert dist.group_spec_unpack(bad) is None, hex(bad)
    assert f(3, 0, 32, 20) == 0 and f(0, 2, 32, 20) == 0 and f(0, 0, 33, 20) == 0 and f(0, 0, 32, 1025) == 0 and f(0, 0, 32, 0) == 0


class _Corpus:
    def __init__(self, orc):
        import manticoresearch_amd as m
        from test_gpu_group import make_rows
        from test_gpu_parity import orc_index_of

        self.m = m
        self.hi = m.synth_index(N_DOCS, PROBS, seed=61, n_fields=4, max_pos=6)
        self.rows = make_rows(N_DOCS)
        self.oi = orc_index_of(orc, self.hi)
        self.oi.attrs = self.rows
        self.cache = {}

    def matches(self, orc, q):
        key = (repr(q.root), q.ranker, q.group.bit_offset, q.group.bit_count)
        if key not in self.cache:
            self.cache[key] = gmc.whole_matches(orc, self.oi, q, self.rows, N_DOCS)
        return self.cache[key]


@pytest.fixture(scope="module")
def corpus(orc):
    return _Corpus(orc)


def _cases(m):
    """(query, must the model answer) -- the limit on both sides at every K"""
    from test_gpu_group import BITS, C2, C16, C17, C64, C65, S1C, S2C, Q

    out = []
    for by, desc in ORDERS:
        for sh in ("one", "and2", "none"):
            out += [(Q(m, sh, S1C, K=1, by=by, desc=desc), True), (Q(m, sh, C2, K=1, by=by, desc=desc), True), (Q(m, sh, S2C, K=1, by=by, desc=desc), False),
                    (Q(m, sh, S2C, K=2, by=by, desc=desc), True), (Q(m, sh, C16, K=2, by=by, desc=desc), False),
                    (Q(m, sh, C16, K=4, by=by, desc=desc), True), (Q(m, sh, C17, K=4, by=by, desc=desc), False),
                    (Q(m, sh, C64, K=20, by=by, desc=desc), True), (Q(m, sh, C65, K=20, by=by, desc=desc), True),
                    (Q(m, sh, BITS, bits=7, shift=9, K=20, by=by, desc=desc), False)]
    return out


def test_merge_np_equals_the_model_over_the_whole_match_set(orc, corpus):
    from manticoresearch_amd import dist

    cases = _cases(corpus.m)
    n_decl = 0
    for i, (q, must) in enumerate(cases):
        mt = corpus.matches(orc, q)
        rows = gmc.shard_rows_np(q, mt, CUTS)[:, None, :]
        merged = dist.merge_grows_np(rows, 1024)
        n_decl += gmc.check_merged(dist, q, mt, merged[0], ("three shards", i), must)
        assert np.array_equal(gmc.staged(dist, rows, 1024), merged), ("staged", i)
        assert np.array_equal(dist.merge_grows_np(rows[::-1], 1024), merged), ("the lists' order", i)
        assert np.array_equal(dist.merge_grows_np(rows, q.max_matches), merged), ("k = the query's own", i)
        one = gmc.shard_rows_np(q, mt, [0, N_DOCS])[:, None, :]
        assert np.array_equal(dist.merge_grows_np(one, 1024), one[0]) and np.array_equal(merged, one[0]), ("one list: the row itself", i)
    assert n_decl == sum(not must for _, must in cases) == 72


def _disjoint(m, K, per_shard, n_docs=N_DOCS, cuts=CUTS):
    """(query, rows, matches): term 0 matches every doc; the group column holds per_shard[s] values nobody else has in shard s"""
    from test_gpu_group import C64, STRIDE, Q, scr

    rows = np.zeros((n_docs, STRIDE), np.uint32)
    r = np.arange(n_docs, dtype=np.uint64)
    for s, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        rows[lo:hi, C64] = scr((s * 100000 + r[lo:hi] % per_shard[s]))
    return Q(m, "none", C64, K=K, by=ge.GROUPSORT_COUNT), rows


def test_the_limit_is_counted_over_all_lists(orc, corpus):
    """shard-disjoint values: 6 + 5 + 5 = 16 = 4 K answer, 6 + 6 + 5 = 17 decline although every list alone is inside its limit; the
    16- and 32-slot tables of K = 1 and K = 2 at limits 4 and 8; staged, the decline falls at the last step"""
    from manticoresearch_amd import dist

    for K, per, must in ((4, (6, 5, 5), True), (4, (6, 6, 5), False), (1, (2, 1, 1), True), (1, (2, 2, 1), False), (2, (3, 3, 2), True), (2, (3, 3, 3), False)):
        q, rows = _disjoint(corpus.m, K, per)
        full = gmc.all_matches(orc, corpus.oi, corpus.m.Query(q.root, ranker=q.ranker, max_matches=q.max_matches), N_DOCS)
        mt = (full.rowid, full.weight, rows[full.rowid, q.group.bit_offset >> 5])
        assert len(full.rowid) == N_DOCS
        lists = gmc.shard_rows_np(q, mt, CUTS)[:, None, :]
        assert [int(x) for x in lists[:, 0, gmc.TOTAL]] == list(per), "every list alone is inside its limit"
        merged = dist.merge_grows_np(lists, 1024)
        assert gmc.check_merged(dist, q, mt, merged[0], ("disjoint", K, per), must) == (not must)
        ab = dist.merge_grows_np(lists[:2], 1024)
        assert int(ab[0, gmc.TOTAL]) == per[0] + per[1], "the first step answers"
        assert np.array_equal(dist.merge_grows_np(np.stack([ab, lists[2]]), 1024), merged), ("staged", K, per)


def test_flags_and_hostile_rows_in_the_mirror(orc, corpus):
    from manticoresearch_amd import dist
    from test_gpu_group import C16, Q

    m = corpus.m
    q = Q(m, "and2", C16, K=10, by=ge.GROUPSORT_WEIGHT, desc=False)
    mt = corpus.matches(orc, q)
    base = gmc.shard_rows_np(q, mt, CUTS)[:, None, :]
    spec, R, D = gmc.spec_of(q), gmc.RERUN, gmc.DECLINED

    def empty(row, flags, sp=spec):
        return int(row[gmc.TOTAL]) == flags and int(row[gmc.CNT]) == 0 and int(row[gmc.SPEC]) == sp and not row[:gmc.G].any() and not row[gmc.PLANE:gmc.SPEC].any()

    def with_list(l, f):
        rows = base.copy()
        f(rows[l, 0])
        return dist.merge_grows_np(rows, 1024)[0]

    def rerun(row):
        row[:gmc.CNT + 1], row[gmc.PLANE:gmc.SPEC], row[gmc.TOTAL] = 0, 0, R

    def planner_declined(row):
        row[:], row[gmc.TOTAL] = 0, D

    def too_many(row):
        row[gmc.CNT] = gmc.G + 1

    def bad_spec(row):
        row[gmc.SPEC] = spec | (1 << 40)

    for fault, flags in ((rerun, R), (planner_declined, D), (too_many, D), (bad_spec, D)):
        got = [with_list(l, fault) for l in range(3)]
        assert empty(got[0], flags) and np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), fault.__name__
    both = base.copy()
    rerun(both[0, 0]), planner_declined(both[2, 0])
    assert empty(dist.merge_grows_np(both, 1024)[0], R | D)
    for other in (dist.group_spec_word(ge.GROUPSORT_COUNT, 0, 32, 10), dist.group_spec_word(ge.GROUPSORT_WEIGHT, 1, 32, 10), dist.group_spec_word(ge.GROUPSORT_WEIGHT, 0, 32, 11)):
        rows = base.copy()
        rows[1, 0, gmc.SPEC] = other
        assert empty(dist.merge_grows_np(rows, 1024)[0], D) and empty(dist.merge_grows_np(rows[[1, 0, 2]], 1024)[0], D, other)
    rel = gmc.grow_of_relevance(np.array([5, 9]), np.array([7, 7]), 2)
    rows = base.copy()
    rows[2, 0] = rel
    assert empty(dist.merge_grows_np(rows, 1024)[0], D)
    got = dist.merge_grows_np(rows[::-1], 1024)[0]  # the relevance row first: its spec, and the narrow merge's sum of totals under the flag
    assert int(got[gmc.TOTAL]) == D | int(rows[:, 0, gmc.TOTAL].sum()) and int(got[gmc.CNT]) == 0 and int(got[gmc.SPEC]) == 0 and not got[:gmc.G].any() and not got[gmc.PLANE:].any()
    assert empty(dist.merge_grows_np(base, 9)[0], D), "max_matches above the call's k"
    # counts: 2^32 - 1 is a count, 2^32 declines
    rows = base.copy()
    v = int(rows[0, 0, gmc.PLANE]) >> 32
    others = sum(int(rows[l, 0, gmc.PLANE + i]) & 0xFFFFFFFF for l in (1, 2) for i in range(int(rows[l, 0, gmc.CNT])) if int(rows[l, 0, gmc.PLANE + i]) >> 32 == v)
    rows[0, 0, gmc.PLANE] = (v << 32) | (0xFFFFFFFF - others)
    got = dist.merge_grows_np(rows, 1024)[0]
    assert not int(got[gmc.TOTAL]) & (R | D) and ((v << 32) | 0xFFFFFFFF) in [int(x) for x in got[gmc.PLANE:gmc.PLANE + int(got[gmc.CNT])]]
    if others:
        rows[0, 0, gmc.PLANE] = (v << 32) | 0xFFFFFFFF
        assert empty(dist.merge_grows_np(rows, 1024)[0], D)


def _merge_rows_np(rows_all, k):
    """The narrow merge in numpy: (weight, docid) = the u64 key descending; totals add up, flags OR through."""
    n_lists, nq, _ = rows_all.shape
    out = np.zeros((nq, 1026), np.uint64)
    mask = np.uint64((1 << 63) | (1 << 62))
    for q in range(nq):
        keys = np.concatenate([rows_all[l, q, :int(rows_all[l, q, 1024])] for l in range(n_lists)])
        keys = np.sort(keys)[::-1][:k]
        out[q, :len(keys)] = keys
        out[q, 1024] = len(keys)
        tf = rows_all[:, q, 1025]
        out[q, 1025] = np.uint64(int((tf & ~mask).sum(dtype=np.uint64)) | int(np.bitwise_or.reduce(tf & mask)))
    return out


def test_relevance_rows_merge_as_the_narrow_rows_do():
    from manticoresearch_amd import dist

    rng = np.random.default_rng(8)
    lists = []
    for s in range(5):
        n = [0, 3, 1024, 700, 1024][s]
        keys = np.sort(gmc.make_keys(rng.integers(1, 50, n), rng.choice(100000, n, replace=False) + s * 100000))[::-1]
        row = np.zeros(gmc.WORDS, np.uint64)
        row[:n], row[gmc.CNT], row[gmc.TOTAL] = keys, n, n + 17
        lists.append(row)
    rows = np.stack(lists)[:, None, :]
    rows[1, 0, gmc.TOTAL] |= np.uint64(gmc.RERUN)
    for k in (1, 10, 1024):
        got = dist.merge_grows_np(rows, k)[0]
        narrow = _merge_rows_np(np.ascontiguousarray(np.concatenate([rows[:, :, :1024], rows[:, :, gmc.CNT:gmc.TOTAL + 1]], axis=2)), k)[0]
        assert np.array_equal(got[:1024], narrow[:1024]) and got[gmc.CNT] == narrow[1024] and got[gmc.TOTAL] == narrow[1025]
        assert not got[1024:gmc.CNT].any() and not got[gmc.PLANE:].any()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc builds the host-only program")
def test_merge_restated_over_the_shared_functions_under_sanitizers(tmp_path):
    exe = str(tmp_path / "group_merge")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "cpp", "group_merge.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.startswith("ok group merge "), out.stdout


# ---------------------------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_queries(m):
    return [q for q, _ in _cases(m)][::7]


def _worker(rank, world, port, queue):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    import torch.distributed as tdist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    from manticoresearch_amd import dist as mdist
    from oracle import oracle as orc

    corpus = _Corpus(orc)
    qs = _gloo_queries(corpus.m)
    mine = np.stack([gmc.shard_rows_np(q, corpus.matches(orc, q), GLOO_CUTS)[rank] for q in qs])
    rows = torch.from_numpy(mine.view(np.int64))
    rows_all = mdist.exchange_rows(rows)
    assert rows_all.shape == (world, len(qs), mdist.GROW_WORDS) and torch.equal(rows_all[rank], rows)
    merged = mdist.merge_grows_np(rows_all.numpy().view(np.uint64), 1024)
    recv, first, count = mdist.exchange_rows_partitioned(rows)
    per = (len(qs) + world - 1) // world
    assert recv.shape == (world, per, mdist.GROW_WORDS) and torch.equal(recv[:, :count], rows_all[:, first:first + count])
    part = mdist.merge_grows_np(recv.numpy().view(np.uint64)[:, :count], 1024)
    queue.put((rank, merged, first, count, part))
    tdist.barrier()
    tdist.destroy_process_group()


def test_group_rows_over_gloo(orc, corpus):
    import torch.multiprocessing as mp
    from manticoresearch_amd import dist

    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, queue)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([queue.get(timeout=900) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    qs = _gloo_queries(corpus.m)
    assert len(qs) >= 20
    assert np.array_equal(got[0][1], got[1][1])  # every rank of the all-gather form merges the same rows
    n_decl = sum(gmc.check_merged(dist, q, corpus.matches(orc, q), got[0][1][i], ("gloo", i)) for i, q in enumerate(qs))
    assert 0 < n_decl < len(qs)
    together = np.concatenate([g[4] for g in got])  # the partitioned slices, rank after rank
    assert [g[2] for g in got] == [0, got[0][3]] and got[0][3] + got[1][3] == len(qs)
    assert np.array_equal(together, got[0][1])
