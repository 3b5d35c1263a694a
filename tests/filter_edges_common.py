"""A plain model of the reference's filters, one crafted corpus and one list of crafted cases for the filter edge suite
(test_filter_edges_cpu.py, test_gpu_filter_edges.py).

The model restates the reference, not oracle/cpu_ref.c and not csrc/mrk_dev.h, in Python integers (nothing overflows silently):

    sphGetRowAttr                        sphinx.h:993-1014        get_row_attr
    GetBlobAttr / CalcBlobRowFlags       attribute.cpp:28-37, 495-513   blob_attr
    EvalRange                            sphinxfilter.h:130-143   eval_range
    MvaEval_Any / _All / _RangeAny / _RangeAll   sphinxfilter.h:160-253   mva_any / mva_all / mva_range_any / mva_range_all
    IFilter_Values::EvalValues           sphinxfilter.cpp:69-91   eval_values
    Filter_FloatRange::Eval              sphinxfilter.cpp:286-289 (numpy.float32 comparisons)
    FilterNot (m_bExclude), Filter_And   row_passes
    Filter_WeightValues / _WeightRange   sphinxfilter.cpp:304-320 weight_passes

The restatement is literal where the reference is odd: MvaEval_Any carries L from one filter value to the next, MvaEval_RangeAny
answers "found the minimum, bound is strict, a next value exists" with true WITHOUT testing that value against the maximum, and
MvaEval_RangeAll casts its bounds to the MVA's type ((T)m_iMinValue: -1 becomes 2^32 - 1 for a 32-bit MVA, 2^32 + 5 becomes 5).

The corpus: N_DOCS = 3 full 128-doc device blocks and a partial one.  Keyword A is in every doc (every row reaches the filter), B..F in
every 2nd .. 6th.  The attribute rows cycle through their patterns with odd periods (5, 7, 9, 11, 13, 17: coprime to 64), so every pattern
sits in both rows of a lane (doc slot < 64 and >= 64 of a block) and in every block; the blob rows of the size-class edges stand on the
block edges and on the last rowid (SIZED_ROWS).  An 8-field and a 32-field twin share rows, pool and cases."""
import functools

import numpy as np

N_DOCS = 3 * 128 + 36
T_A, T_B, T_C, T_D, T_E, T_F = range(6)
N_TERMS = 6
EVERY = [1, 2, 3, 4, 5, 6]

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U32_MAX = (1 << 32) - 1
FLT_MIN_BITS, FLT_MAX_BITS = 0x00800000, 0x7F7FFFFF

# ------------------------------------------------------------------------------------------------ the rows
# dwords of a row: id (64 bits), blob offset (64 bits), a 32-bit attribute, three dwords of bit fields, a float, the ORDER BY
# attribute, and a 64-bit attribute in the LAST two dwords (the read the spare dword pair behind the device copy exists for)
D_ID, D_BLOB, D_U32, D_BFA, D_BFB, D_BFC, D_FLT, D_SORT, D_I64 = 0, 2, 4, 5, 6, 7, 8, 9, 10
STRIDE = 12
LOC = {"id": (D_ID * 32, 64), "u32": (D_U32 * 32, 32), "bfa1": (D_BFA * 32, 1), "bfa31": (D_BFA * 32 + 1, 31), "bfb31": (D_BFB * 32, 31),
       "bfb1": (D_BFB * 32 + 31, 1), "bfc5": (D_BFC * 32 + 27, 5), "flt": (D_FLT * 32, 32), "sort": (D_SORT * 32, 32), "i64": (D_I64 * 32, 64)}
N_BLOB = 3
BLOB_ID = {"m32": 0, "str": 1, "m64": 2}

U32_VALUES = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
ONES31 = 0x7FFFFFFF
# (the 1-bit field, the 31-bit field next to it): each field with all-ones and all-zero neighbours
BF_PAIRS = [(0, 0), (1, 0), (0, ONES31), (1, ONES31), (1, 0x2AAAAAAA), (0, 1), (1, 0x40000000)]
# (the 5-bit field at shift 27, the 27 bits below it)
BFC_PAIRS = [(0, 0), (0, 0x7FFFFFF), (31, 0), (31, 0x7FFFFFF), (21, 0x7FFFFFF), (10, 0), (1, 0x7FFFFFF), (16, 0), (16, 0x7FFFFFF)]
I64_VALUES = [I64_MIN, -1, 0, 1 << 31, U32_MAX, 1 << 32, I64_MAX]
NEG_DENORM, MID_DENORM = 0x80000400, 0x00012345
FLOAT_BITS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
              0x7FC00000, 0x7F800001, 0xFFC00001,              # quiet, signalling, negative NaN
              0x00000001, 0x007FFFFF, NEG_DENORM,              # the least and the largest denormal, a negative one
              FLT_MIN_BITS, FLT_MAX_BITS, 0xFF7FFFFF,          # FLT_MIN, +-FLT_MAX
              0x3F800000, 0xBFC00000, MID_DENORM, 0x42C88000]  # 1.0, -1.5, a denormal in between, 100.25
M32_LISTS = [[], [0], [1 << 31], [U32_MAX], [0, U32_MAX], [5, 1 << 31], [1 << 31, U32_MAX], [1, 2, 3], [3, 10, 20, 30], [0, 1], [10, 20]]
M64_LISTS = [[], [I64_MIN], [-1], [I64_MAX], [I64_MIN, I64_MAX], [-1, 0], [-5, 7, 100], [I64_MIN, -1, I64_MAX], [0], [-(1 << 33), 1 << 33],
             [7, 100], [-5, 7], [100, 1 << 40]]
ATTR_PERIODS = {"u32": 5, "bfa": 7, "bfb": 7, "bfc": 9, "i64": 7, "flt": 17, "m32": 11, "m64": 13}


def big_m32(n):
    """n sorted unique 32-bit values that hold 0, 2^31 and 2^32 - 1"""
    v = sorted({0, 1 << 31, U32_MAX} | {7 + i * 262143 for i in range(n - 3)})
    assert len(v) == n and v[-1] == U32_MAX
    return v


# rowid -> (MVA32 values, string length, MVA64 values): blob rows of a given TOTAL data size, on the block edges and the last rowid.
# 254 / 255 and 65534 / 65535 are the reference's class thresholds (CalcBlobRowFlags: < 0xFF one-byte lengths, < 0xFFFF two-byte ones)
SIZED_ROWS = {
    0: (0, ([], 0, [])),
    63: (254, ([0, 1 << 31], 230, [I64_MIN, -1])),
    64: (255, ([1 << 31, U32_MAX], 231, [-1, I64_MAX])),
    127: (65534, (big_m32(16370), 38, [I64_MIN, -1])),
    128: (65535, (big_m32(16370), 39, [-1, I64_MAX])),
    256: (0, ([], 0, [])),
    383: (256, ([0, U32_MAX], 232, [I64_MIN, I64_MAX])),
    N_DOCS - 1: (65536, (big_m32(16384), 0, [])),  # the neighbour of the MVA32 is empty (l0 == l1), and so is the MVA64
}


def pattern_index(attr, r):
    """which pattern of `attr` row r holds (blob attributes: of the rows outside SIZED_ROWS)"""
    p = ATTR_PERIODS[attr]
    return {"bfb": (3 * r + 1) % p, "i64": (3 * r + 2) % p}.get(attr, r % p)


def blob_values(r):
    if r in SIZED_ROWS:
        return SIZED_ROWS[r][1]
    slen = 0 if r % 9 == 4 else 1 + 2 * (r % 5)  # odd: the MVA64 behind it starts unaligned
    return M32_LISTS[pattern_index("m32", r)], slen, M64_LISTS[pattern_index("m64", r)]


def blob_bytes(r):
    m32, slen, m64 = blob_values(r)
    return [b"".join(v.to_bytes(4, "little") for v in m32), bytes((0xFF - 37 * i - r) & 0xFF for i in range(slen)),
            b"".join(v.to_bytes(8, "little", signed=True) for v in m64)]


@functools.lru_cache(maxsize=None)
def attr_rows():
    """-> (rows uint32 [N_DOCS, STRIDE], pool uint8) -- read-only"""
    from helpers import build_blob_pool

    pool, offs = build_blob_pool([blob_bytes(r) for r in range(N_DOCS)])
    rows = np.zeros((N_DOCS, STRIDE), np.uint32)
    for r in range(N_DOCS):
        doc_id = (1 << 33) + 7 * r
        rows[r, D_ID], rows[r, D_ID + 1] = doc_id & U32_MAX, doc_id >> 32
        rows[r, D_BLOB], rows[r, D_BLOB + 1] = offs[r] & U32_MAX, offs[r] >> 32
        rows[r, D_U32] = U32_VALUES[pattern_index("u32", r)]
        one, wide = BF_PAIRS[pattern_index("bfa", r)]
        rows[r, D_BFA] = one | (wide << 1)
        one, wide = BF_PAIRS[pattern_index("bfb", r)]
        rows[r, D_BFB] = wide | (one << 31)
        five, below = BFC_PAIRS[pattern_index("bfc", r)]
        rows[r, D_BFC] = below | (five << 27)
        rows[r, D_FLT] = FLOAT_BITS[pattern_index("flt", r)]
        rows[r, D_SORT] = (r * 37) % 13
        big = I64_VALUES[pattern_index("i64", r)] & ((1 << 64) - 1)
        rows[r, D_I64], rows[r, D_I64 + 1] = big & U32_MAX, big >> 32
    rows.setflags(write=False)
    pool.setflags(write=False)
    return rows, pool


def dead_map():
    """every 8th row from 3 on (no attribute pattern dies out: the periods are odd), and the block edges 127 / 128"""
    dead = np.zeros((N_DOCS + 31) // 32, np.uint32)
    for r in list(range(3, N_DOCS, 8)) + [127, 128]:
        dead[r >> 5] |= np.uint32(1 << (r & 31))
    return dead


def is_dead(dead, r):
    return bool((int(dead[r >> 5]) >> (r & 31)) & 1)


# ------------------------------------------------------------------------------------------------ the postings
def field_weights(n_fields):
    """negative ones among them: weights fall below 0"""
    return ([3, -2, 5, -7, 1, -1, 2, -3] * 4)[:n_fields]


@functools.lru_cache(maxsize=None)
def hits(n_fields):
    """-> index_from_hits' arrays.  Doc r holds its keywords side by side (positions 1..6) in field (r + r // 8) % n_fields (so the docs
    of B, every 2nd one, reach the fields of negative weight too); every third doc holds A once more in another field."""
    rows = []
    for r in range(N_DOCS):
        f = (r + r // 8) % n_fields
        for t in range(N_TERMS):
            if r % EVERY[t] == 0:
                rows.append((t + 1, r, (f << 24) | (1 + t)))
        if r % 3 == 1:
            rows.append((T_A + 1, r, (((r * 7 + 3) % n_fields) << 24) | 9))
    a = np.array(sorted(rows), np.uint64)
    return a[:, 0].copy(), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32)


SEGMENTS = [("N", 8), ("W", 32)]
SEGMENT_IDS = [s[0] for s in SEGMENTS]


@functools.lru_cache(maxsize=None)
def segment(name):
    """-> HostIndex of the 8-field corpus N or of its 32-field twin W"""
    import manticoresearch_amd as m

    n_fields = dict(SEGMENTS)[name]
    W, R, H = hits(n_fields)
    return m.index_from_hits(W, R, H, n_terms=N_TERMS, total_docs=N_DOCS, n_fields=n_fields)


# ------------------------------------------------------------------------------------------------ the model
def get_row_attr(row, bit_offset, bit_count):
    """sphGetRowAttr: SphAttr_t ( pRow[iItem] ) zero-extends; 64 bits are read as a signed SphAttr_t"""
    item = bit_offset >> 5
    if bit_count == 32:
        return int(row[item])
    if bit_count == 64:
        u = int(row[item]) | (int(row[item + 1]) << 32)
        return u - (1 << 64) if u >> 63 else u
    return (int(row[item]) >> (bit_offset & 31)) & ((1 << bit_count) - 1)


def blob_size_class(total):
    """CalcBlobRowFlags"""
    return 0 if total < 0xFF else 1 if total < 0xFFFF else 2


def blob_attr(pool, off, attr_id, n_attrs):
    """GetBlobAttr: the bytes of one blob attribute of the blob row at pool[off]"""
    flags = int(pool[off])
    assert flags in (0, 1, 2), "Unknown blob row type"
    sz = (1, 2, 4)[flags]
    base = off + 1

    def length(i):
        return int.from_bytes(bytes(pool[base + i * sz: base + (i + 1) * sz]), "little")

    l1 = length(attr_id)
    l0 = length(attr_id - 1) if attr_id > 0 else 0
    assert l1 >= l0
    start = base + n_attrs * sz + l0
    return bytes(pool[start: start + l1 - l0])


def mva_of(blob, bits):
    """the MVA as the reference's T reads it: DWORD (unsigned) or int64_t"""
    w = bits // 8
    return [int.from_bytes(blob[i * w: (i + 1) * w], "little", signed=(bits == 64)) for i in range(len(blob) // w)]


def eval_range(v, lo, hi, eq_min, eq_max, open_left=False, open_right=False):
    if open_left:
        return v <= hi if eq_max else v < hi
    if open_right:
        return v >= lo if eq_min else v > lo
    return bool((v >= lo if eq_min else v > lo) and (v <= hi if eq_max else v < hi))


def eval_values(v, values):
    """IFilter_Values::EvalValues, as written"""
    a, b = 0, len(values) - 1
    if v == values[a] or v == values[b]:
        return True
    if v < values[a] or v > values[b]:
        return False
    while b - a > 1:
        mid = a + (b - a) // 2
        if v == values[mid]:
            return True
        if v < values[mid]:
            b = mid
        else:
            a = mid
    return False


def mva_any(mva, values):
    if not mva or not values:
        return False
    lo = 0  # L: NOT reset between the filter values
    for f in values:
        hi = len(mva) - 1
        while lo <= hi:
            mid = lo + (hi - lo) // 2
            if f > mva[mid]:
                lo = mid + 1
            elif f < mva[mid]:
                hi = mid - 1
            else:
                return True
    return False


def mva_all(mva, values):
    if not mva or not values:
        return False
    return all(v in values for v in mva)


def mva_range_any(mva, lo_v, hi_v, eq_min, eq_max):
    if not mva:  # ( !pMva )
        return False
    n = len(mva)
    lo, hi = 0, n - 1
    while lo <= hi:
        mid = lo + (hi - lo) // 2
        if lo_v > mva[mid]:
            lo = mid + 1
        elif lo_v < mva[mid]:
            hi = mid - 1
        else:
            return bool(eq_min or mid + 1 < n)  # (the next value is not tested against the maximum)
    if lo == n:
        return False
    return mva[lo] <= hi_v if eq_max else mva[lo] < hi_v


def mva_range_all(mva, lo_v, hi_v, eq_min, eq_max, bits):
    if not mva:
        return False
    if bits == 32:  # (T)m_iMinValue, (T)m_iMaxValue with T = DWORD
        lo_v, hi_v = lo_v & U32_MAX, hi_v & U32_MAX
    return bool((mva[0] >= lo_v if eq_min else mva[0] > lo_v) and (mva[-1] <= hi_v if eq_max else mva[-1] < hi_v))


_mva_cache = {}


def row_mva(r, rows, pool, attr_id, n_attrs, bits):
    key = (id(pool), r, attr_id, n_attrs, bits)
    if key not in _mva_cache:
        off = int(rows[r, D_BLOB]) | (int(rows[r, D_BLOB + 1]) << 32)
        _mva_cache[key] = mva_of(blob_attr(pool, off, attr_id, n_attrs), bits)
    return _mva_cache[key]


def filter_eval(f, r, rows, pool):
    """one filter dict (the oracle's spelling, Filter.as_dict) over row r, m_bExclude applied"""
    eq_min, eq_max = f.get("has_equal_min", True), f.get("has_equal_max", True)
    if f.get("mva_bits"):
        mva = row_mva(r, rows, pool, f["blob_attr_id"], f["n_blob_attrs"], f["mva_bits"])
        if "values" in f:
            ok = mva_all(mva, f["values"]) if f.get("mva_all") else mva_any(mva, f["values"])
        elif f.get("mva_all"):
            ok = mva_range_all(mva, f["min"], f["max"], eq_min, eq_max, f["mva_bits"])
        else:
            ok = mva_range_any(mva, f["min"], f["max"], eq_min, eq_max)
    else:
        v = get_row_attr(rows[r], f["bit_offset"], f["bit_count"])
        if "values" in f:
            ok = eval_values(v, f["values"])
        elif "fmin" in f:  # GetAttrFloat = sphDW2F ( (DWORD) GetAttr ); no open-sided form
            fv = np.array([v & U32_MAX], np.uint32).view(np.float32)[0]
            lo, hi = np.float32(f["fmin"]), np.float32(f["fmax"])
            ok = bool((fv >= lo if eq_min else fv > lo) and (fv <= hi if eq_max else fv < hi))
        else:
            ok = eval_range(v, f["min"], f["max"], eq_min, eq_max, f.get("open_left", False), f.get("open_right", False))
    return (not ok) if f.get("exclude") else bool(ok)


def row_passes(filters, r, rows, pool):
    return all(filter_eval(f, r, rows, pool) for f in filters)


def weight_passes(wfilters, weight):
    """Filter_WeightValues: EvalValues ( m_iWeight ); Filter_WeightRange: EvalRange<eq_min, eq_max> ( (SphAttr_t) m_iWeight, .. )"""
    for f in wfilters:
        ok = eval_values(int(weight), f["values"]) if "values" in f else eval_range(int(weight), f["min"], f["max"], f.get("has_equal_min", True), f.get("has_equal_max", True))
        if bool(ok) == bool(f.get("exclude")):
            return False
    return True


def model_rows(case, candidates, rows, pool, dead=None, cutoff=0):
    """the rowids of `candidates` (ascending) that the case's filters let through; cutoff counts the rows that passed"""
    out = []
    for r in candidates:
        if row_passes(case.filters, r, rows, pool) and not (dead is not None and is_dead(dead, r)):
            out.append(r)
            if cutoff and len(out) == cutoff:
                break
    return out


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, filters, trivial=None):
        self.name, self.filters, self.trivial = name, filters, trivial  # trivial: "all" / "none" where that answer is the point

    def __repr__(self):
        return self.name


def F(loc, **kw):
    off, cnt = LOC[loc]
    return dict(bit_offset=off, bit_count=cnt, **kw)


def MV(attr, **kw):
    return dict(bit_offset=0, bit_count=0, mva_bits=32 if attr == "m32" else 64, blob_attr_id=BLOB_ID[attr], n_blob_attrs=N_BLOB, **kw)


def f32(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


INF, NAN = float("inf"), float("nan")


@functools.lru_cache(maxsize=None)
def cases():
    c = []

    def add(name, *filters, trivial=None):
        c.append(Case(name, list(filters), trivial))

    # --- VALUES over the 32-bit attribute: a row of 0xFFFFFFFF is 2^32 - 1, never -1; 0x80000000 is 2^31, never negative
    add("u32_values_ends", F("u32", values=[0, U32_MAX]))
    add("u32_values_minus1_and_2p32", F("u32", values=[-1, 1 << 32]), trivial="none")
    add("u32_values_minus1_1_2p32", F("u32", values=[-1, 1, 1 << 32]))
    add("u32_values_int32_min", F("u32", values=[-(1 << 31), ONES31]))
    add("u32_values_beside", F("u32", values=[2, ONES31 - 1, 1 << 31, (1 << 31) + 1, U32_MAX - 1]))
    add("u32_values_8", F("u32", values=[-1, 0, 2, ONES31, (1 << 31) + 1, U32_MAX - 1, U32_MAX, 1 << 32]))
    add("u32_values_exclude", F("u32", values=[1, 1 << 31], exclude=True))
    # --- RANGE [1, 2^31] over it: every flag combination, the bounds are row values
    for eq_min in (1, 0):
        for eq_max in (1, 0):
            for ol in (0, 1):
                for orr in (0, 1):
                    for ex in (0, 1):
                        add(f"u32_range_eq{eq_min}{eq_max}_open{ol}{orr}_ex{ex}", F("u32", min=1, max=1 << 31, has_equal_min=bool(eq_min), has_equal_max=bool(eq_max),
                                                                                  open_left=bool(ol), open_right=bool(orr), exclude=bool(ex)))
    add("u32_range_negative_min", F("u32", min=-5, max=1))
    add("u32_range_to_2p32", F("u32", min=1 << 31, max=1 << 32))
    add("u32_range_strict_at_max", F("u32", min=ONES31, max=U32_MAX, has_equal_min=False, has_equal_max=False))
    # --- the 64-bit attribute in the row's last two dwords, and the id in its first two
    add("i64_values_ends", F("i64", values=[I64_MIN, I64_MAX]))
    add("i64_values_beside", F("i64", values=[I64_MIN + 1, -2, -1, 1, U32_MAX, I64_MAX - 1]))
    add("i64_values_8", F("i64", values=[I64_MIN, -2, 0, 1 << 31, (1 << 32) + 1, 1 << 33, I64_MAX - 1, I64_MAX]))
    add("i64_values_low_dword_only", F("i64", values=[U32_MAX - 1, U32_MAX], exclude=True))
    add("i64_range_full", F("i64", min=I64_MIN, max=I64_MAX), trivial="all")
    add("i64_range_full_strict", F("i64", min=I64_MIN, max=I64_MAX, has_equal_min=False, has_equal_max=False))
    add("i64_range_inverted", F("i64", min=5, max=-5), trivial="none")
    add("i64_range_inverted_exclude", F("i64", min=5, max=-5, exclude=True), trivial="all")
    add("i64_range_inverted_open_left", F("i64", min=5, max=-5, open_left=True))
    add("i64_range_2p31_2p32", F("i64", min=1 << 31, max=1 << 32))
    add("i64_range_2p31_2p32_strict", F("i64", min=1 << 31, max=1 << 32, has_equal_min=False, has_equal_max=False))
    add("i64_range_negative", F("i64", min=I64_MIN, max=-1, has_equal_min=False))
    add("i64_range_open_right_at_max", F("i64", min=I64_MAX, max=0, open_right=True))
    add("id_range", F("id", min=(1 << 33) + 7 * 100, max=(1 << 33) + 7 * 300, has_equal_max=False))
    # --- bit fields: 1 bit at shift 0 and 31, 31 bits at shift 1 and 0, 5 bits at shift 27
    add("bfa1_is_1", F("bfa1", values=[1]))
    add("bfa31_ends", F("bfa31", values=[0, ONES31]))
    add("bfa31_inner", F("bfa31", values=[1, 0x2AAAAAAA, 0x40000000, 1 << 31]))
    add("bfa31_range", F("bfa31", min=1, max=ONES31 - 1))
    add("bfb31_ends", F("bfb31", values=[0, ONES31]))
    add("bfb31_range_strict", F("bfb31", min=0, max=ONES31, has_equal_min=False, has_equal_max=False))
    add("bfb1_is_1", F("bfb1", values=[1]))
    add("bfb1_not_0", F("bfb1", values=[0], exclude=True))
    add("bfc5_ends", F("bfc5", values=[0, 31]))
    add("bfc5_inner", F("bfc5", values=[1, 16, 21, 32]))
    add("bfc5_range", F("bfc5", min=10, max=21))
    # --- float ranges: both bounds always, NaN fails every comparison, denormals are numbers
    add("flt_zeros", F("flt", fmin=-0.0, fmax=0.0))
    add("flt_0_to_flt_min_strict", F("flt", fmin=0.0, fmax=f32(FLT_MIN_BITS), has_equal_min=False, has_equal_max=False))
    add("flt_denormal_bounds", F("flt", fmin=f32(NEG_DENORM), fmax=f32(MID_DENORM)))
    add("flt_denormal_bounds_strict", F("flt", fmin=f32(NEG_DENORM), fmax=f32(MID_DENORM), has_equal_min=False, has_equal_max=False))
    add("flt_least_denormal_up", F("flt", fmin=f32(1), fmax=f32(0x007FFFFF), has_equal_min=False))
    add("flt_nan_min", F("flt", fmin=NAN, fmax=1.0), trivial="none")
    add("flt_nan_max", F("flt", fmin=-1.0, fmax=NAN), trivial="none")
    add("flt_nan_min_exclude", F("flt", fmin=NAN, fmax=1.0, exclude=True), trivial="all")
    add("flt_inf_inclusive", F("flt", fmin=-INF, fmax=INF))
    add("flt_inf_strict", F("flt", fmin=-INF, fmax=INF, has_equal_min=False, has_equal_max=False))
    add("flt_max_exclude", F("flt", fmin=f32(0xFF7FFFFF), fmax=f32(FLT_MAX_BITS), exclude=True))
    add("flt_strict_above_flt_max", F("flt", fmin=f32(FLT_MAX_BITS), fmax=INF, has_equal_min=False))
    add("flt_strict_below_minus_flt_max", F("flt", fmin=-INF, fmax=f32(0xFF7FFFFF), has_equal_max=False))
    add("flt_negative", F("flt", fmin=-2.0, fmax=-0.0))
    # --- MVA, values
    add("m32_any_ends", MV("m32", values=[0, 1 << 31, U32_MAX]))
    add("m32_any_minus1_3_2p32", MV("m32", values=[-1, 3, 1 << 32]))
    add("m32_any_walks_on", MV("m32", values=[2, 10, 25]))
    add("m32_any_8", MV("m32", values=[-1, 1, 4, 20, 262150, (1 << 31) - 1, U32_MAX - 1, 1 << 32]))
    add("m32_all_ends", MV("m32", values=[0, 1 << 31, U32_MAX], mva_all=True))
    add("m32_all_8", MV("m32", values=[0, 1, 2, 3, 5, 10, 20, 30], mva_all=True))
    add("m64_any_ends", MV("m64", values=[I64_MIN, I64_MAX]))
    add("m64_any_minus1", MV("m64", values=[-1]))
    add("m64_any_8", MV("m64", values=[I64_MIN + 1, -5, 0, 7, 1 << 33, 1 << 40, I64_MAX - 1, I64_MAX]))
    add("m64_all_ends", MV("m64", values=[I64_MIN, -1, 0, I64_MAX], mva_all=True))
    add("m64_all_small", MV("m64", values=[-5, 7, 100], mva_all=True))
    # every exclude form over an empty list: the test fails on it, so the row passes
    add("m32_any_exclude", MV("m32", values=[0, 3, U32_MAX], exclude=True))
    add("m32_all_exclude", MV("m32", values=[0, 1, U32_MAX], mva_all=True, exclude=True))
    add("m32_range_any_exclude", MV("m32", min=2, max=1 << 31, exclude=True))
    add("m32_range_all_exclude", MV("m32", min=0, max=1 << 31, mva_all=True, exclude=True))
    add("m64_any_exclude", MV("m64", values=[-1, 7], exclude=True))
    add("m64_all_exclude", MV("m64", values=[I64_MIN, -1, 0, 7, 100, I64_MAX], mva_all=True, exclude=True))
    add("m64_range_any_exclude", MV("m64", min=-5, max=100, exclude=True))
    add("m64_range_all_exclude", MV("m64", min=-5, max=I64_MAX, mva_all=True, exclude=True))
    # --- MVA, range-any: [10, 20] finds the minimum 20 at its LAST position, [3, 10, 20, 30] at an inner one with 30 > max behind it
    add("m32_rany_min_found_strict", MV("m32", min=20, max=25, has_equal_min=False))
    add("m32_rany_min_found", MV("m32", min=20, max=25))
    add("m32_rany_min_below_all", MV("m32", min=-7, max=2))
    add("m32_rany_min_above_some", MV("m32", min=31, max=1 << 33))
    add("m32_rany_min_above_all", MV("m32", min=1 << 32, max=1 << 40), trivial="none")
    add("m32_rany_strict_max", MV("m32", min=4, max=10, has_equal_max=False))
    add("m32_rany_inclusive_max", MV("m32", min=4, max=10))
    add("m32_rany_at_2p31", MV("m32", min=1 << 31, max=1 << 31, has_equal_min=False))
    add("m64_rany_min_found_strict", MV("m64", min=I64_MIN, max=-1, has_equal_min=False))
    add("m64_rany_at_min", MV("m64", min=I64_MIN, max=I64_MIN))
    add("m64_rany_to_max", MV("m64", min=1, max=I64_MAX, has_equal_max=False))
    add("m64_rany_inner", MV("m64", min=7, max=50, has_equal_min=False))
    # --- MVA, range-all: the bounds are cast to the MVA's type
    add("m32_rall_min_minus1", MV("m32", min=-1, max=U32_MAX, mva_all=True))
    add("m32_rall_max_2p32_plus_5", MV("m32", min=0, max=(1 << 32) + 5, mva_all=True))
    add("m32_rall_plain_strict_min", MV("m32", min=1, max=30, mva_all=True, has_equal_min=False))
    add("m32_rall_upper_half", MV("m32", min=1 << 31, max=U32_MAX, mva_all=True))
    add("m64_rall_full", MV("m64", min=I64_MIN, max=I64_MAX, mva_all=True))
    add("m64_rall_full_strict", MV("m64", min=I64_MIN, max=I64_MAX, mva_all=True, has_equal_min=False, has_equal_max=False))
    add("m64_rall_negative", MV("m64", min=I64_MIN, max=-1, mva_all=True))
    add("m64_rall_2p33", MV("m64", min=-(1 << 33), max=1 << 33, mva_all=True, has_equal_max=False))
    # --- two filters, both orders
    pairs = [(F("u32", min=1, max=1 << 31), F("i64", values=[I64_MIN, -1, U32_MAX, I64_MAX])),
             (F("flt", fmin=f32(NEG_DENORM), fmax=INF), MV("m32", values=[0, 3, U32_MAX])),
             (MV("m64", min=I64_MIN, max=-1, mva_all=True), F("bfc5", values=[0, 16, 31])),
             (MV("m32", min=-1, max=U32_MAX, mva_all=True, exclude=True), MV("m64", min=I64_MIN, max=-1, has_equal_min=False)),
             (F("bfa31", values=[0, ONES31], exclude=True), F("bfb1", values=[1]))]
    for i, (a, b) in enumerate(pairs):
        add(f"pair{i}_ab", a, b)
        add(f"pair{i}_ba", b, a)
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


TRIVIAL = {"u32_values_minus1_and_2p32": "none", "i64_range_full": "all", "i64_range_inverted": "none", "i64_range_inverted_exclude": "all",
           "flt_nan_min": "none", "flt_nan_max": "none", "flt_nan_min_exclude": "all", "m32_rany_min_above_all": "none"}


def weight_cases(weights):
    """[(name, row filters, weight filters)] for one route, from the weights of its unfiltered answer: ranges that straddle 0, values
    that hold a negative weight.  Which weights exist is read from the answer; what a filter does with them is the model's business."""
    distinct = sorted(set(int(w) for w in weights))
    neg, pos = [w for w in distinct if w < 0], [w for w in distinct if w > 0]
    assert len(neg) >= 2 and len(pos) >= 2, "the negative field weights put weights on both sides of 0"
    lo, hi = neg[len(neg) // 2], pos[len(pos) // 2]
    vals = sorted({neg[0], neg[-1], -1, 0, 1, pos[0], pos[-1], hi})[:8]
    out = [("w_range_straddles_0", [], [dict(bit_offset=0, bit_count=0, min=lo, max=hi)]),
           ("w_range_straddles_0_strict", [], [dict(bit_offset=0, bit_count=0, min=lo, max=hi, has_equal_min=False, has_equal_max=False)]),
           ("w_range_straddles_0_exclude", [], [dict(bit_offset=0, bit_count=0, min=lo, max=hi, exclude=True)]),
           ("w_range_below_0", [], [dict(bit_offset=0, bit_count=0, min=-(1 << 31), max=-1)]),
           ("w_range_from_0", [], [dict(bit_offset=0, bit_count=0, min=0, max=I64_MAX, has_equal_min=False)]),
           ("w_range_one_negative_weight", [], [dict(bit_offset=0, bit_count=0, min=neg[-1], max=neg[-1])]),
           ("w_values_negative", [], [dict(bit_offset=0, bit_count=0, values=vals)]),
           ("w_values_negative_exclude", [], [dict(bit_offset=0, bit_count=0, values=[neg[0], neg[-1]], exclude=True)]),
           ("w_two_filters", [], [dict(bit_offset=0, bit_count=0, min=lo, max=I64_MAX), dict(bit_offset=0, bit_count=0, values=[hi], exclude=True)]),
           ("w_next_to_u32", [F("u32", min=1, max=1 << 31)], [dict(bit_offset=0, bit_count=0, min=lo, max=hi)]),
           ("w_next_to_m64", [MV("m64", values=[I64_MIN, -1])], [dict(bit_offset=0, bit_count=0, min=-(1 << 31), max=0, exclude=True)])]
    return out


# ------------------------------------------------------------------------------------------------ the DevFilter image
DEV_FILTER = np.dtype([("kind", "<u4"), ("item", "<u4"), ("shift", "<u4"), ("bits", "<u4"), ("n_values", "<u4"), ("mva", "<u4"), ("lo", "<i8"), ("hi", "<i8"),
                       ("values", "<i8", (8,))])
assert DEV_FILTER.itemsize == 104


def dev_filter(f, on_weight=False):
    """one filter dict packed the way mrk_plan.cpp's translate_filter packs a mrk_filter into a DevFilter"""
    d = np.zeros((), DEV_FILTER)
    kind = 0 if "values" in f else 2 if "fmin" in f else 1
    in_row = not on_weight and not f.get("mva_bits")
    if not on_weight and f.get("mva_bits"):
        d["mva"] = f["mva_bits"] | (int(bool(f.get("mva_all"))) << 8) | (f["blob_attr_id"] << 16) | (f["n_blob_attrs"] << 24)
    elif in_row:
        d["item"], d["shift"], d["bits"] = f["bit_offset"] >> 5, f["bit_offset"] & 31, f["bit_count"]
    k = kind | (int(bool(f.get("exclude"))) << 8) | (int(bool(f.get("has_equal_min", True))) << 9) | (int(bool(f.get("has_equal_max", True))) << 10)
    if in_row:
        k |= (int(bool(f.get("open_left"))) << 11) | (int(bool(f.get("open_right"))) << 12)
    d["kind"] = k
    d["lo"], d["hi"] = f.get("min", 0), f.get("max", 0)
    if kind == 2:
        d["lo"], d["hi"] = (int(np.array([f[key]], np.float32).view(np.uint32)[0]) for key in ("fmin", "fmax"))
    if kind == 0:
        d["n_values"] = len(f["values"])
        d["values"][: len(f["values"])] = f["values"]
    return d
