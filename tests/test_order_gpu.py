"""Ordered row scan on the GPU: Engine.select(..., order_by=...) against numpy
over the arrays the test generated (never the engine, never the oracle; the
oracle module only encodes the input blobs).

The reference is a stable sort on (null class, canonical key, scan position):
the canonical key is written independently of the engine's encoding — integers
as they are, floats as (isnan, value with -0.0 folded), strings as their bytes
— turned into dense ranks by np.lexsort, negated for DESC.  Every comparison
is on raw bytes of every projected column, ROWID and validity included, and
every case asserts 0 < k_eff and that its reference differs from the first
k_eff matching rows in scan order unless it is named in SCAN_ORDER_OK.

The base table's batches are 17445 rows (a full 16 K tile, one full chunk, a
37-row tail), the same again, 63 rows (less than a wave), 1 row and 16384 rows
(exactly one tile)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se

pytestmark = pytest.mark.gpu

ROWID = abi.PROJ_ROWID
SIZES = (17445, 17445, 63, 1, 16384)
KS = (1, 63, 64, 65, 1000, 8192)
NAN_A, NAN_B = 0x7FF8000000000001, 0xFFF4000000ABCDEF
FNAN_A, FNAN_B = 0x7FC00001, 0xFFA00123
WORDS = [b"TRUCK", b"AIRX", b"AIR", b"MAIL", b"\xc3\xa9t\xc3\xa9", b"RAIL",
         b"SHIP", b"AIR ", b"zebra", b"FOB", b"\x80up"]
# cases whose result is, by construction, a prefix of the scan order
SCAN_ORDER_OK = {"all-equal", "bool-desc-k1", "bitset-desc-k1"}


def bits(x):
    return np.array(x, dtype=np.uint64).view(np.float64)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        bool((a.view(np.uint8) == b.view(np.uint8)).all())


# ---- the reference ----

def canon(v):
    """canonical key components of a value array, major first"""
    if v.dtype.kind == "f":
        nan = np.isnan(v)
        return [nan, np.where(nan | (v == 0), 0, v).astype(v.dtype)]
    return [v]


def dense_rank(components):
    order = np.lexsort(tuple(reversed(components)))
    step = np.zeros(len(order), dtype=bool)
    for c in components:
        s = c[order]
        step[1:] |= s[1:] != s[:-1]
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.cumsum(step)
    return rank


class Tab:
    """a table's reference image: val[c] (NULL rows zeroed), ok[c], canonical
    components key[c], live rows, (batch, ordinal) per row"""

    def reference(self, mask, c, k, desc=False, nulls_first=None):
        idx = np.flatnonzero(mask & self.live)
        rank = dense_rank([x[idx] for x in self.key[c]])
        if desc:
            rank = -rank
        ok = self.ok[c][idx]
        if nulls_first is None:
            nulls_first = not desc
        cls = np.where(ok, 1, 0 if nulls_first else 2)
        rank = np.where(ok, rank, 0)
        order = np.lexsort((idx, rank, cls))
        return idx[order][:k], idx[:k]


def check(tb, rs, idx, cols, name=""):
    assert rs.count() == len(idx), (name, rs.count(), len(idx))
    for p, c in enumerate(cols):
        vals, valid = rs.column(p)
        if c == ROWID:
            gb, go = rs.rowids(p)
            assert valid.all(), name
            assert same_bytes(gb, tb.batch[idx]), (name, "rowid batch")
            assert same_bytes(go, tb.ordinal[idx]), (name, "rowid ordinal")
        elif c in tb.words:
            exp = [tb.words[c][i] for i in tb.val[c][idx]]
            assert rs.strings(p) == exp, (name, "strings")
        else:
            assert same_bytes(valid, tb.ok[c][idx]), (name, c, "validity")
            exp = tb.val[c][idx]
            if c in tb.nan_payload_free:
                nan = np.isnan(exp)
                assert same_bytes(np.isnan(vals), nan), (name, c)
                assert same_bytes(vals[~nan], exp[~nan]), (name, c)
            else:
                assert same_bytes(vals, exp), (name, c)


def run(tb, preds, mask, cols, c, k, name, desc=False, nulls_first=None):
    """one ordered query against the reference; returns (RowSet, reference)"""
    exp, scan = tb.reference(mask, c, k, desc, nulls_first)
    assert 0 < len(exp), name
    if name in SCAN_ORDER_OK:
        assert (exp == scan).all(), name
    else:
        assert not (exp == scan).all(), (name, "ordering is a no-op here")
    rs = tb.eng.select(abi.make_plan(table=tb.t, preds=preds), cols, limit=k,
                       order_by=c, descending=desc, nulls_first=nulls_first)
    check(tb, rs, exp, cols, name)
    assert rs.rows_passed() == int((mask & tb.live).sum()), name
    return rs, exp


# ---- the base table: every key type, clean batches ----

ID, I32, I64, F64, I16, I8, BO, STR, F32, T3, EQ, NARROW = range(12)
BASE_TYPES = [po.T_INT32, po.T_INT32, po.T_INT64, po.T_DOUBLE, po.T_INT16,
              po.T_INT8, po.T_BOOL, po.T_STRING, po.T_FLOAT, po.T_INT32,
              po.T_INT32, po.T_DOUBLE]
BASE_ABI = [abi.T_INT32, abi.T_INT32, abi.T_INT64, abi.T_DOUBLE, abi.T_INT16,
            abi.T_INT8, abi.T_BOOL, abi.T_STRING, abi.T_FLOAT, abi.T_INT32,
            abi.T_INT32, abi.T_DOUBLE]


def make_base():
    rng = np.random.default_rng(20241021)
    f64_special = np.concatenate([
        bits([NAN_A, NAN_B]),
        np.array([-0.0, 0.0, np.inf, -np.inf, 5e-324, -5e-324])])
    f32_special = np.concatenate([
        np.array([FNAN_A, FNAN_B], dtype=np.uint32).view(np.float32),
        np.array([-0.0, 0.0, np.inf, -np.inf, 1e-45], dtype=np.float32)])
    nvals = np.concatenate([np.arange(11) / 128.0, np.array([-0.0]),
                            bits([NAN_A])])
    out, start = [], 0
    for n in SIZES:
        ident = np.arange(start, start + n, dtype=np.int32)
        i32 = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
        i32[rng.integers(0, n, max(1, n // 50))] = 2 ** 31 - 1
        i32[rng.integers(0, n, max(1, n // 50))] = -2 ** 31
        i64 = rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)
        i64[::3] += np.int64(2 ** 62)
        i64[1::3] -= np.int64(2 ** 62)
        f64 = rng.standard_normal(n) * 1e6
        at = rng.integers(0, n, max(1, n // 9))
        f64[at] = f64_special[rng.integers(0, len(f64_special), len(at))]
        i16 = rng.integers(-32768, 32768, n).astype(np.int16)
        i8 = rng.integers(-128, 128, n).astype(np.int8)
        bo = (rng.random(n) > 0.5).astype(np.uint8)
        w = rng.integers(0, len(WORDS), n).astype(np.int64)
        f32 = (rng.standard_normal(n) * 100).astype(np.float32)
        at = rng.integers(0, n, max(1, n // 9))
        f32[at] = f32_special[rng.integers(0, len(f32_special), len(at))]
        t3 = rng.integers(0, 3, n).astype(np.int32)
        eq = np.full(n, 7, dtype=np.int32)
        nn = nvals[rng.integers(0, len(nvals), n)]
        if start == 0:
            # the first row is neither smallest nor largest of any key
            i32[0], i64[0], f64[0], i16[0], i8[0] = 0, 0, 0.5, 0, 0
            bo[0], bo[1], f32[0], t3[0], nn[0] = 1, 0, 0.5, 1, 5 / 128.0
            w[0] = WORDS.index(b"MAIL")
        out.append([ident, i32, i64, f64, i16, i8, bo, w, f32, t3, eq, nn])
        start += n
    return out


def base_blobs(cols):
    U = po.ENC_UNCOMPRESSED
    blobs = []
    for c, (dt, v) in enumerate(zip(BASE_TYPES, cols)):
        if c == STR:
            blobs.append(po.encode(dt, po.ENC_DICT, [WORDS[i] for i in v]))
        elif c == I8:
            blobs.append(po.encode(dt, U, v.view(np.uint8)))
        else:
            blobs.append(po.encode(dt, U, v))
    return blobs


def base_stats(cols):
    n = len(cols[ID])
    lo = [0] * len(BASE_TYPES)
    hi = [0] * len(BASE_TYPES)
    lo[ID], hi[ID] = int(cols[ID].min()), int(cols[ID].max())
    hb = [0] * len(BASE_TYPES)
    hb[ID] = 1
    return po.encode_stats(BASE_TYPES, n, lo, hi,
                           null_counts=[0] * len(BASE_TYPES), has_bounds=hb)


@pytest.fixture(scope="module")
def base():
    tb = Tab()
    batches = make_base()
    tb.eng = se.Engine(device=0)
    tb.t = tb.eng.table_define("ord_base", [(dt, False) for dt in BASE_ABI])
    for bi, cols in enumerate(batches):
        tb.eng.batch_put(tb.t, 1000 + bi, 3 * bi, len(cols[0]),
                         base_blobs(cols), stats=base_stats(cols))
    ncol = len(BASE_TYPES)
    tb.val = {c: np.concatenate([b[c] for b in batches]) for c in range(ncol)}
    tb.nrows = len(tb.val[ID])
    tb.ok = {c: np.ones(tb.nrows, dtype=bool) for c in range(ncol)}
    tb.words = {STR: WORDS}
    tb.nan_payload_free = set()
    tb.key = {c: canon(tb.val[c]) for c in range(ncol)}
    byte_rank = {w: r for r, w in enumerate(sorted(WORDS))}
    tb.key[STR] = [np.array([byte_rank[WORDS[i]] for i in tb.val[STR]])]
    tb.live = np.ones(tb.nrows, dtype=bool)
    tb.batch = np.concatenate([np.full(len(b[0]), bi, dtype=np.int64)
                               for bi, b in enumerate(batches)])
    tb.ordinal = np.concatenate([np.arange(len(b[0]), dtype=np.int64)
                                 for b in batches])
    tb.starts = np.cumsum((0,) + SIZES)[:-1]
    tb.all = np.ones(tb.nrows, dtype=bool)
    yield tb
    tb.eng.close()


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("c", [I8, I16, I32, I64, BO, STR, F32, F64],
                         ids=["i8", "i16", "i32", "i64", "bool", "str", "f32",
                              "f64"])
def test_every_key_type(base, c, desc):
    tb = base
    cols = [ID, c, ROWID, F64]
    for k in KS:
        name = "bool-desc-k1" if (c == BO and desc and k == 1) else f"k{k}"
        rs, exp = run(tb, [], tb.all, cols, c, k, name, desc)
        assert rs.count() == k
    if c == F64:
        # the special values are among the keys, and come back bit for bit
        rs, exp = run(tb, [], tb.all, [F64], F64, 8192, "f64-special", desc)
        got = rs.column(0)[0].view(np.uint64)
        want = (NAN_A, NAN_B) if desc else (0xFFF0000000000000,)
        for pattern in want:
            assert (got == np.uint64(pattern)).any(), hex(pattern)


def test_fewer_matching_rows_than_k(base):
    tb = base
    lo, hi = 17000, 17499                      # 500 rows across two batches
    mask = (tb.val[ID] >= lo) & (tb.val[ID] <= hi)
    for c, desc in [(I64, False), (F64, True), (STR, False)]:
        rs, exp = run(tb, [dict(col=ID, lo=lo, hi=hi)], mask,
                      [c, ID, ROWID], c, 1000, "few", desc)
        assert rs.count() == 500 == len(exp)


# ---- digit coverage: each radix pass is the deciding one ----

def make_digits():
    rng = np.random.default_rng(11)
    sizes = (5000, 3000)
    base64 = np.uint64(0x3FF0000000000123)
    base32 = np.uint32(0x40000123)
    cols = []
    for d in range(6):
        j = rng.integers(0, 2048, sum(sizes)).astype(np.uint64)
        j &= np.uint64(2047 if d < 5 else 511)
        cols.append((base64 ^ (j << np.uint64(11 * d))).view(np.int64))
    for d in range(6):
        j = rng.integers(0, 2048, sum(sizes)).astype(np.uint64)
        j &= np.uint64(2047 if d < 5 else 511)
        cols.append((base64 ^ (j << np.uint64(11 * d))).view(np.float64))
    for d in range(3):
        j = rng.integers(0, 2048, sum(sizes)).astype(np.uint32)
        j &= np.uint32(2047 if d < 2 else 1023)
        cols.append((base32 ^ (j << np.uint32(11 * d))).view(np.int32))
    cols.append(np.arange(sum(sizes), dtype=np.int32))
    return sizes, cols


DIG_TYPES = [po.T_INT64] * 6 + [po.T_DOUBLE] * 6 + [po.T_INT32] * 4
DIG_ABI = [abi.T_INT64] * 6 + [abi.T_DOUBLE] * 6 + [abi.T_INT32] * 4
DIG_ID = 15


@pytest.fixture(scope="module")
def digits():
    tb = Tab()
    sizes, cols = make_digits()
    tb.eng = se.Engine(device=0)
    tb.t = tb.eng.table_define("ord_digits", [(dt, False) for dt in DIG_ABI])
    start = 0
    for bi, n in enumerate(sizes):
        sl = slice(start, start + n)
        tb.eng.batch_put(tb.t, 10 + bi, bi, n,
                         [po.encode(dt, po.ENC_UNCOMPRESSED, v[sl])
                          for dt, v in zip(DIG_TYPES, cols)])
        start += n
    n = sum(sizes)
    tb.val = dict(enumerate(cols))
    tb.ok = {c: np.ones(n, dtype=bool) for c in tb.val}
    tb.key = {c: canon(v) for c, v in tb.val.items()}
    tb.words, tb.nan_payload_free = {}, set()
    tb.live = np.ones(n, dtype=bool)
    tb.batch = np.concatenate([np.full(s, bi, dtype=np.int64)
                               for bi, s in enumerate(sizes)])
    tb.ordinal = np.concatenate([np.arange(s, dtype=np.int64) for s in sizes])
    tb.all = np.ones(n, dtype=bool)
    yield tb
    tb.eng.close()


@pytest.mark.parametrize("c", range(15),
                         ids=[f"i64-d{d}" for d in range(6)] +
                             [f"f64-d{d}" for d in range(6)] +
                             [f"i32-d{d}" for d in range(3)])
def test_each_digit_decides(digits, c):
    tb = digits
    # only digit d differs from row to row
    d = c % 6 if c < 12 else c - 12
    raw = tb.val[c].view(np.uint64 if c < 12 else np.uint32).astype(np.uint64)
    assert 256 < len(np.unique(raw)) <= 2048
    digit = np.uint64((2047 << (11 * d)) & (2 ** 64 - 1))
    assert ((raw ^ raw[0]) & ~digit == 0).all()
    for desc in (False, True):
        for k in (100, 1001):
            run(tb, [], tb.all, [c, DIG_ID, ROWID], c, k, f"digit-k{k}", desc)


# ---- ties ----

def test_three_values_over_all_rows(base):
    tb = base
    for desc in (False, True):
        for k in (1, 64, 1000, 8192):
            rs, exp = run(tb, [], tb.all, [T3, ID, ROWID], T3, k, "t3", desc)
            # the tie class is far larger than k and spans tiles and batches
            assert (tb.val[T3][exp] == (2 if desc else 0)).all()
    assert (tb.val[T3] == 0).sum() > 2 * 8192
    assert len(np.unique(tb.batch[tb.val[T3] == 0])) >= 3


def test_all_equal_key_keeps_scan_order(base):
    tb = base
    for desc in (False, True):
        run(tb, [], tb.all, [ID, EQ, ROWID], EQ, 100, "all-equal", desc)
        run(tb, [], tb.all, [ID, ROWID], EQ, 8192, "all-equal", desc)


def test_k_on_and_next_to_a_class_boundary(base):
    tb = base
    hi = 9000
    mask = tb.val[ID] < hi
    n0 = int((tb.val[T3][mask] == 0).sum())
    n1 = int((tb.val[T3][mask] == 1).sum())
    assert n0 > 1 and n1 > 1 and n0 + n1 <= 8192
    preds = [dict(col=ID, hi=hi, hi_strict=True)]
    for k in (n0 + n1, n0 + n1 - 1, n0 + n1 + 1, n0, n0 - 1, n0 + 1):
        rs, exp = run(tb, preds, mask, [T3, ID, ROWID], T3, k, f"edge-{k}")
        assert (tb.val[T3][exp] == 0).sum() == min(k, n0)
        assert (tb.val[T3][exp] == 2).sum() == max(0, k - n0 - n1)


# ---- the general path: nulls, deletes, deltas, RLE, bitset, int8, float ----

GKEY, GPN, GQN, GU, GR, GB, GI8, GFL = range(8)
GSIZES = (2500, 1100, 1030)
PATCH_IN_ROW, PATCH_NULL_ROW, DELETED_MIN_ROW = 5, 129, 1500


@pytest.fixture(scope="module")
def general():
    tb = Tab()
    rng = np.random.default_rng(77)
    U = po.ENC_UNCOMPRESSED
    tb.eng = se.Engine(device=0)
    tb.t = tb.eng.table_define("ord_general", [
        (abi.T_INT32, False), (abi.T_DOUBLE, True), (abi.T_INT32, True),
        (abi.T_INT64, True), (abi.T_INT32, False), (abi.T_BOOL, False),
        (abi.T_INT8, False), (abi.T_FLOAT, False)])
    n0 = GSIZES[0]
    vals = {c: [] for c in range(8)}
    oks = {c: [] for c in range(8)}
    start = 0
    for bi, n in enumerate(GSIZES):
        nulls = bi < 2                    # the last batch is null-free: clean
        key = np.arange(start, start + n, dtype=np.int32)
        pn = rng.standard_normal(n)
        pn[:3] = bits([NAN_A, NAN_B, 0x8000000000000000])
        pn_ok = (rng.random(n) > 0.2) if nulls else np.ones(n, dtype=bool)
        qn = rng.integers(0, 100, n).astype(np.int32)
        qn_ok = (rng.random(n) > 0.1) if nulls else np.ones(n, dtype=bool)
        u = rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64)
        u_ok = np.ones(n, dtype=bool)
        r = np.repeat(rng.integers(-5, 5, n // 7 + 1), 7)[:n].astype(np.int32)
        bo = (rng.random(n) > 0.5).astype(np.uint8)
        i8 = rng.integers(-128, 128, n).astype(np.int8)
        fl = (rng.standard_normal(n) * 100).astype(np.float32)
        fl[:4] = np.array([np.inf, -0.0, np.nan, -np.inf], dtype=np.float32)
        if bi == 0:
            # row 0 is deleted; row 1, the first live row, is neither smallest
            # nor largest of any key (but of the boolean, where it is true)
            bo[1], bo[2], r[:7], i8[1] = 1, 0, 0, 0
            qn[1], qn_ok[1], pn[1], pn_ok[1] = 50, True, 0.25, True
            u[1] = 0
            u[DELETED_MIN_ROW] = -2 ** 62 - 100      # the minimum, deleted
        blobs = [po.encode(po.T_INT32, U, key),
                 po.encode(po.T_DOUBLE, U, pn,
                           pn_ok.astype(np.uint8) if nulls else None),
                 po.encode(po.T_INT32, U, qn,
                           qn_ok.astype(np.uint8) if nulls else None),
                 po.encode(po.T_INT64, U, u),
                 po.encode(po.T_INT32, po.ENC_RLE, r),
                 po.encode(po.T_BOOL, po.ENC_BOOLBITSET if bi == 0 else U, bo),
                 po.encode(po.T_INT8, U, i8.view(np.uint8)),
                 po.encode(po.T_FLOAT, U, fl)]
        if bi == 0:
            tb.deleted = np.array([0, 63, 64, DELETED_MIN_ROW], dtype=np.int32)
            # a patch that moves row 5 below every other value, one to NULL
            d_pos = np.array([PATCH_IN_ROW, PATCH_NULL_ROW, n0 - 1],
                             dtype=np.int32)
            d_val = np.array([-2 ** 62 - 5, 0, 2 ** 53 + 1], dtype=np.int64)
            d_ok = np.array([1, 0, 1], dtype=np.uint8)
            deltas = [(None, None)] * 8
            deltas[GU] = (po.encode_delta(po.T_INT64, U, d_pos, n0, d_val,
                                          d_ok), None)
            tb.unpatched = int(u[PATCH_IN_ROW])
            tb.eng.batch_put(tb.t, 50, 0, -n0, blobs,
                             delete_mask=po.encode_delete(tb.deleted, n0),
                             deltas=deltas)
            u[d_pos] = d_val
            u_ok[PATCH_NULL_ROW] = False
        else:
            tb.eng.batch_put(tb.t, 50 + bi, bi, n, blobs)
        for c, (v, ok) in enumerate([(key, None), (pn, pn_ok), (qn, qn_ok),
                                     (u, u_ok), (r, None), (bo, None),
                                     (i8, None), (fl, None)]):
            ok = np.ones(n, dtype=bool) if ok is None else ok
            vals[c].append(np.where(ok, v, 0).astype(v.dtype))
            oks[c].append(ok)
        start += n
    tb.val = {c: np.concatenate(v) for c, v in vals.items()}
    tb.ok = {c: np.concatenate(v) for c, v in oks.items()}
    tb.key = {c: canon(v) for c, v in tb.val.items()}
    tb.words = {}
    tb.nan_payload_free = {GFL}    # a FLOAT NaN's payload is not pinned here
    n = sum(GSIZES)
    tb.live = np.ones(n, dtype=bool)
    tb.live[tb.deleted] = False
    tb.batch = np.concatenate([np.full(s, bi, dtype=np.int64)
                               for bi, s in enumerate(GSIZES)])
    tb.ordinal = np.concatenate([np.arange(s, dtype=np.int64) for s in GSIZES])
    tb.all = np.ones(n, dtype=bool)
    yield tb
    tb.eng.close()


@pytest.mark.parametrize("desc,nulls_first", [
    (False, None), (True, None), (False, True), (False, False), (True, True),
    (True, False)], ids=["asc", "desc", "asc-first", "asc-last", "desc-first",
                         "desc-last"])
def test_nullable_key(general, desc, nulls_first):
    tb = general
    nulls = tb.live & ~tb.ok[GPN]
    nn = int(nulls.sum())
    assert 100 < nn < 8192
    assert set(np.unique(tb.batch[nulls])) == {0, 1}     # some batches only
    cols = [GPN, GKEY, ROWID, GU]
    for k in (nn - 5, nn, nn + 5, 8192):
        rs, exp = run(tb, [], tb.all, cols, GPN, k, f"nulls-k{k}", desc,
                      nulls_first)
        first = nulls_first if nulls_first is not None else not desc
        got_nulls = int((~tb.ok[GPN][exp]).sum())
        if first:
            assert got_nulls == min(k, nn)
        elif k < 8192:
            assert got_nulls == 0
        else:
            assert got_nulls == nn               # every live row came back
    # NULL against NULL ties keep scan order; NaN sorts above every value
    rs, exp = run(tb, [], tb.all, [GPN], GPN, 8192, "nulls-nan", False, False)
    got, valid = rs.column(0)
    v = got[valid]
    nnan = int(np.isnan(tb.val[GPN][tb.live & tb.ok[GPN]]).sum())
    assert nnan >= 2 and np.isnan(v[-nnan:]).all() and \
        not np.isnan(v[:-nnan]).any()


@pytest.mark.parametrize("c", [GR, GB, GQN, GI8, GFL],
                         ids=["rle", "bitset", "nullable-i32", "i8", "f32"])
def test_general_path_encodings(general, c):
    tb = general
    for desc in (False, True):
        for k in (1, 65, 1000):
            name = f"{c}-k{k}"
            if c == GB and desc and k == 1:
                name = "bitset-desc-k1"     # the first live row is true
            run(tb, [], tb.all, [c, GKEY, ROWID, GPN], c, k, name, desc)


def test_deltas_and_deletes(general):
    tb = general
    rs, exp = run(tb, [], tb.all, [GU, GKEY, ROWID], GU, 10, "delta-top",
                  False, False)
    where = list(zip(tb.batch[exp], tb.ordinal[exp]))
    # the patched row leads; unpatched it would not have made the top 10
    assert where[0] == (0, PATCH_IN_ROW)
    assert tb.unpatched > np.sort(tb.val[GU][tb.live & tb.ok[GU]])[10]
    # the deleted minimum is gone
    assert (0, DELETED_MIN_ROW) not in where
    vals, valid = rs.column(0)
    assert vals[0] == -2 ** 62 - 5 and valid.all()
    # the patch to NULL: first under NULLS FIRST, value bytes zero
    rs, exp = run(tb, [], tb.all, [GU, ROWID], GU, 3, "delta-null", False)
    vals, valid = rs.column(0)
    assert not valid[0] and vals[0] == 0 and valid[1:].all()
    assert (tb.batch[exp[0]], tb.ordinal[exp[0]]) == (0, PATCH_NULL_ROW)
    run(tb, [], tb.all, [GU, ROWID], GU, 1000, "delta-desc", True)
    # under a predicate on another general-path column
    mask = tb.ok[GQN] & (tb.val[GQN] >= 10) & (tb.val[GQN] <= 60)
    run(tb, [dict(col=GQN, lo=10, hi=60)], mask, [GU, GQN, GKEY, ROWID], GU,
        500, "delta-pred", True)


def test_dictionary_string_and_narrowed_keys(base):
    tb = base
    assert tb.eng.narrowed_batches(tb.t, NARROW) == len(SIZES) > 0
    for desc in (False, True):
        for k in (1, 1000):
            run(tb, [], tb.all, [NARROW, ID, ROWID], NARROW, k, "narrow", desc)
    rs, exp = run(tb, [], tb.all, [NARROW], NARROW, 8192, "narrow-zeros")
    got = rs.column(0)[0].view(np.uint64)
    # -0.0 and 0.0 are one key, in scan order, each with its own bytes
    assert (got == np.uint64(0x8000000000000000)).any() and (got == 0).any()
    # bytewise, not by dictionary id: a byte >= 0x80 sorts above "zebra", a
    # value before its extensions
    rs, exp = run(tb, [], tb.all, [STR, ID], STR, 8192, "str-desc", True)
    s = rs.strings(0)
    assert s[0] == b"\xc3\xa9t\xc3\xa9" and s[-1] == b"\x80up"
    rs, exp = run(tb, [], tb.all, [STR], STR, 8192, "str-asc")
    s = rs.strings(0)
    assert s[0] == b"AIR" and s[-1] == b"AIR " and s == sorted(s)


def test_stats_skipping_keeps_table_batch_indices(base):
    tb = base
    lo = int(tb.starts[1])                          # batch 0 lies below
    mask = tb.val[ID] >= lo
    rs, exp = run(tb, [dict(col=ID, lo=lo)], mask, [ROWID, I64, ID], I64, 100,
                  "skip")
    res = rs.result()
    assert res.batches_skipped == 1 and res.batches_seen == len(SIZES)
    gb, _ = rs.rowids()
    assert gb.min() >= 1 and len(np.unique(gb)) > 1
    # two leading and one trailing batch skipped
    lo, hi = int(tb.starts[2]) + 1, int(tb.starts[3])
    mask = (tb.val[ID] >= lo) & (tb.val[ID] <= hi)
    rs, exp = run(tb, [dict(col=ID, lo=lo, hi=hi)], mask, [ROWID, I16], I16,
                  40, "skip-both-ends", True)
    assert rs.result().batches_skipped == 3
    assert set(rs.rowids()[0]) <= {2, 3}


# ---- predicates ----

def test_predicates(base):
    tb = base
    cols = [F64, ID, STR, ROWID]
    run(tb, [], tb.all, cols, F64, 100, "pred-none")
    lo, hi = 16000, 40000
    run(tb, [dict(col=ID, lo=lo, hi=hi)],
        (tb.val[ID] >= lo) & (tb.val[ID] <= hi), cols, F64, 100, "pred-range",
        True)
    inl = list(range(-300, 300, 7)) + [-32768]      # some 70 rows
    run(tb, [dict(col=I16, **{"in": inl})], np.isin(tb.val[I16], inl),
        [I16, F64, ROWID], F64, 5, "pred-in")
    run(tb, [dict(col=STR, eq=b"MAIL")], tb.val[STR] == WORDS.index(b"MAIL"),
        cols, F64, 1000, "pred-str", True)
    # Q6's shape: several predicates at once
    m = (tb.val[ID] >= 1000) & (tb.val[ID] < 45000) & (tb.val[I16] < 0) & \
        (tb.val[NARROW] >= 5 / 128) & (tb.val[NARROW] <= 7 / 128)
    run(tb, [dict(col=ID, lo=1000, hi=45000, hi_strict=True),
             dict(col=I16, hi=0, hi_strict=True),
             dict(col=NARROW, is_double=True, lo=5 / 128, hi=7 / 128)], m,
        [I64, ID, NARROW, ROWID], I64, 100, "pred-q6", True)


def test_nothing_matches(base):
    tb = base
    rs = tb.eng.select(abi.make_plan(
        table=tb.t, preds=[dict(col=NARROW, is_double=True, lo=0.5, hi=0.6)]),
        [ID, F64, ROWID], limit=10, order_by=F64)
    assert rs.count() == 0 and rs.rows_passed() == 0
    for p in range(3):
        vals, valid = rs.column(p)
        assert len(vals) == 0 and len(valid) == 0
    assert rs.kernel_ms() > 0                     # mark + offsets still ran
    assert rs.kernel_ms_parts()[2] == 0


# ---- determinism, the handle ----

def test_same_query_same_bytes_and_unordered_is_untouched(base):
    tb = base
    cols = [F32, F64, STR, ID, ROWID]
    plan = dict(table=tb.t, preds=[dict(col=I16, hi=0, hi_strict=True)])
    a = tb.eng.select(abi.make_plan(**plan), cols, limit=1000, order_by=F32)
    b = tb.eng.select(abi.make_plan(**plan), cols, limit=1000, order_by=F32)
    for p in range(len(cols)):
        (va, oa), (vb, ob) = a.column(p), b.column(p)
        assert same_bytes(va, vb) and same_bytes(oa, ob), p
    mask = tb.val[I16] < 0
    rs = tb.eng.select(abi.make_plan(**plan), cols, limit=1000)
    check(tb, rs, np.flatnonzero(mask)[:1000], cols, "scan-order")
    rs = tb.eng.select(abi.make_plan(**plan), [ID])
    assert rs.count() == int(mask.sum())


def test_handle_contract(base):
    tb = base
    rs, exp = run(tb, [], tb.all, [ID], I32, 5, "handle")
    assert rs.rows_passed() == tb.nrows and rs.count() == 5
    assert rs.used_jit() is False and rs.late_cols() == []
    mark, offsets, order = rs.kernel_ms_parts()
    assert mark > 0 and offsets > 0 and order > 0
    assert abs(rs.kernel_ms() - (mark + offsets + order)) < 1e-3
    res = rs.result()
    assert (res.nrows, res.naggs) == (0, 0) and res.rows_scanned == tb.nrows
    L_ = se.lib()
    sr, dv = abi.SnResult(), abi.SnDecVal()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    U = abi.ERR_UNSUPPORTED
    assert L_.sn_query_result_page(rs._h, 0, C.byref(sr)) == U
    assert L_.sn_query_order_by(rs._h, 0, 0, 0) == U
    assert L_.sn_query_partial_bytes(rs._h) == U
    assert L_.sn_query_partials(rs._h, buf.ctypes.data, 0) == U
    assert L_.sn_query_merge(rs._h, buf.ctypes.data, 8, 1) == U
    assert L_.sn_query_result_dec(rs._h, 0, 0, C.byref(dv)) == U
    assert L_.sn_query_wait(rs._h) == 0
    # fetch ranges work as on any rows handle
    vals, valid = rs.column(0, 2, 3)
    assert same_bytes(vals, tb.val[ID][exp[2:5]]) and valid.all()
