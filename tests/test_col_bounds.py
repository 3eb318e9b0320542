"""Exact checks of the put-time batch bounds (k_col_minmax).

(a) launches sn_launch_col_minmax directly and compares the two u64 outputs
    with numpy's min/max of the same array, bit for bit;
(b) goes through ingest_columns (the raw path) and asserts that a predicate
    literal sitting exactly on a batch bound never loses a row (the safety
    bar) and that a literal in the gap between two batches skips exactly the
    batches numpy proves empty (the tightness bar)."""
import ctypes as C
import struct

import numpy as np
import pytest

from snappydata_amd import abi, engine as se
from tests import devmem as dm

pytestmark = pytest.mark.gpu

# SN_K_* of engine_internal.h
K_F64, K_I32, K_I64, K_F32, K_I16 = 0, 1, 2, 3, 6
DTYPE = {K_F64: np.float64, K_F32: np.float32, K_I64: np.int64,
         K_I32: np.int32, K_I16: np.int16}
KIND_IDS = {K_F64: "f64", K_F32: "f32", K_I64: "i64", K_I32: "i32",
            K_I16: "i16"}
SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 1024 * 4096 + 1]
TOP = 1 << 63
M64 = (1 << 64) - 1


def ord_f64(o):
    """Python twin of sn_ord_f64_h: order-preserving u64 -> double."""
    b = (o ^ TOP) if (o & TOP) else (~o & M64)
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def is_float(kind):
    return kind in (K_F64, K_F32)


# ------------------------------------------------------------ (a) direct

@pytest.fixture(scope="module")
def launch():
    return dm.launcher("sn_launch_col_minmax",
                       [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p,
                        C.c_void_p, C.c_void_p])


class Runner:
    """One device body buffer of n elements and one guarded (omin, omax)
    pair, reused for every variant of a (kind, n) case."""

    def __init__(self, launch, kind, n):
        self.launch, self.kind, self.n = launch, kind, n
        self.body = self.out = None
        self.body = dm.malloc(n * np.dtype(DTYPE[kind]).itemsize)
        self.out = dm.guarded(16)

    def run(self, arr):
        assert arr.dtype == DTYPE[self.kind] and len(arr) == self.n
        dm.to_device(self.body, np.ascontiguousarray(arr))
        self.out.write(b"\xff" * 8 + b"\x00" * 8)      # the engine's seeds
        rc = self.launch(self.body, self.n, self.kind, self.out.ptr,
                         self.out.ptr + 8, None)
        dm.sync()
        assert rc == 0
        lo, hi = struct.unpack("<QQ", self.out.read())
        self.out.check_bands()
        return lo, hi

    def close(self):
        if self.out is not None:
            self.out.free()
        dm.free(self.body)


def check(r, arr, what):
    """Bounds of arr (which holds at least one non-NaN) against numpy."""
    lo, hi = r.run(arr)
    if is_float(r.kind):
        wide = arr.astype(np.float64)                  # f32 widens exactly
        exp_lo, exp_hi = float(np.nanmin(wide)), float(np.nanmax(wide))
        got_lo, got_hi = ord_f64(lo), ord_f64(hi)
        print(what, "lo", got_lo, exp_lo, "hi", got_hi, exp_hi)
        assert got_lo == exp_lo, (what, "lo", got_lo, exp_lo)
        assert got_hi == exp_hi, (what, "hi", got_hi, exp_hi)
    else:
        exp_lo = (int(arr.min()) & M64) ^ TOP
        exp_hi = (int(arr.max()) & M64) ^ TOP
        print(what, "lo", hex(lo), hex(exp_lo), "hi", hex(hi), hex(exp_hi))
        assert lo == exp_lo, (what, "lo", hex(lo), hex(exp_lo))
        assert hi == exp_hi, (what, "hi", hex(hi), hex(exp_hi))


def base_values(kind, n, rng):
    """Mid-range random values, well inside every type's limits."""
    dt = DTYPE[kind]
    if is_float(kind):
        return (rng.random(n) * 2000.0 - 1000.0).astype(dt)
    return rng.integers(-1000, 1001, n).astype(dt)


def limit_pairs(kind):
    """(min, max) pairs at the type's own limits."""
    if kind == K_F64:
        fi = np.finfo(np.float64)
        tiny = np.float64(5e-324)
        return [(fi.min, fi.max), (-np.inf, np.inf), (-tiny, tiny),
                (tiny, 3 * tiny), (-3 * tiny, -tiny)]
    if kind == K_F32:
        fi = np.finfo(np.float32)
        tiny = np.float32(1e-45)                       # smallest f32 denormal
        assert tiny > 0 and tiny == np.float32(2.0) ** -149
        return [(fi.min, fi.max), (np.float32(-np.inf), np.float32(np.inf)),
                (-tiny, tiny), (tiny, np.float32(3) * tiny),
                (np.float32(-3) * tiny, -tiny)]
    ii = np.iinfo(DTYPE[kind])
    return [(ii.min, ii.max)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", [K_F64, K_F32, K_I64, K_I32, K_I16],
                         ids=lambda k: KIND_IDS[k])
def test_direct_bounds(launch, kind, n):
    rng = np.random.default_rng(7000 + 31 * kind + n % 9973)
    dt = DTYPE[kind]
    big = dt(30000)                       # beyond every base value, fits i16
    r = Runner(launch, kind, n)
    try:
        # extremes planted at index 0 and at index n-1
        a = base_values(kind, n, rng)
        a[0], a[n - 1] = -big, big
        check(r, a, "min@0 max@last")
        a = base_values(kind, n, rng)
        a[0], a[n - 1] = big, -big
        check(r, a, "max@0 min@last")
        # the extremum only in the last element (a ragged block's last row)
        a = base_values(kind, n, rng)
        a[n - 1] = big
        check(r, a, "max only@last")
        a = base_values(kind, n, rng)
        a[n - 1] = -big
        check(r, a, "min only@last")

        # the type's own limits: at random inner positions, then at the ends
        for mn, mx in limit_pairs(kind):
            if is_float(kind) and abs(float(mx)) < 1.0:    # denormals
                a = np.full(n, (dt(mn) + dt(mx)) / dt(2) if mn < 0 < mx
                            else dt(mn) + (dt(mx) - dt(mn)) / dt(2), dtype=dt)
            else:
                a = base_values(kind, n, rng)
            i, j = (int(x) for x in rng.integers(0, n, 2))
            a[i] = mn
            a[j] = mx
            check(r, a, f"limits {mn!r},{mx!r} inner")
            a[0], a[n - 1] = mx, mn
            check(r, a, f"limits {mn!r},{mx!r} ends")

        # all equal
        check(r, np.full(n, dt(-7), dtype=dt), "all equal")

        if is_float(kind):
            # -0.0 / +0.0 mix: both bounds compare equal to 0.0
            a = np.where(rng.random(n) < 0.5, dt(-0.0), dt(0.0)).astype(dt)
            a[n - 1] = dt(-0.0)
            lo, hi = r.run(a)
            assert ord_f64(lo) == 0.0 and ord_f64(hi) == 0.0
            # NaN at ~10% of positions, index 0 and n-1 included
            if n >= 3:
                a = base_values(kind, n, rng)
                a[rng.random(n) < 0.1] = np.nan
                a[0] = a[n - 1] = np.nan
                a[n // 2] = big                        # at least one value
                assert np.isnan(a).any() and not np.isnan(a).all()
                check(r, a, "10% NaN")
                a[n // 2] = -big
                check(r, a, "10% NaN, min")
    finally:
        r.close()


@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("kind", [K_F64, K_F32], ids=lambda k: KIND_IDS[k])
def test_direct_all_nan(launch, kind, n):
    """All-NaN column: the launch succeeds and no finite value lies outside
    [lo, hi] (vacuously true: there is none); the encodings are not pinned."""
    r = Runner(launch, kind, n)
    try:
        a = np.full(n, np.nan, dtype=DTYPE[kind])
        lo, hi = (ord_f64(x) for x in r.run(a))
        finite = a[np.isfinite(a)]
        assert not ((finite < lo) | (finite > hi)).any()
    finally:
        r.close()


# ------------------------------------------------------- (b) engine level

NB, ROWS = 6, 300
ENGINE_TYPES = {
    "double": (abi.T_DOUBLE, np.float64, True),
    "float": (abi.T_FLOAT, np.float32, True),
    "int64": (abi.T_INT64, np.int64, False),
    "int32": (abi.T_INT32, np.int32, False),
    "int16": (abi.T_INT16, np.int16, False),
}


@pytest.fixture
def eng():
    e = se.Engine(device=0)
    yield e
    e.close()


def ingest_batches(eng, name, sn_type, batches):
    t = eng.table_define(name, [(sn_type, False)])
    for bi, b in enumerate(batches):
        assert eng.ingest_columns(t, [{"data": np.ascontiguousarray(b)}],
                                  len(b), batch_rows=len(b),
                                  first_bucket=bi) == len(b)
    return t


def disjoint_batches(np_type, base, span, rng):
    """NB batches of ROWS rows; batch i lies in [base + i*span,
    base + i*span + span/2], its minimum only at row 0 and its maximum only
    at row ROWS-1.  Every value is an integer small enough for f32."""
    out = []
    for i in range(NB):
        lo = base + i * span
        hi = lo + span // 2
        v = rng.integers(lo + 1, hi, ROWS)
        v[0], v[ROWS - 1] = lo, hi
        out.append(v.astype(np_type))
        assert int(out[-1][0]) == lo and int(out[-1][-1]) == hi
    return out


def np_mask(v, side, lit, strict):
    if side == "lo":
        return v > lit if strict else v >= lit
    return v < lit if strict else v <= lit


def check_predicates(eng, t, batches, literals, gap_literals, is_double):
    for lit in list(literals) + list(gap_literals):
        for side in ("lo", "hi"):
            for strict in (False, True):
                pred = {"col": 0, side: lit, side + "_strict": strict}
                if is_double:
                    pred["is_double"] = True
                q = eng.query(abi.make_plan(table=t, preds=[pred],
                                            aggs=[("count", [])]))
                rows = q.rows()
                res = q.result()
                got = int(rows[0][1][0] or 0) if rows else 0
                per_batch = [int(np_mask(b, side, lit, strict).sum())
                             for b in batches]
                empty = sum(1 for c in per_batch if c == 0)
                what = (lit, side, strict, got, sum(per_batch),
                        int(res.batches_skipped), empty)
                print(what)
                assert got == sum(per_batch), what          # safety
                assert res.batches_seen == len(batches), what
                assert res.batches_skipped <= empty, what
                if lit in gap_literals:
                    assert res.batches_skipped == empty, what   # tightness


@pytest.mark.parametrize("tname", list(ENGINE_TYPES))
def test_engine_literal_on_batch_bounds(eng, tname):
    sn_type, np_type, is_double = ENGINE_TYPES[tname]
    rng = np.random.default_rng(500 + len(tname))
    batches = disjoint_batches(np_type, -3000, 1000, rng)
    t = ingest_batches(eng, "bnd_" + tname, sn_type, batches)
    conv = float if is_double else int
    literals = []
    for i in (0, 2, NB - 1):
        literals += [conv(batches[i][0]), conv(batches[i][-1])]
    # strictly between batch 2's maximum and batch 3's minimum
    gap = [conv(int(batches[2][-1]) + 100)]
    check_predicates(eng, t, batches, literals, gap, is_double)


def test_engine_int64_bounds_beyond_f64(eng):
    """Values around +-2^62 that differ only below the f64 mantissa: a pass
    of the bounds (or the literal) through f64 loses a row here."""
    rng = np.random.default_rng(62)
    batches = []
    for i in range(NB):
        centre = (-(1 << 62) if i < NB // 2 else (1 << 62)) + (i % 3) * 2048
        lo, hi = centre + 1, centre + 201
        v = rng.integers(lo + 1, hi, ROWS)
        v[0], v[ROWS - 1] = lo, hi
        batches.append(v.astype(np.int64))
        assert float(lo) == float(hi)          # indistinguishable as doubles
    t = ingest_batches(eng, "bnd_i64_big", abi.T_INT64, batches)
    literals = []
    for b in batches:
        literals += [int(b[0]), int(b[-1])]
    gap = [int(batches[0][-1]) + 100, 0]
    check_predicates(eng, t, batches, literals, gap, False)


def test_engine_double_batch_with_nan(eng):
    rng = np.random.default_rng(77)
    batches = disjoint_batches(np.float64, -3000, 1000, rng)
    nan_rows = [0, 7, 150, ROWS - 1]           # the extrema rows included
    batches[2][nan_rows] = np.nan
    batches[2][1], batches[2][ROWS - 2] = -1000.0, -500.0
    t = ingest_batches(eng, "bnd_nan", abi.T_DOUBLE, batches)
    rows = eng.query(abi.make_plan(table=t, aggs=[("count", [])])).rows()
    assert rows[0][1][0] == float(NB * ROWS)
    literals = [-1000.0, -500.0, float(batches[1][-1]), float(batches[3][0])]
    with np.errstate(invalid="ignore"):
        check_predicates(eng, t, batches, literals, [-400.0], True)
