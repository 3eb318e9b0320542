"""The image-free ("direct") keyless compiled scan and the residency-sized
grid.

Tables, plans and survivor patterns are those of tests/test_late_scan_gpu.py,
whose data make every partial sum exact in f64, so results are compared bit
for bit whatever the order of addition.  Every table is queried from a
default engine and from one created with SN_DIRECT=0 (the late kernel with
the LDS image), and checked against the CPU oracle.  Every positive case
asserts through Query.direct() that the direct kernel ran on the default
engine and did not on the other.

The dictionary cases replace the discount column: multiples of 1/1024 of
magnitude at most 1, so products stay multiples of 2^-13 below 2^13 and the
sums stay exact.  Their batch statistics say [-1, 1] for that column, so no
bound used here lets a batch be skipped."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi
from snappydata_amd import engine as se
from tests import test_late_scan_gpu as L

pytestmark = pytest.mark.gpu

QTY, EP, DISC, KEY = L.QTY, L.EP, L.DISC, L.KEY
BIG = L.BIG
THREE = (2500, 17415, 1024)
SIZES = [(1,), (255,), (257,), (1024,), (1025,), (16383,), (16384,), (16385,),
         BIG, THREE]
SWITCHES = ("SN_LATE", "SN_NARROW", "SN_DIRECT", "SN_GRID_RESIDENT")


def new_engine(**env):
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return se.Engine(device=0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    on, off = new_engine(), new_engine(SN_DIRECT="0")
    yield on, off
    on.close()
    off.close()


def load(eng, batches, delete_masks=None, disc_bounds=(0.0, 10 / 128)):
    t = eng.table_define("direct_%d" % next(L._names),
                         [(abi.T_DOUBLE, False)] * 3 + [(abi.T_INT32, False)])
    for bi, cols in enumerate(batches):
        n = len(cols[0])
        stats = po.encode_stats(L.DTYPES, n, [1.0, 0.0, disc_bounds[0], 0],
                                [50.0, 8192.0, disc_bounds[1], L.KEY_MAX],
                                null_counts=[0, 0, 0, 0])
        eng.batch_put(t, bi, bi, n, L.blobs_of(cols), stats=stats,
                      delete_mask=None if delete_masks is None
                      else delete_masks[bi])
    return t


def check(engines, batches, plan, direct=1, late=(EP,), delete_masks=None,
          **kw):
    """both engines and the oracle agree bit for bit; the default engine ran
    the direct kernel iff `direct`, the other engine never"""
    got = []
    for eng in engines:
        t = load(eng, batches, delete_masks=delete_masks, **kw)
        q = eng.query(abi.make_plan(table=t, **plan))
        got.append((q.rows(), q.used_jit(), q.late_cols(), q.direct()))
    (rows_on, jit_on, late_on, direct_on), (rows_off, jit_off, late_off,
                                             direct_off) = got
    assert jit_on and jit_off
    assert late_on == late_off == list(late), (late_on, late_off)
    assert direct_on == direct and direct_off == 0, (direct_on, direct_off)
    assert L.same(rows_on, rows_off), (rows_on, rows_off)
    orows = L.oracle_rows(batches, plan, delete_masks=delete_masks)
    assert L.same(rows_on, orows), (rows_on, orows)
    return rows_on


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_sizes_and_survivor_patterns(engines, sizes):
    for pattern in L.PATTERNS:
        rows = check(engines, L.make_batches(sizes, pattern), L.q6_plan())
        surv = L.survivors(pattern, sum(sizes))
        assert rows[0][1][1] == float(surv.sum()), pattern


# ---- dictionaries of a narrowed predicate column -------------------------

def disc_plan(lo, hi):
    plan = L.q6_plan()
    plan["preds"][1] = dict(col=DISC, is_double=True, lo=lo, hi=hi)
    return plan


def disc_batches(pool, must=()):
    """THREE batches whose discount column draws from `pool`, every value of
    it present in every batch; rows whose other predicates pass carry the
    values of `must` among others"""
    n = sum(THREE)
    cols = L.make_columns(L.survivors("two_pct", n))
    rng = np.random.default_rng(11)
    disc = rng.choice(np.asarray(pool, dtype=np.float64), n)
    at = 0
    for size in THREE:
        disc[at:at + len(pool)] = pool
        others = np.nonzero((cols[KEY][at:at + size] >= L.KEY_LO) &
                            (cols[KEY][at:at + size] <= L.KEY_HI) &
                            (cols[QTY][at:at + size] < 24))[0] + at
        others = others[others >= at + len(pool)]
        assert len(others) >= len(must)
        disc[others[:len(must)]] = must
        at += size
    cols[DISC] = disc
    return L.split(cols, THREE), cols


def passing(cols, lo, hi):
    with np.errstate(invalid="ignore"):
        return ((cols[KEY] >= L.KEY_LO) & (cols[KEY] <= L.KEY_HI) &
                (cols[QTY] < 24) & (cols[DISC] >= lo) & (cols[DISC] <= hi))


def test_dictionary_of_256_values_negative_half_included(engines):
    """128 positive and 128 negative values.  By bit pattern the positives
    come first, ascending, then the negatives by falling value: the bounds
    keep codes 0..64 and 128..255 and drop 65..127, so the passing codes are
    no interval of codes.  Survivors carry codes 0, 63, 64 and 255."""
    pos = np.arange(1, 129) / 1024.0
    pool = np.concatenate([pos, -pos])
    lo, hi = -128 / 1024.0, 65 / 1024.0
    must = [pos[0], pos[63], pos[64], -pos[127], pos[65], pos[127]]
    batches, cols = disc_batches(pool, must)
    for b in batches:
        assert len(np.unique(b[DISC])) == 256
    rows = check(engines, batches, disc_plan(lo, hi), disc_bounds=(-1.0, 1.0))
    ok = passing(cols, lo, hi)
    for v in must[:4]:
        assert (ok & (cols[DISC] == v)).any()
    for v in must[4:]:
        assert not (ok & (cols[DISC] == v)).any()
    assert rows[0][1][1] == float(ok.sum())


def test_dictionary_with_negatives_signed_zeros_and_nan(engines):
    """NaN fails every range predicate (the pinned deviation); -0.0 and +0.0
    are entries of their own and both satisfy lo = 0.0"""
    pool = [-0.5, -1 / 1024, -0.0, 0.0, 1 / 1024, 0.25, np.nan]
    batches, cols = disc_batches(pool, pool)
    for lo, hi in ((0.0, 0.25), (-0.5, -0.0), (-1.0, 1.0)):
        rows = check(engines, batches, disc_plan(lo, hi),
                     disc_bounds=(-1.0, 1.0))
        ok = passing(cols, lo, hi)
        assert ok.any() and not (ok & np.isnan(cols[DISC])).any()
        assert rows[0][1][1] == float(ok.sum())


def test_bounds_that_no_entry_or_every_entry_satisfies(engines):
    pool = np.arange(-20, 21) / 1024.0
    batches, cols = disc_batches(pool)
    rows = check(engines, batches, disc_plan(0.3, 0.4),
                 disc_bounds=(-1.0, 1.0))
    # no row passes: the oracle's NULL sum (Spark semantics) and a zero count
    assert rows[0][1][1] == 0.0
    rows = check(engines, batches, disc_plan(-1.0, 1.0),
                 disc_bounds=(-1.0, 1.0))
    assert rows[0][1][1] == float(passing(cols, -1.0, 1.0).sum())


# ---- deletes and non-finite values ---------------------------------------

def test_delete_mask_removes_every_survivor_of_a_1024_row_span(engines):
    batches = L.make_batches(BIG, "two_pct")
    surv = L.survivors("two_pct", BIG[0])
    gone = np.nonzero(surv[2048:3072])[0] + 2048
    assert len(gone) > 5
    pos = np.unique(np.concatenate([gone, [0, 5000, BIG[0] - 2]]))
    masks = [po.encode_delete(pos.astype(np.int32), BIG[0])]
    rows = check(engines, batches, L.q6_plan(), delete_masks=masks)
    left = surv.copy()
    left[pos] = False
    assert rows[0][1][1] == float(left.sum())


def test_nonfinite_values_in_rows_that_do_not_pass(engines):
    batches = L.make_batches(BIG, "two_pct")
    surv = L.survivors("two_pct", BIG[0])
    dead = np.nonzero(~surv)[0]
    hit = np.unique(np.concatenate([dead[:6], dead[1020:1030], dead[-5:]]))
    deleted = np.nonzero(surv)[0][[0, 7, -1]]
    for i, r in enumerate(np.concatenate([hit, deleted])):
        batches[0][EP][r] = L.NONFINITE[i % 3]
    masks = [po.encode_delete(deleted.astype(np.int32), BIG[0])]
    plain = [c.copy() for c in batches[0]]
    plain[EP] = L.make_batches(BIG, "two_pct")[0][EP]
    rows = check(engines, batches, L.q6_plan(), delete_masks=masks)
    assert L.same(rows, L.oracle_rows([plain], L.q6_plan(),
                                      delete_masks=masks))
    assert rows[0][1][1] == float(surv.sum()) - 3


@pytest.mark.parametrize("planted,expect", [
    ((np.inf,), np.inf), ((-np.inf,), -np.inf), ((np.nan,), np.nan),
    ((np.inf, -np.inf), np.nan), ((np.inf, np.inf), np.inf)],
    ids=["pinf", "ninf", "nan", "pinf_ninf", "pinf_pinf"])
def test_nonfinite_values_in_passing_rows(engines, planted, expect):
    """SUM is the IEEE sum of the passing rows"""
    batches = L.make_batches(THREE, "two_pct")
    rows_of = np.nonzero(L.survivors("two_pct", sum(THREE))[2500:2500 + 17415])[0]
    for v, r in zip(planted, (rows_of[3], rows_of[-1])):
        batches[1][EP][r] = v
    got = check(engines, batches, L.q6_plan())[0][1][0]
    assert got == expect or (got != got and expect != expect), got


# ---- plans the direct kernel does not take -------------------------------

def test_not_engaged(engines):
    batches = L.make_batches(THREE, "two_pct")
    # MIN/MAX aggregates keep the late kernel of the grouped layout
    check(engines, batches, direct=0, plan=L.q6_plan(
        aggs=[("min", [(EP, 0.0, 1.0)]), ("max", [(EP, 0.0, 1.0)]),
              ("count", [])]))
    # an IN-list next to the range predicates
    check(engines, batches, direct=0, plan=L.q6_plan(
        extra_preds=[dict(col=KEY, **{"in": [L.KEY_LO, L.KEY_LO + 3,
                                             L.KEY_HI]})]))
    # an f64 predicate column with more than 256 values keeps its f64 body
    wide = [[c.copy() for c in b] for b in batches]
    for b in wide:
        n = len(b[QTY])
        b[QTY] = b[QTY] + (np.arange(n) % 1024) / 2048.0 * \
            ((b[QTY] >= 24) & (b[QTY] < 50))
        assert len(np.unique(b[QTY])) > 256
    check(engines, wide, L.q6_plan(), direct=0)


# ---- the residency-sized grid --------------------------------------------

def test_more_tiles_than_any_residency():
    """3,001 tiles: 3,000 batches of 1 to 5 rows and one of 300 rows with
    distinct prices, which keeps the price column un-narrowed under the
    uniform-kind rule.  More blocks than a 256-CU device holds of any kernel,
    so the default engine's grid differs from that of SN_GRID_RESIDENT=0."""
    sizes = tuple(1 + (i * 7) % 5 for i in range(3000)) + (300,)
    surv = L.survivors("two_pct", sum(sizes))
    surv[:4] = True
    batches = L.split(L.make_columns(surv), sizes)
    plan = L.q6_plan()
    orows = L.oracle_rows(batches, plan)
    assert orows[0][1][1] == float(surv.sum())
    for env in ({}, {"SN_GRID_RESIDENT": "0"}):
        eng = new_engine(**env)
        try:
            q = eng.query(abi.make_plan(table=load(eng, batches), **plan))
            rows = q.rows()
            assert q.used_jit() and q.late_cols() == [EP] and q.direct() == 1
            assert L.same(rows, orows), (env, rows, orows)
        finally:
            eng.close()
