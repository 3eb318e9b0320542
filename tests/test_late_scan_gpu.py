"""Keyless compiled scans that read an aggregate-only f64 column "late": for
the rows that pass the predicates alone (SN_K_F64_LATE).

The table is (f64 low-card, f64 high-card, f64 low-card, int32) under a
Q6-shaped plan.  Every table is queried from two engines in one process, the
default one and one created with SN_LATE=0, and checked against the CPU
oracle.
Quantities are integers, prices multiples of 1/8 below 8,192 and discounts
multiples of 1/128, so every product is a multiple of 2^-10 below 2^10 and
every partial sum of the at most 21,000 rows is exact in f64: the sums do not
depend on the order of addition, and "bit for bit" is a fair demand in all
three directions.

Prices are distinct per row, so a batch of more than 256 rows keeps its f64
body (a narrowed column is scanned from 1-byte codes and is never late);
tables whose batches are smaller get one more batch of 300 rows without
survivors.  The batch statistics carry the columns' domains, not the batch's
own extremes, so the selectivity estimate is the same, about 0.001, whatever
rows a case lets through, and no batch is skipped.

Every positive case asserts through Query.late_cols() that the late path
ran, and that it did not with SN_LATE=0."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se

pytestmark = pytest.mark.gpu

DTYPES = [po.T_DOUBLE, po.T_DOUBLE, po.T_DOUBLE, po.T_INT32]
QTY, EP, DISC, KEY = 0, 1, 2, 3
KEY_LO, KEY_HI, KEY_MAX = 500, 509, 1000
PAD = 300
BIG = (16384 + 2048 + 5,)

SIZES = [(1,), (255,), (257,), (1024,), (1025,), (2047,), (2048,), (2049,),
         (16383,), (16384,), (16385,), BIG, (2500, 17415, 1024)]
PATTERNS = ("none", "row0", "last", "one_per_line", "one_wave_slot", "two_pct")


def survivors(pattern, n):
    s = np.zeros(n, dtype=bool)
    if pattern == "row0":
        s[0] = True
    elif pattern == "last":
        s[n - 1] = True
    elif pattern == "one_per_line":          # 16 doubles = one 128-B line
        i = np.arange(n)
        s[(i % 16) == ((i // 16) * 7) % 16] = True
    elif pattern == "one_wave_slot":         # lanes 64..127 of row slot k = 1
        start = 320 if n > 384 else 64 if n > 128 else 0
        s[start:min(start + 64, n)] = True
    elif pattern == "two_pct":
        s[np.random.default_rng(n).random(n) < 0.02] = True
    return s


def make_columns(surv, seed=7):
    """columns of len(surv) rows in which exactly the rows of `surv` pass
    q6_plan; every predicate rejects some of the others"""
    n = len(surv)
    rng = np.random.default_rng(seed)
    qty = rng.integers(1, 51, n).astype(np.float64)
    ep = ((np.arange(n) * 7919) % 65536) / 8.0           # distinct per row
    disc = rng.integers(0, 11, n) / 128.0
    key = rng.integers(0, KEY_MAX + 1, n).astype(np.int32)
    key[rng.random(n) < 0.3] = KEY_LO + 3
    qty[surv] = rng.integers(1, 24, int(surv.sum()))
    disc[surv] = rng.integers(5, 8, int(surv.sum())) / 128.0
    key[surv] = rng.integers(KEY_LO, KEY_HI + 1, int(surv.sum()))
    passing = ((key >= KEY_LO) & (key <= KEY_HI) & (disc >= 5 / 128) &
               (disc <= 7 / 128) & (qty < 24))
    key[passing & ~surv] = 0
    return [qty, ep, disc, key]


def split(cols, sizes):
    out, at = [], 0
    for n in sizes:
        out.append([c[at:at + n].copy() for c in cols])
        at += n
    return out


def make_batches(sizes, pattern):
    pad = PAD if min(sizes) <= 256 else 0
    surv = np.concatenate([survivors(pattern, sum(sizes)),
                           np.zeros(pad, dtype=bool)])
    return split(make_columns(surv), sizes + ((pad,) if pad else ()))


def q6_plan(aggs=None, extra_preds=(), **kw):
    return dict(
        preds=[dict(col=KEY, lo=KEY_LO, hi=KEY_HI),
               dict(col=DISC, is_double=True, lo=5 / 128, hi=7 / 128),
               dict(col=QTY, is_double=True, hi=24.0, hi_strict=True)] +
        list(extra_preds),
        aggs=aggs or [("sum", [(EP, 0.0, 1.0), (DISC, 0.0, 1.0)]),
                      ("count", [])], **kw)


def blobs_of(cols, ep_valid=None):
    return [po.encode(dt, po.ENC_UNCOMPRESSED, v,
                      ep_valid if c == EP else None)
            for c, (dt, v) in enumerate(zip(DTYPES, cols))]


def stats_of(n, ep_nulls=0):
    return po.encode_stats(DTYPES, n, [1.0, 0.0, 0.0, 0],
                           [50.0, 8192.0, 10 / 128, KEY_MAX],
                           null_counts=[0, ep_nulls, 0, 0])


def new_engine(**env):
    old = {k: os.environ.get(k) for k in ("SN_LATE", "SN_NARROW")}
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


_names = iter(range(1 << 30))


def load(eng, batches, delete_masks=None, ep_valid=None):
    schema = [(abi.T_DOUBLE, False), (abi.T_DOUBLE, ep_valid is not None),
              (abi.T_DOUBLE, False), (abi.T_INT32, False)]
    t = eng.table_define("late_%d" % next(_names), schema)
    for bi, cols in enumerate(batches):
        n = len(cols[0])
        v = None if ep_valid is None else ep_valid[bi]
        eng.batch_put(t, bi, bi, n, blobs_of(cols, v),
                      stats=stats_of(n, 0 if v is None else int((v == 0).sum())),
                      delete_mask=None if delete_masks is None
                      else delete_masks[bi])
    return t


def oracle_rows(batches, plan, delete_masks=None, ep_valid=None, deltas=None):
    ot = po.OracleTable(DTYPES)
    for bi, cols in enumerate(batches):
        n = len(cols[0])
        dl = None if deltas is None else deltas[bi]
        ot.add_batch(-n if dl else n,
                     blobs_of(cols, None if ep_valid is None else ep_valid[bi]),
                     delete_mask=None if delete_masks is None
                     else delete_masks[bi], deltas=dl)
    return po.result_rows(ot.query(po.make_plan(**plan)))


def same(a, b):
    """bit for bit, with every NaN equal to every NaN"""
    if len(a) != len(b):
        return False
    for (ka, va), (kb, vb) in zip(a, b):
        if ka != kb or len(va) != len(vb):
            return False
        for x, y in zip(va, vb):
            if x is None or y is None:
                if x is not y:
                    return False
            elif not (x == y or (x != x and y != y)):
                return False
    return True


def run(eng, t, plan):
    q = eng.query(abi.make_plan(table=t, **plan))
    return q.rows(), q.used_jit(), q.late_cols()


@pytest.fixture(scope="module")
def engines():
    on, off = new_engine(), new_engine(SN_LATE="0")
    yield on, off
    on.close()
    off.close()


def check(engines, batches, plan, late=(EP,), jit=True, **kw):
    """both engines and the oracle agree bit for bit; the default engine read
    exactly `late` late, the SN_LATE=0 engine nothing"""
    on, off = engines
    t_on, t_off = load(on, batches, **kw), load(off, batches, **kw)
    rows_on, jit_on, late_on = run(on, t_on, plan)
    rows_off, jit_off, late_off = run(off, t_off, plan)
    assert jit_on == jit_off == jit
    assert late_on == list(late), late_on
    assert late_off == []
    assert same(rows_on, rows_off), (rows_on, rows_off)
    orows = oracle_rows(batches, plan, **kw)
    assert same(rows_on, orows), (rows_on, orows)
    return rows_on, t_on


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_sizes_and_survivor_patterns(engines, sizes):
    for pattern in PATTERNS:
        batches = make_batches(sizes, pattern)
        rows, _ = check(engines, batches, q6_plan())
        surv = survivors(pattern, sum(sizes))
        assert rows[0][1][1] == float(surv.sum()), pattern


def test_unnarrowed_predicate_columns():
    """SN_NARROW=0: the staged columns of the late kernel are plain f64"""
    engines = new_engine(SN_NARROW="0"), new_engine(SN_NARROW="0", SN_LATE="0")
    try:
        check(engines, make_batches(BIG, "two_pct"), q6_plan())
        check(engines, make_batches((2500, 17415, 1024), "one_per_line"),
              q6_plan())
    finally:
        for e in engines:
            e.close()


def test_delete_mask_removes_every_survivor_of_a_chunk(engines):
    batches = make_batches(BIG, "two_pct")
    surv = survivors("two_pct", BIG[0])
    gone = np.nonzero(surv[2048:4096])[0] + 2048
    assert len(gone) > 10
    # and some rows that do not pass, some of them past the last full chunk
    pos = np.unique(np.concatenate([gone, [0, 5000, BIG[0] - 2]]))
    masks = [po.encode_delete(pos.astype(np.int32), BIG[0])]
    rows, _ = check(engines, batches, q6_plan(), delete_masks=masks)
    left = surv.copy()
    left[pos] = False
    assert rows[0][1][1] == float(left.sum())


def test_minmax_and_repeated_late_factor(engines):
    batches = make_batches((2500, 17415, 1024), "two_pct")
    check(engines, batches, q6_plan(
        aggs=[("min", [(EP, 0.0, 1.0)]), ("max", [(EP, 0.0, 1.0)]),
              ("max", [(EP, 0.0, 1.0), (DISC, 0.0, 1.0)]), ("count", [])]))
    check(engines, batches, q6_plan(
        aggs=[("sum", [(EP, 0.0, 1.0)]), ("sum", [(EP, 0.0, 1.0), (EP, 0.0, 1.0)]),
              ("sum", [(EP, 1.0, -0.5), (DISC, 0.0, 1.0)]), ("count", [])]))


NONFINITE = [np.inf, -np.inf, np.nan]


def test_nonfinite_values_in_rows_that_do_not_pass(engines):
    batches = make_batches(BIG, "two_pct")
    clean = oracle_rows(batches, q6_plan())
    surv = survivors("two_pct", BIG[0])
    dead = np.nonzero(~surv)[0]
    hit = np.unique(np.concatenate([dead[:6], dead[2040:2060], dead[-5:]]))
    deleted = np.nonzero(surv)[0][[0, 7, -1]]
    ep = batches[0][EP]
    for i, r in enumerate(np.concatenate([hit, deleted])):
        ep[r] = NONFINITE[i % 3]
    masks = [po.encode_delete(deleted.astype(np.int32), BIG[0])]
    plain = [c.copy() for c in batches[0]]
    plain[EP] = make_batches(BIG, "two_pct")[0][EP]
    exp = oracle_rows([plain], q6_plan(), delete_masks=masks)
    assert exp[0][1][1] == clean[0][1][1] - 3
    for aggs in (None, [("min", [(EP, 0.0, 1.0)]), ("max", [(EP, 0.0, 1.0)]),
                        ("sum", [(EP, 0.0, 1.0)])]):
        rows, _ = check(engines, batches, q6_plan(aggs=aggs),
                        delete_masks=masks)
        assert same(rows, oracle_rows([plain], q6_plan(aggs=aggs),
                                      delete_masks=masks))


@pytest.mark.parametrize("planted,expect", [
    ((np.inf,), np.inf), ((-np.inf,), -np.inf), ((np.nan,), np.nan),
    ((np.inf, -np.inf), np.nan), ((np.inf, np.inf), np.inf)],
    ids=["pinf", "ninf", "nan", "pinf_ninf", "pinf_pinf"])
def test_nonfinite_values_in_passing_rows(engines, planted, expect):
    """SUM is the IEEE sum of the passing rows"""
    batches = make_batches((2500, 17415, 1024), "two_pct")
    rows_of = np.nonzero(
        survivors("two_pct", 2500 + 17415 + 1024)[2500:2500 + 17415])[0]
    for v, r in zip(planted, (rows_of[3], rows_of[-1])):
        batches[1][EP][r] = v
    rows, _ = check(engines, batches, q6_plan())
    got = rows[0][1][0]
    assert got == expect or (got != got and expect != expect), got


def test_not_engaged(engines):
    on, _ = engines
    batches = make_batches((2500, 17415, 1024), "two_pct")
    # the column is in a predicate too
    check(engines, batches, late=(), plan=q6_plan(
        extra_preds=[dict(col=EP, is_double=True, lo=0.0)]))
    # grouped
    check(engines, batches, late=(), plan=q6_plan(
        group_cols=[KEY], aggs=[("sum", [(EP, 0.0, 1.0)]), ("count", [])]))
    # no predicate at all
    check(engines, batches, late=(), plan=dict(
        aggs=[("sum", [(EP, 0.0, 1.0), (DISC, 0.0, 1.0)]), ("count", [])]))
    # the only predicate covers its column's whole [min, max]: estimate 1.0
    check(engines, batches, late=(), plan=dict(
        preds=[dict(col=KEY, lo=0, hi=KEY_MAX)],
        aggs=[("sum", [(EP, 0.0, 1.0), (DISC, 0.0, 1.0)]), ("count", [])]))
    # half the rows: above the threshold
    check(engines, batches, late=(), plan=dict(
        preds=[dict(col=KEY, lo=0, hi=KEY_MAX // 2)],
        aggs=[("sum", [(EP, 0.0, 1.0), (DISC, 0.0, 1.0)]), ("count", [])]))
    # real nulls in the column: the plan leaves the compiled kernels
    rng = np.random.default_rng(5)
    valid = [(rng.random(len(b[0])) >= 0.25).astype(np.uint8) if bi == 1 else None
             for bi, b in enumerate(batches)]
    check(engines, batches, q6_plan(), late=(), jit=False, ep_valid=valid)


def test_patched_batch_is_not_engaged(engines):
    on, off = engines
    batches = make_batches((2500, 17415, 1024), "two_pct")
    plan = q6_plan()
    _, t_on = check(engines, batches, plan)
    t_off = load(off, batches)
    n = 17415
    pos = np.array([0, 5, 16383, 16384, n - 1], dtype=np.int32)
    vals = np.array([0.5, 1.5, 2.5, 3.5, 4.5])
    d = po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED, pos, n, vals)
    deltas = [(None, None), (d, None), (None, None), (None, None)]
    for eng, t in ((on, t_on), (off, t_off)):
        eng.batch_mutate(t, 1, 1, deltas=deltas, stats=stats_of(n))
    rows_on, jit_on, late_on = run(on, t_on, plan)
    rows_off, _, late_off = run(off, t_off, plan)
    assert jit_on and late_on == [] and late_off == []
    assert same(rows_on, rows_off)
    assert same(rows_on, oracle_rows(batches, plan,
                                     deltas=[None, deltas, None]))
