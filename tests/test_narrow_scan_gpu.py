"""Scans over narrowed f64 columns (1-byte codes + per-batch value
dictionary, built on device at put) against the same data scanned from the
f64 bodies and against the CPU oracle.

The table is (f64 low-card, f64 high-card, f64 low-card, int32) in three
batches of 2,500, 17,415 and 1,024 rows: a short tail chunk; a 16 K tile
boundary followed by one staged chunk and a 7-row tail; one exact chunk.
Narrowing does not change the chunk geometry, so the narrowed results must
equal those of an engine created with SN_NARROW=0 bit for bit; both match the
oracle under the engine tests' relative tolerance.

Every value is a small dyadic rational (quantities are integers, prices
multiples of 1/4, discounts multiples of 1/128), so every product and every
partial sum is exact in f64 and the sums do not depend on the order of
addition.  That is what makes "bit for bit" a property of the decoded values
alone: the scan kernels fold their four per-wave partials into the block
accumulator with LDS atomics in arrival order, so with inexact sums two runs
of one and the same kernel may already differ in the last bit, and a 1-ulp
difference would say nothing about the dictionary.  A wrong decoded double
still moves an exact sum."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se

pytestmark = pytest.mark.gpu

REL = 1e-6                      # tests/test_engine_gpu.py's tolerance
SIZES = (2500, 17415, 1024)
DTYPES = [po.T_DOUBLE, po.T_DOUBLE, po.T_DOUBLE, po.T_INT32]
QTY, EP, DISC, KEY = 0, 1, 2, 3


def make_batches(seed, qty_distinct=(50, 50, 50)):
    """per batch: [qty, ep, disc, key] arrays"""
    rng = np.random.default_rng(seed)
    out = []
    for n, nq in zip(SIZES, qty_distinct):
        qty = rng.integers(1, nq + 1, n).astype(np.float64)
        qty[:nq] = np.arange(1, nq + 1)          # every value present
        ep = rng.integers(0, 400_000, n) / 4.0
        disc = rng.integers(0, 11, n) / 128.0
        key = rng.integers(0, 6, n).astype(np.int32)
        out.append([qty, ep, disc, key])
    return out


def blobs_of(cols, extra=None):
    b = [po.encode(dt, po.ENC_UNCOMPRESSED, v) for dt, v in zip(DTYPES, cols)]
    if extra is not None:
        vals, valid = extra
        b.append(po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, vals, valid))
    return b


def stats_of(cols, extra=None):
    dts, lo, hi, nulls = list(DTYPES), [], [], []
    for dt, v in zip(DTYPES, cols):
        lo.append(v.min()); hi.append(v.max()); nulls.append(0)
    if extra is not None:
        vals, valid = extra
        live = vals if valid is None else vals[valid.astype(bool)]
        dts.append(po.T_DOUBLE)
        lo.append(live.min()); hi.append(live.max())
        nulls.append(0 if valid is None else int((valid == 0).sum()))
    return po.encode_stats(dts, len(cols[0]), lo, hi, null_counts=nulls)


def q6_plan(**kw):
    return dict(
        preds=[dict(col=KEY, lo=1, hi=4),
               dict(col=DISC, is_double=True, lo=5 / 128, hi=7 / 128),
               dict(col=QTY, is_double=True, hi=24.0, hi_strict=True)],
        aggs=[("sum", [(EP, 0.0, 1.0), (DISC, 0.0, 1.0)]), ("count", [])], **kw)


def grouped_plan(**kw):
    return dict(
        group_cols=[KEY],
        aggs=[("sum", [(QTY, 0.0, 1.0)]), ("sum", [(EP, 0.0, 1.0)]),
              ("sum", [(EP, 0.0, 1.0), (DISC, 1.0, -1.0)]), ("count", [])], **kw)


PLANS = {"q6": (q6_plan, (1,)), "grouped": (grouped_plan, (3,))}


def new_engine(narrow):
    old = os.environ.get("SN_NARROW")
    if narrow:
        os.environ.pop("SN_NARROW", None)
    else:
        os.environ["SN_NARROW"] = "0"
    try:
        return se.Engine(device=0)
    finally:
        if old is None:
            os.environ.pop("SN_NARROW", None)
        else:
            os.environ["SN_NARROW"] = old


def load(eng, name, batches, delete_masks=None, extras=None):
    ncols = 4 if extras is None else 5
    schema = [(abi.T_DOUBLE, False)] * 3 + [(abi.T_INT32, False)]
    if extras is not None:
        schema.append((abi.T_DOUBLE, True))
    assert len(schema) == ncols
    t = eng.table_define(name, schema)
    for bi, cols in enumerate(batches):
        ex = None if extras is None else extras[bi]
        dm = None if delete_masks is None else delete_masks[bi]
        eng.batch_put(t, bi, bi, len(cols[0]), blobs_of(cols, ex),
                      stats=stats_of(cols, ex), delete_mask=dm)
    return t


def oracle_rows(batches, plan_fn, delete_masks=None, deltas=None, extras=None):
    dts = DTYPES + ([po.T_DOUBLE] if extras is not None else [])
    ot = po.OracleTable(dts)
    for bi, cols in enumerate(batches):
        ex = None if extras is None else extras[bi]
        dl = None if deltas is None else deltas[bi]
        n = len(cols[0])
        ot.add_batch(-n if dl else n, blobs_of(cols, ex),
                     delete_mask=None if delete_masks is None else delete_masks[bi],
                     deltas=dl)
    return po.result_rows(ot.query(po.make_plan(**plan_fn())))


def assert_matches_oracle(grows, orows, count_aggs):
    assert len(grows) == len(orows), (grows, orows)
    for (gk, gv), (ok, ov) in zip(grows, orows):
        assert gk == ok
        for a, (g, o) in enumerate(zip(gv, ov)):
            if a in count_aggs:
                assert g == o, (a, g, o)
            else:
                assert abs(g - o) <= REL * max(1.0, abs(o)), (a, g, o)


def run(eng, t, plan_fn):
    q = eng.query(abi.make_plan(table=t, **plan_fn()))
    return q.rows(), q.used_jit()


@pytest.fixture(scope="module")
def engines():
    on, off = new_engine(True), new_engine(False)
    yield on, off
    on.close()
    off.close()


@pytest.fixture(scope="module")
def base():
    return make_batches(20)


@pytest.fixture(scope="module")
def base_oracle(base):
    return {k: oracle_rows(base, fn) for k, (fn, _) in PLANS.items()}


@pytest.fixture(scope="module")
def base_tables(engines, base):
    on, off = engines
    return load(on, "nw_base", base), load(off, "nw_base", base)


def test_engagement(engines, base_tables):
    on, off = engines
    t_on, t_off = base_tables
    assert on.narrowed_batches(t_on, QTY) == 3
    assert on.narrowed_batches(t_on, DISC) == 3
    assert on.narrowed_batches(t_on, EP) == 0
    for c in (QTY, EP, DISC):
        assert off.narrowed_batches(t_off, c) == 0
    for fn, _ in PLANS.values():
        assert run(on, t_on, fn)[1]
        assert run(off, t_off, fn)[1]


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_equal_to_unnarrowed_scan_and_oracle(engines, base_tables,
                                             base_oracle, plan):
    on, off = engines
    t_on, t_off = base_tables
    fn, counts = PLANS[plan]
    rows_on, jit_on = run(on, t_on, fn)
    rows_off, jit_off = run(off, t_off, fn)
    assert jit_on and jit_off
    assert rows_on == rows_off                   # bit for bit
    assert_matches_oracle(rows_on, base_oracle[plan], counts)
    assert_matches_oracle(rows_off, base_oracle[plan], counts)


def test_raw_put_path_narrows_too(engines):
    on, _ = engines
    n = 5000
    rng = np.random.default_rng(21)
    lo = rng.integers(0, 40, n) / 8.0
    hi = rng.random(n)
    t = on.table_define("nw_raw", [(abi.T_DOUBLE, False), (abi.T_DOUBLE, False)])
    on.ingest_columns(t, [{"data": lo}, {"data": hi}], n, batch_rows=2048)
    assert on.num_batches(t) == 3
    assert on.narrowed_batches(t, 0) == 3
    assert on.narrowed_batches(t, 1) == 0
    q = on.query(abi.make_plan(
        table=t, preds=[dict(col=0, is_double=True, lo=1.0, hi=3.0)],
        aggs=[("sum", [(0, 0.0, 1.0), (1, 0.0, 1.0)]), ("count", [])]))
    rows = q.rows()
    m = (lo >= 1.0) & (lo <= 3.0)
    assert rows[0][1][1] == float(m.sum())
    exp = float((lo[m] * hi[m]).sum())
    assert abs(rows[0][1][0] - exp) <= REL * max(1.0, abs(exp))


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_mixed_kinds_fall_back_to_the_body(engines, plan):
    """300 distinct values in one batch: the column scans as F64 everywhere"""
    on, off = engines
    batches = make_batches(22, qty_distinct=(50, 300, 50))
    t_on = load(on, "nw_mixed_" + plan, batches)
    t_off = load(off, "nw_mixed_" + plan, batches)
    assert on.narrowed_batches(t_on, QTY) == 2
    assert on.narrowed_batches(t_on, DISC) == 3
    fn, counts = PLANS[plan]
    rows_on, jit_on = run(on, t_on, fn)
    rows_off, _ = run(off, t_off, fn)
    assert jit_on
    assert rows_on == rows_off
    assert_matches_oracle(rows_on, oracle_rows(batches, fn), counts)


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_deletes(engines, base, plan):
    on, off = engines
    rng = np.random.default_rng(23)
    masks = [None,
             po.encode_delete(np.unique(rng.integers(0, SIZES[1], 900))
                              .astype(np.int32), SIZES[1]),
             None]
    t_on = load(on, "nw_del_" + plan, base, delete_masks=masks)
    t_off = load(off, "nw_del_" + plan, base, delete_masks=masks)
    assert on.narrowed_batches(t_on, QTY) == 3
    fn, counts = PLANS[plan]
    rows_on, jit_on = run(on, t_on, fn)
    rows_off, _ = run(off, t_off, fn)
    assert jit_on                                 # the compiled has_del shape
    assert rows_on == rows_off
    assert_matches_oracle(rows_on, oracle_rows(base, fn, delete_masks=masks),
                          counts)


def test_mutation_rebuilds_then_drops_the_sidecar(engines, base):
    on, _ = engines
    t = load(on, "nw_mut", base)
    fn, counts = PLANS["q6"]
    run(on, t, fn)                  # a cached scan set the mutation must drop
    assert on.narrowed_batches(t, QTY) == 3
    n = SIZES[1]

    def mutate(pos, vals):
        order = np.argsort(pos)
        pos, vals = pos[order], vals[order]
        d = po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED,
                            pos.astype(np.int32), n, vals)
        deltas = [(d, None), (None, None), (None, None), (None, None)]
        cols = [c.copy() for c in base[1]]
        cols[QTY][pos] = vals
        on.batch_mutate(t, 1, 1, deltas=deltas, stats=stats_of(cols))
        rows, jit = run(on, t, fn)
        assert jit                                # materialised: still clean
        orows = oracle_rows(base, fn, deltas=[None, deltas, None])
        assert_matches_oracle(rows, orows, counts)
        return rows

    # a value the dictionary does not hold (and that passes qty < 24), on
    # rows across the tile boundary: the sidecar is rebuilt with 51 entries
    qty, _, disc, key = base[1]
    flips = np.nonzero((qty >= 24) & (disc >= 5 / 128) & (disc <= 7 / 128) &
                       (key >= 1) & (key <= 4))[0]
    assert len(flips) >= 3              # rows the update brings into the sum
    pos = np.unique(np.concatenate([[0, 5, 16383, 16384, n - 1],
                                    flips[:2], flips[-1:]]))
    mutate(pos, np.full(len(pos), 0.5))
    assert on.narrowed_batches(t, QTY) == 3

    # cumulative delta with 300 more new values: past 256, the sidecar goes
    pos2 = np.concatenate([pos, np.setdiff1d(np.arange(100, 500), pos)[:300]])
    vals2 = np.concatenate([np.full(len(pos), 0.5),
                            np.arange(300) / 1024.0 + 2.0])
    mutate(pos2, vals2)
    assert on.narrowed_batches(t, QTY) == 2
    assert on.narrowed_batches(t, DISC) == 3


def test_interpreted_route_reads_the_codes(engines, base):
    """a nullable column with real nulls keeps the plan off the compiled
    kernels; the narrowed columns still come from their sidecars.  Only the
    first batch carries nulls, so it takes the general per-row read while
    the other two stay clean and go through the interpreted kernels' staged
    pipeline and clean conversion loop."""
    on, off = engines
    rng = np.random.default_rng(24)
    extras = []
    for bi, n in enumerate(SIZES):
        valid = (rng.random(n) >= 0.25).astype(np.uint8) if bi == 0 else None
        extras.append((rng.integers(0, 1024, n) / 1024.0, valid))

    def plan_fn():
        p = q6_plan()
        p["aggs"] = p["aggs"] + [("sum", [(4, 0.0, 1.0)]),
                                 ("sum", [(QTY, 0.0, 1.0), (4, 0.0, 1.0)])]
        return p

    t_on = load(on, "nw_interp", base, extras=extras)
    t_off = load(off, "nw_interp", base, extras=extras)
    assert on.narrowed_batches(t_on, QTY) == 3
    assert on.narrowed_batches(t_on, DISC) == 3
    assert on.narrowed_batches(t_on, 4) == 0      # null words: not eligible
    rows_on, jit_on = run(on, t_on, plan_fn)
    rows_off, jit_off = run(off, t_off, plan_fn)
    assert not jit_on and not jit_off
    assert rows_on == rows_off
    assert_matches_oracle(rows_on, oracle_rows(base, plan_fn, extras=extras),
                          (1,))
