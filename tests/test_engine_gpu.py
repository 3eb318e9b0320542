"""GPU parity tests: the HIP engine vs the CPU oracle on identical inputs,
including the reference's TPC-H golden vectors replayed from the committed
fixture (no reference tree needed).

Bars (north star): bit-exact COUNT/integer results; <= 1e-6 relative for
double SUM/AVG (GPU tree-reduction order differs from the JVM loop's).
"""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se
from tests import tpch_util as tu
from tests.golden.make_fixtures import read_batches

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-6


@pytest.fixture(scope="module")
def eng():
    e = se.Engine(device=0)
    yield e
    e.close()


def assert_close(got, exp, rel=REL):
    if exp is None or got is None:
        assert got == exp
        return
    assert abs(got - exp) <= rel * max(1.0, abs(exp)), (got, exp)


def compare_results(grows, orows, count_aggs=()):
    assert len(grows) == len(orows), (grows, orows)
    for (gk, gv), (ok, ov) in zip(grows, orows):
        assert gk == ok
        for a, (g, o) in enumerate(zip(gv, ov)):
            if a in count_aggs:
                assert g == o, f"agg {a} count mismatch: {g} != {o}"
            else:
                assert_close(g, o)


def test_config1_sum_where(eng):
    """BASELINE config 1: SELECT SUM(d) WHERE i > k, 10M rows."""
    n = 10_000_000
    rng = np.random.default_rng(42)
    i32 = rng.integers(0, 10**6, n).astype(np.int32)
    f64 = rng.random(n)
    k = int(np.median(i32))
    t = eng.table_define("c1", [(abi.T_INT32, False), (abi.T_DOUBLE, False)])
    eng.ingest_columns(t, [{"data": i32}, {"data": f64}], n, batch_rows=600_000)
    plan = abi.make_plan(table=t, preds=[dict(col=0, lo=k, lo_strict=True)],
                         aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
    rows = eng.query(plan).rows()
    m = i32 > k
    assert rows[0][1][1] == float(m.sum())            # COUNT bit-exact
    assert_close(rows[0][1][0], float(f64[m].sum()))


@pytest.fixture(scope="module")
def li_fixture_table(eng):
    batches = read_batches(os.path.join(GOLD, "lineitem_batches.bin"))
    t = eng.table_define("li_fix", [(abi.T_DOUBLE, False)] * 4 +
                         [(abi.T_STRING, False)] * 2 + [(abi.T_INT32, False)])
    for bi, (num_rows, cols, stats) in enumerate(batches):
        eng.batch_put(t, bi, bi, num_rows, cols, stats=stats)
    return t


def q6_plan_engine(table):
    return abi.make_plan(
        table=table,
        preds=[dict(col=tu.COL_SHIP, lo=tu.days(1994, 1, 1),
                    hi=tu.days(1995, 1, 1), hi_strict=True),
               dict(col=tu.COL_DISC, is_double=True, lo=0.05, hi=0.07),
               dict(col=tu.COL_QTY, is_double=True, hi=24.0, hi_strict=True)],
        aggs=[("sum", [(tu.COL_EP, 0.0, 1.0), (tu.COL_DISC, 0.0, 1.0)])])


def q1_plan_engine(table):
    cutoff = tu.days(1997, 12, 31) - 90
    return abi.make_plan(
        table=table,
        preds=[dict(col=tu.COL_SHIP, hi=cutoff)],
        group_cols=[tu.COL_RF, tu.COL_LS],
        aggs=[("sum", [(tu.COL_QTY, 0.0, 1.0)]),
              ("sum", [(tu.COL_EP, 0.0, 1.0)]),
              ("sum", [(tu.COL_EP, 0.0, 1.0), (tu.COL_DISC, 1.0, -1.0)]),
              ("sum", [(tu.COL_EP, 0.0, 1.0), (tu.COL_DISC, 1.0, -1.0),
                       (tu.COL_TAX, 1.0, 1.0)]),
              ("avg", [(tu.COL_QTY, 0.0, 1.0)]),
              ("avg", [(tu.COL_EP, 0.0, 1.0)]),
              ("avg", [(tu.COL_DISC, 0.0, 1.0)]),
              ("count", [])])


def test_q6_golden_on_gpu(eng, li_fixture_table):
    rows = eng.query(q6_plan_engine(li_fixture_table)).rows()
    assert len(rows) == 1
    assert tu.fmt(rows[0][1][0]) == tu.GOLDEN_Q6[0]


def test_q1_golden_on_gpu(eng, li_fixture_table):
    rows = eng.query(q1_plan_engine(li_fixture_table)).rows()
    assert tu.q1_result_lines(rows) == tu.GOLDEN_Q1


def test_q6_stats_skip_on_gpu(eng, li_fixture_table):
    q = eng.query(q6_plan_engine(li_fixture_table))
    res = q.result()
    assert res.batches_seen == 8
    # fixture batches are unclustered; skip count may be 0 — just consistency
    assert 0 <= res.batches_skipped < res.batches_seen


def test_q1_synthetic_vs_oracle(eng):
    """Engine and oracle on the same synthetic lineitem data (1M rows)."""
    n = 1_000_000
    t = eng.table_define("li_syn", [(abi.T_DOUBLE, False)] * 4 +
                         [(abi.T_STRING, False)] * 2 + [(abi.T_INT32, False)])
    eng.datagen_lineitem(t, n, seed=42, batch_rows=200_000)
    assert eng.num_rows(t) == n
    grows = eng.query(q1_plan_engine(t)).rows()

    d = se.gen_lineitem_arrays(0, n, seed=42)
    ot = po.OracleTable(tu.LINEITEM_DTYPES)
    for num_rows, cols, stats in tu.encode_lineitem_batches(d, 200_000):
        ot.add_batch(num_rows, cols, stats=stats)
    orows = po.result_rows(ot.query(tu.q1_plan()))
    compare_results(grows, orows, count_aggs={7})


def test_nulls_on_gpu_keyless(eng):
    """nullable inputs through the general path (null bitset + prefix)."""
    n = 100_000
    rng = np.random.default_rng(5)
    vals = rng.random(n)
    valid = (rng.random(n) >= 0.3).astype(np.uint8)
    ivals = rng.integers(0, 1000, n).astype(np.int32)
    t = eng.table_define("tn", [(abi.T_DOUBLE, True), (abi.T_INT32, False)])
    eng.ingest_columns(t, [{"data": vals, "valid": valid}, {"data": ivals}],
                       n, batch_rows=30_000)
    plan = abi.make_plan(table=t, preds=[dict(col=1, hi=500, hi_strict=True)],
                         aggs=[("sum", [(0, 0.0, 1.0)]),
                               ("avg", [(0, 0.0, 1.0)]), ("count", [])])
    rows = eng.query(plan).rows()
    m = ivals < 500
    mv = m & valid.astype(bool)
    assert rows[0][1][2] == float(m.sum())
    assert_close(rows[0][1][0], float(vals[mv].sum()))
    assert_close(rows[0][1][1], float(vals[mv].sum()) / mv.sum())


def test_deletes_and_deltas_on_gpu(eng):
    """delete mask + 2-deep update deltas, engine vs oracle bit-for-bit on
    integer COUNT and 1e-6 on sums (reference formats via oracle encoders)."""
    n = 50_000
    rng = np.random.default_rng(6)
    f64 = rng.random(n)
    i32 = rng.integers(0, 100, n).astype(np.int32)
    cols = [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64),
            po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, i32)]
    del_pos = np.unique(rng.integers(0, n, 500)).astype(np.int32)
    dmask = po.encode_delete(del_pos, n)
    upd_pos = np.unique(rng.integers(0, n, 800)).astype(np.int32)
    upd_vals = rng.random(len(upd_pos)) * 10
    d1 = po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED, upd_pos, n, upd_vals)
    upd2_pos = np.unique(rng.integers(0, n, 400)).astype(np.int32)
    upd2_vals = rng.random(len(upd2_pos)) * 100
    d2 = po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED, upd2_pos, n, upd2_vals)
    deltas = [(d1, d2), (None, None)]

    t = eng.table_define("tdd", [(abi.T_DOUBLE, False), (abi.T_INT32, False)])
    eng.batch_put(t, 0, 0, -n, cols, delete_mask=dmask, deltas=deltas)
    plan = abi.make_plan(table=t, preds=[dict(col=1, hi=50, hi_strict=True)],
                         aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])
    grows = eng.query(plan).rows()

    ot = po.OracleTable([po.T_DOUBLE, po.T_INT32])
    ot.add_batch(-n, cols, delete_mask=dmask, deltas=deltas)
    orows = po.result_rows(ot.query(po.make_plan(
        preds=[dict(col=1, hi=50, hi_strict=True)],
        aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])))
    assert grows[0][1][1] == orows[0][1][1]
    assert_close(grows[0][1][0], orows[0][1][0])


def test_partials_roundtrip_single_gpu(eng, li_fixture_table):
    """partials export + merge(1 block) == direct result (the exchange path).
    Same query object on both sides: two separate launches differ at ~1e-13
    (atomic accumulation order), which the 1e-6 budget allows but a bit-exact
    comparison must avoid."""
    q = eng.query(q6_plan_engine(li_fixture_table))
    direct = q.rows()
    block = q.partials_host()
    q.merge_host(block, len(block), 1)
    assert q.rows() == direct

    q2 = eng.query(q1_plan_engine(li_fixture_table))
    direct = q2.rows()
    block = q2.partials_host()
    q2.merge_host(block, len(block), 1)
    assert q2.rows() == direct


def test_empty_result_on_gpu(eng, li_fixture_table):
    """predicate selecting nothing: SUM -> NULL, COUNT -> 0 (Spark semantics)."""
    plan = abi.make_plan(table=li_fixture_table,
                         preds=[dict(col=tu.COL_SHIP, lo=10**6)],
                         aggs=[("sum", [(tu.COL_EP, 0.0, 1.0)]), ("count", [])])
    rows = eng.query(plan).rows()
    assert rows == [((), [None, 0.0])]


def test_sharded_two_engines_merge(eng):
    """The multi-GPU path on one device: two shard engines (rank 0/1 of 2)
    each hold disjoint buckets; gathered partial blocks merge to the same
    result as an unsharded engine — the exact semantics bench.py runs over
    RCCL at N>1 (partial->final exchange, SnappyHashAggregateExec partial
    modes)."""
    n = 2_000_000
    shards = []
    for rank in range(2):
        e = se.Engine(device=0, shard_rank=rank, shard_count=2)
        t = e.table_define("li", [(abi.T_DOUBLE, False)] * 4 +
                           [(abi.T_STRING, False)] * 2 + [(abi.T_INT32, False)])
        e.datagen_lineitem(t, n, seed=7, batch_rows=100_000)
        shards.append((e, t))
    full = eng.table_define("li_full", [(abi.T_DOUBLE, False)] * 4 +
                            [(abi.T_STRING, False)] * 2 + [(abi.T_INT32, False)])
    eng.datagen_lineitem(full, n, seed=7, batch_rows=100_000)
    assert shards[0][0].num_rows(0) + shards[1][0].num_rows(0) == n

    for plan_fn, count_aggs in ((q6_plan_engine, set()), (q1_plan_engine, {7})):
        qs = [e.query(plan_fn(t)) for e, t in shards]
        blocks = [q.partials_host() for q in qs]
        stride = len(blocks[0])
        assert len(blocks[1]) == stride  # equal-size blocks (all_gather contract)
        gathered = np.concatenate(blocks)
        qs[0].merge_host(gathered, stride, 2)
        merged = qs[0].rows()
        direct = eng.query(plan_fn(full)).rows()
        compare_results(merged, direct, count_aggs=count_aggs)
        for q in qs:
            q.close()
    for e, _ in shards:
        e.close()


def test_q6_with_deltas_workload(eng):
    """BASELINE config 5 shape: Q6 scan with ~2% of rows covered by update
    deltas and ~1% deleted, vs the oracle on identical inputs."""
    n = 500_000
    rng = np.random.default_rng(11)
    d = se.gen_lineitem_arrays(0, n, seed=11)
    cols = [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, d["qty"]),
            po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, d["ep"]),
            po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, d["disc"]),
            po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, d["tax"]),
            po.encode(po.T_STRING, po.ENC_DICT, d["rf"]),
            po.encode(po.T_STRING, po.ENC_DICT, d["ls"]),
            po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, d["ship"])]
    upd = np.unique(rng.integers(0, n, 10_000)).astype(np.int32)
    upd_vals = rng.random(len(upd))  # new discounts
    d1 = po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED, upd, n, upd_vals)
    deltas = [(None, None), (None, None), (d1, None), (None, None),
              (None, None), (None, None), (None, None)]
    dels = np.unique(rng.integers(0, n, 5_000)).astype(np.int32)
    dmask = po.encode_delete(dels, n)

    t = eng.table_define("li_d5", [(abi.T_DOUBLE, False)] * 4 +
                         [(abi.T_STRING, False)] * 2 + [(abi.T_INT32, False)])
    eng.batch_put(t, 0, 0, -n, cols, delete_mask=dmask, deltas=deltas)
    grows = eng.query(q6_plan_engine(t)).rows()

    ot = po.OracleTable(tu.LINEITEM_DTYPES)
    ot.add_batch(-n, cols, delete_mask=dmask, deltas=deltas)
    orows = po.result_rows(ot.query(tu.q6_plan()))
    assert_close(grows[0][1][0], orows[0][1][0])


def test_rle_and_bool_columns_on_gpu(eng):
    """RunLength-encoded int columns (host-built run aux + device binary
    search) and bool columns (byte body + boolean bitset) vs the oracle."""
    n = 200_000
    rng = np.random.default_rng(13)
    rle_vals = np.repeat(rng.integers(0, 50, 4000),
                         rng.integers(20, 80, 4000))[:n].astype(np.int32)
    assert len(rle_vals) == n
    rle64 = (rle_vals.astype(np.int64) * 3) << 33   # exercise raw-i64 path
    bools = (rng.random(n) < 0.3).astype(np.uint8)
    meas = rng.random(n)
    cols = [po.encode(po.T_INT32, po.ENC_RLE, rle_vals),
            po.encode(po.T_INT64, po.ENC_RLE, rle64),
            po.encode(po.T_BOOL, po.ENC_BOOLBITSET, bools),
            po.encode(po.T_BOOL, po.ENC_UNCOMPRESSED, bools),
            po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, meas)]
    schema = [(abi.T_INT32, False), (abi.T_INT64, False), (abi.T_BOOL, False),
              (abi.T_BOOL, False), (abi.T_DOUBLE, False)]
    t = eng.table_define("trle", schema)
    for st in range(0, n, 70_000):
        e_ = min(n, st + 70_000)
        sub = [po.encode(po.T_INT32, po.ENC_RLE, rle_vals[st:e_]),
               po.encode(po.T_INT64, po.ENC_RLE, rle64[st:e_]),
               po.encode(po.T_BOOL, po.ENC_BOOLBITSET, bools[st:e_]),
               po.encode(po.T_BOOL, po.ENC_UNCOMPRESSED, bools[st:e_]),
               po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, meas[st:e_])]
        eng.batch_put(t, st, st // 70_000, e_ - st, sub)
    k = int(np.median(rle_vals))
    i64cut = int(np.median(rle64))
    plan_kw = dict(
        preds=[dict(col=0, hi=k),
               dict(col=1, lo=i64cut, lo_strict=True),
               dict(col=2, lo=1), dict(col=3, lo=1)],   # bools == true
        aggs=[("sum", [(4, 0.0, 1.0)]), ("sum", [(0, 0.0, 1.0)]), ("count", [])])
    grows = eng.query(abi.make_plan(table=t, **plan_kw)).rows()
    ot = po.OracleTable([po.T_INT32, po.T_INT64, po.T_BOOL, po.T_BOOL, po.T_DOUBLE])
    ot.add_batch(n, cols)
    orows = po.result_rows(ot.query(po.make_plan(**plan_kw)))
    assert grows[0][1][2] == orows[0][1][2]           # COUNT bit-exact
    assert grows[0][1][1] == orows[0][1][1]           # integer SUM bit-exact
    assert_close(grows[0][1][0], orows[0][1][0])
    # sanity vs numpy too
    m = (rle_vals <= k) & (rle64 > i64cut) & (bools == 1)
    assert grows[0][1][2] == float(m.sum())


def test_large_group_cardinality_on_gpu(eng):
    """>16 group slots (the LDS hash-aggregate path, SHAMap analogue for
    dictionary keys): 40x25 = 1000 groups vs the oracle."""
    n = 1_000_000
    rng = np.random.default_rng(31)
    k1 = [b"K%02d" % v for v in rng.integers(0, 40, n)]
    k2 = [b"J%02d" % v for v in rng.integers(0, 25, n)]
    meas = rng.random(n)
    mask_col = rng.integers(0, 100, n).astype(np.int32)

    def blobs(sl):
        return [po.encode(po.T_STRING, po.ENC_DICT, k1[sl]),
                po.encode(po.T_STRING, po.ENC_DICT, k2[sl]),
                po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, meas[sl]),
                po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, mask_col[sl])]

    t = eng.table_define("tbig", [(abi.T_STRING, False), (abi.T_STRING, False),
                                  (abi.T_DOUBLE, False), (abi.T_INT32, False)])
    ot = po.OracleTable([po.T_STRING, po.T_STRING, po.T_DOUBLE, po.T_INT32])
    for st in range(0, n, 250_000):
        e_ = min(n, st + 250_000)
        b = blobs(slice(st, e_))
        eng.batch_put(t, st, st // 250_000, e_ - st, b)
        ot.add_batch(e_ - st, b)
    kw = dict(preds=[dict(col=3, hi=80, hi_strict=True)], group_cols=[0, 1],
              aggs=[("sum", [(2, 0.0, 1.0)]), ("avg", [(2, 0.0, 1.0)]), ("count", [])])
    grows = eng.query(abi.make_plan(table=t, **kw)).rows()
    orows = po.result_rows(ot.query(po.make_plan(**kw)))
    assert len(grows) == len(orows) == 1000
    for (gk, gv), (ok_, ov) in zip(grows, orows):
        assert gk == ok_
        assert gv[2] == ov[2]
        for a in (0, 1):
            assert abs(gv[a] - ov[a]) <= 1e-6 * max(1.0, abs(ov[a]))


def test_single_group_col_and_avg_only(eng):
    """ngroup=1 grouped path + AVG-only aggregates vs oracle."""
    n = 300_000
    rng = np.random.default_rng(41)
    keys = [b"G%d" % v for v in rng.integers(0, 5, n)]
    vals = rng.random(n) * 7
    blobs = [po.encode(po.T_STRING, po.ENC_DICT, keys),
             po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, vals)]
    t = eng.table_define("tg1", [(abi.T_STRING, False), (abi.T_DOUBLE, False)])
    eng.batch_put(t, 0, 0, n, blobs)
    ot = po.OracleTable([po.T_STRING, po.T_DOUBLE])
    ot.add_batch(n, blobs)
    kw = dict(group_cols=[0], aggs=[("avg", [(1, 0.0, 1.0)])])
    grows = eng.query(abi.make_plan(table=t, **kw)).rows()
    orows = po.result_rows(ot.query(po.make_plan(**kw)))
    assert len(grows) == len(orows) == 5
    for (gk, gv), (ok_, ov) in zip(grows, orows):
        assert gk == ok_
        assert abs(gv[0] - ov[0]) <= 1e-6 * max(1.0, abs(ov[0]))


def test_sharded_merge_large_groups(eng):
    """sharded partial merge at high cardinality (the path an 8-GPU Q1
    overflow run exercises): 2 shard engines x 600 groups."""
    n = 400_000
    rng = np.random.default_rng(43)
    keys = [b"K%03d" % v for v in rng.integers(0, 600, n)]
    vals = rng.random(n)
    shards = []
    for rank in range(2):
        e = se.Engine(device=0, shard_rank=rank, shard_count=2)
        t = e.table_define("tb", [(abi.T_STRING, False), (abi.T_DOUBLE, False)])
        for bi, st in enumerate(range(0, n, 50_000)):
            e_ = min(n, st + 50_000)
            e.batch_put(t, bi, bi, e_ - st,
                        [po.encode(po.T_STRING, po.ENC_DICT, keys[st:e_]),
                         po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, vals[st:e_])])
        shards.append((e, t))
    kw = dict(group_cols=[0], aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
    qs = [e.query(abi.make_plan(table=t, **kw)) for e, t in shards]
    blocks = [q.partials_host() for q in qs]
    qs[0].merge_host(np.concatenate(blocks), len(blocks[0]), 2)
    merged = qs[0].rows()

    full = eng.table_define("tbf", [(abi.T_STRING, False), (abi.T_DOUBLE, False)])
    for bi, st in enumerate(range(0, n, 50_000)):
        e_ = min(n, st + 50_000)
        eng.batch_put(full, bi, bi, e_ - st,
                      [po.encode(po.T_STRING, po.ENC_DICT, keys[st:e_]),
                       po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, vals[st:e_])])
    direct = eng.query(abi.make_plan(table=full, **kw)).rows()
    assert len(merged) == len(direct) == 600
    for (mk, mv), (dk, dv) in zip(merged, direct):
        assert mk == dk and mv[1] == dv[1]
        assert abs(mv[0] - dv[0]) <= 1e-6 * max(1.0, abs(dv[0]))
    for q in qs:
        q.close()
    for e, _ in shards:
        e.close()


def test_jit_engages_on_clean_scans(eng, li_fixture_table):
    """Clean fixture batches with uniform kinds must run the query-compiled
    (hipRTC) kernel — and fall back to the interpreted kernels the moment a
    delta patch dirties a batch, with identical results either way."""
    q6 = eng.query(q6_plan_engine(li_fixture_table))
    q6.rows()
    assert q6.used_jit(), "Q6 over clean batches should run the JIT kernel"
    q1 = eng.query(q1_plan_engine(li_fixture_table))
    q1.rows()
    assert q1.used_jit(), "Q1 over clean batches should run the JIT kernel"

    # value-only patches materialize into the device body at put time, so
    # the batch still runs the JIT kernel with the patched values
    n = 40_000
    rng = np.random.default_rng(77)
    f64 = np.round(rng.random(n), 3)
    t = eng.table_define("tjit", [(abi.T_DOUBLE, False)])
    eng.batch_put(t, 0, 0, n,
                  [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)])
    plan = abi.make_plan(table=t, aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])
    qa = eng.query(plan)
    ra = qa.rows()
    assert qa.used_jit()
    pos = np.array([1, 5], dtype=np.int32)
    nv = np.array([9.5, 10.5])
    delta = se.encode_update_delta(abi.T_DOUBLE, pos, n, nv)
    t2 = eng.table_define("tjit2", [(abi.T_DOUBLE, False)])
    eng.batch_put(t2, 0, 0, n,
                  [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)],
                  deltas=[(delta, None)])
    plan2 = abi.make_plan(table=t2, aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])
    qb = eng.query(plan2)
    rb = qb.rows()
    assert qb.used_jit(), "value-only patches materialize; JIT should engage"
    assert rb[0][1][1] == ra[0][1][1]
    exp = f64.sum() - f64[pos].sum() + nv.sum()
    assert abs(rb[0][1][0] - exp) <= 1e-9 * abs(exp)

    # a patch that writes NULL cannot materialize -> interpreted path
    nvn = np.array([3.25, 0.0])
    deltan = se.encode_update_delta(abi.T_DOUBLE, pos, n, nvn,
                                    valid=np.array([1, 0], dtype=np.uint8))
    t3 = eng.table_define("tjit3", [(abi.T_DOUBLE, True)])
    eng.batch_put(t3, 0, 0, n,
                  [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)],
                  deltas=[(deltan, None)])
    plan3 = abi.make_plan(table=t3, aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])
    qc = eng.query(plan3)
    rcc = qc.rows()
    assert not qc.used_jit(), "null-writing patch must use the interpreted path"
    assert rcc[0][1][1] == float(n)      # COUNT(*) keeps the row
    exp3 = f64.sum() - f64[1] - f64[5] + 3.25
    assert abs(rcc[0][1][0] - exp3) <= 1e-9 * abs(exp3)

    # deletes alone stay on the JIT path (del_bm honored by generated code)
    dels = np.arange(0, n, 97, dtype=np.int32)
    dmask = po.encode_delete(dels, n)
    t4 = eng.table_define("tjit4", [(abi.T_DOUBLE, False)])
    eng.batch_put(t4, 0, 0, n,
                  [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)],
                  delete_mask=dmask)
    plan4 = abi.make_plan(table=t4, aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])
    qd = eng.query(plan4)
    rd = qd.rows()
    assert qd.used_jit(), "delete-only batches should stay on the JIT path"
    keep = np.ones(n, dtype=bool); keep[dels] = False
    assert rd[0][1][1] == float(keep.sum())
    exp4 = f64[keep].sum()
    assert abs(rd[0][1][0] - exp4) <= 1e-9 * abs(exp4)


def test_key_sharded_a2a_split_merge(eng):
    """Key-sharded all-to-all exchange: each shard splits its
    grouped partials by key-hash owner; after the (emulated) all-to-all each
    rank merges only the blocks carrying its keys, and the union across
    ranks equals the unsharded result.  Transport (all_to_all_single /
    all_gather) is covered by test_distributed; this test pins the C-side
    split + merge semantics with real partial blocks."""
    n = 300_000
    world = 2
    rng = np.random.default_rng(91)
    keys = [b"K%03d" % v for v in rng.integers(0, 500, n)]
    vals = rng.random(n)
    kw = dict(group_cols=[0], aggs=[("sum", [(1, 0.0, 1.0)]),
                                    ("avg", [(1, 0.0, 1.0)]), ("count", [])])

    def put_all(e, t, shard=None):
        for bi, st in enumerate(range(0, n, 60_000)):
            en = min(n, st + 60_000)
            e.batch_put(t, bi, bi, en - st,
                        [po.encode(po.T_STRING, po.ENC_DICT, keys[st:en]),
                         po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, vals[st:en])])

    shards = []
    for rank in range(world):
        e = se.Engine(device=0, shard_rank=rank, shard_count=world)
        t = e.table_define("ta2a", [(abi.T_STRING, False), (abi.T_DOUBLE, False)])
        put_all(e, t)
        shards.append((e, t))
    qs = [e.query(abi.make_plan(table=t, **kw)) for e, t in shards]
    bb = qs[0].partial_bytes()
    split = [q.partials_sharded(world) for q in qs]   # [src][dst] blocks
    union = {}
    for rank in range(world):
        # the all-to-all delivers split[src][rank] for every src
        recv = np.concatenate([split[src][rank] for src in range(world)])
        qs[rank].merge_host(recv, bb, world)
        for k, v in qs[rank].rows():
            assert k not in union, f"key {k} owned by two ranks"
            union[k] = v

    full_e = se.Engine(device=0)
    tf = full_e.table_define("ta2af", [(abi.T_STRING, False), (abi.T_DOUBLE, False)])
    put_all(full_e, tf)
    direct = full_e.query(abi.make_plan(table=tf, **kw)).rows()
    assert len(union) == len(direct) == 500
    for dk, dv in direct:
        uv = union[dk]
        assert uv[2] == dv[2]
        for a in (0, 1):
            assert abs(uv[a] - dv[a]) <= 1e-6 * max(1.0, abs(dv[a]))
    for q in qs:
        q.close()
    for e, _ in shards:
        e.close()
    full_e.close()


def test_edge_all_rows_deleted(eng):
    """A batch whose every row is deleted: scans to an empty/NULL result
    (SUM of nothing is NULL, COUNT(*) 0 — Spark semantics)."""
    n = 10_000
    f64 = np.arange(n, dtype=np.float64)
    dmask = po.encode_delete(np.arange(n, dtype=np.int32), n)
    t = eng.table_define("tdel_all", [(abi.T_DOUBLE, False)])
    eng.batch_put(t, 0, 0, n, [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)],
                  delete_mask=dmask)
    plan = abi.make_plan(table=t, aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])
    rows = eng.query(plan).rows()
    assert rows[0][1][1] == 0.0
    assert rows[0][1][0] is None


def test_edge_delta_covers_every_row(eng):
    """An update delta patching EVERY row (materialized at put): result must
    reflect only the new values."""
    n = 20_000
    rng = np.random.default_rng(13)
    f64 = rng.random(n)
    nv = rng.random(n) * 7
    delta = se.encode_update_delta(abi.T_DOUBLE, np.arange(n, dtype=np.int32),
                                   n, nv)
    t = eng.table_define("tdelta_all", [(abi.T_DOUBLE, False)])
    eng.batch_put(t, 0, 0, n, [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)],
                  deltas=[(delta, None)])
    q = eng.query(abi.make_plan(table=t, aggs=[("sum", [(0, 0.0, 1.0)]),
                                               ("count", [])]))
    rows = q.rows()
    assert q.used_jit()
    assert rows[0][1][1] == float(n)
    assert abs(rows[0][1][0] - nv.sum()) <= 1e-9 * abs(nv.sum())


def test_edge_delete_wins_over_delta(eng):
    """A row both updated and deleted: the delete wins (the reference checks
    the delete bitmap before the delta merge) — engine vs oracle."""
    n = 5_000
    rng = np.random.default_rng(14)
    f64 = rng.random(n)
    pos = np.array([10, 20, 30], dtype=np.int32)
    nv = np.array([100.0, 200.0, 300.0])
    delta = po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED, pos, n, nv)
    dmask = po.encode_delete(np.array([20], dtype=np.int32), n)
    cols = [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)]
    t = eng.table_define("tdd2", [(abi.T_DOUBLE, False)])
    eng.batch_put(t, 0, 0, -n, cols, delete_mask=dmask,
                  deltas=[(delta, None)])
    grows = eng.query(abi.make_plan(table=t, aggs=[("sum", [(0, 0.0, 1.0)]),
                                                   ("count", [])])).rows()
    ot = po.OracleTable([po.T_DOUBLE])
    ot.add_batch(-n, cols, delete_mask=dmask, deltas=[(delta, None)])
    orows = po.result_rows(ot.query(po.make_plan(
        aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])))
    assert grows[0][1][1] == orows[0][1][1] == float(n - 1)
    assert abs(grows[0][1][0] - orows[0][1][0]) <= 1e-9 * abs(orows[0][1][0])


def test_edge_mixed_clean_and_null_patched_batches(eng):
    """A table mixing clean batches and a null-writing-patched batch must
    fall back to the interpreted kernels as a whole and stay correct."""
    n = 30_000
    rng = np.random.default_rng(15)
    a, b = rng.random(n), rng.random(n)
    t = eng.table_define("tmix", [(abi.T_DOUBLE, True)])
    eng.batch_put(t, 0, 0, n, [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, a)])
    deltan = se.encode_update_delta(abi.T_DOUBLE, np.array([3], dtype=np.int32),
                                    n, np.array([0.0]),
                                    valid=np.array([0], dtype=np.uint8))
    eng.batch_put(t, 1, 1, n, [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, b)],
                  deltas=[(deltan, None)])
    q = eng.query(abi.make_plan(table=t, aggs=[("sum", [(0, 0.0, 1.0)]),
                                               ("count", [])]))
    rows = q.rows()
    assert not q.used_jit()
    exp = a.sum() + b.sum() - b[3]
    assert rows[0][1][1] == float(2 * n)
    assert abs(rows[0][1][0] - exp) <= 1e-9 * abs(exp)


def test_concurrent_ingest_and_scan(eng):
    """BASELINE config 5's 'concurrent' part: one thread keeps ingesting
    batches while another queries; every result must be a consistent
    prefix of the batches (rowcount never decreases, sums match the
    prefix expectation) and the final query sees everything."""
    import threading
    n_batches, rows = 40, 20_000
    rng = np.random.default_rng(17)
    data = [np.round(rng.random(rows), 3) for _ in range(n_batches)]
    t = eng.table_define("tconc", [(abi.T_DOUBLE, False)])
    plan = abi.make_plan(table=t, aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])
    stop = threading.Event()
    errs = []

    def ingest():
        try:
            for bi in range(n_batches):
                eng.batch_put(t, bi, bi, rows,
                              [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED,
                                         data[bi])])
        except Exception as ex:  # pragma: no cover
            errs.append(ex)
        finally:
            stop.set()

    prefix_sums = np.cumsum([d.sum() for d in data])
    seen = []

    def scan():
        try:
            while not stop.is_set() or not seen:
                res = eng.query(plan).rows()
                cnt = res[0][1][1]
                if cnt == 0.0:
                    continue
                k = int(cnt // rows)
                assert cnt == k * float(rows), "partial batch visible"
                assert abs(res[0][1][0] - prefix_sums[k - 1]) <= \
                    1e-9 * prefix_sums[k - 1]
                if seen and k < seen[-1]:
                    raise AssertionError("rowcount went backwards")
                seen.append(k)
        except Exception as ex:  # pragma: no cover
            errs.append(ex)

    ti = threading.Thread(target=ingest)
    ts = threading.Thread(target=scan)
    ti.start(); ts.start()
    ti.join(timeout=120); ts.join(timeout=120)
    assert not errs, errs
    final = eng.query(plan).rows()
    assert final[0][1][1] == float(n_batches * rows)
    assert abs(final[0][1][0] - prefix_sums[-1]) <= 1e-9 * prefix_sums[-1]


def test_partials_into_device_matches_host(eng):
    """The N>1 keyless exchange writes partials straight into a device
    buffer (bench all_reduces a torch CUDA tensor) — must equal the host
    export bit-for-bit."""
    import ctypes as C
    n = 100_000
    rng = np.random.default_rng(19)
    f64 = rng.random(n)
    t = eng.table_define("tpd", [(abi.T_DOUBLE, False)])
    eng.batch_put(t, 0, 0, n, [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)])
    q = eng.query(abi.make_plan(table=t, aggs=[("sum", [(0, 0.0, 1.0)]),
                                               ("avg", [(0, 0.0, 1.0)]),
                                               ("count", [])]))
    host = q.partials_host()
    hip = C.CDLL("libamdhip64.so")
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), C.c_size_t(len(host))) == 0
    q.partials_into_device(ptr.value)
    back = np.zeros(len(host), dtype=np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), ptr,
                         C.c_size_t(len(host)), 2) == 0   # DeviceToHost
    hip.hipFree(ptr)
    assert bytes(back) == bytes(host)


def test_tokenized_plan_cache_reuse(eng):
    """The reference tokenizes literals so different predicate values share
    one generated class (TokenizationTest); here different bounds and
    aggregate coefficients must reuse ONE compiled kernel per plan shape."""
    n = 100_000
    rng = np.random.default_rng(23)
    i32 = rng.integers(0, 1000, n).astype(np.int32)
    f64 = rng.random(n)
    t = eng.table_define("ttok", [(abi.T_INT32, False), (abi.T_DOUBLE, False)])
    eng.ingest_columns(t, [{"data": i32}, {"data": f64}], n, batch_rows=50_000)
    before = eng.jit_count()
    for k, mul in ((100, 1.0), (500, 2.5), (900, -1.0)):
        q = eng.query(abi.make_plan(
            table=t, preds=[dict(col=0, hi=k, hi_strict=True)],
            aggs=[("sum", [(1, 0.0, mul)]), ("count", [])]))
        rows = q.rows()
        assert q.used_jit()
        m = i32 < k
        assert rows[0][1][1] == float(m.sum())
        exp = mul * f64[m].sum()
        assert abs(rows[0][1][0] - exp) <= 1e-9 * max(1.0, abs(exp))
    after = eng.jit_count()
    # three literal variants add AT MOST one shape entry (zero when an
    # earlier test already compiled this shape)
    assert after - before <= 1, (before, after)


def test_stats_skip_never_drops_patched_batches(eng):
    """A batch whose update delta moves values INTO the predicate range must
    not be stats-skipped off the base bounds (has_deltas regression: deltas
    with a positive row count)."""
    n = 50_000
    rng = np.random.default_rng(29)
    f64 = rng.random(n)          # all < 1.0: base stats say hi < 1.0
    i32 = rng.integers(0, 100, n).astype(np.int32)
    pos = np.array([7, 9], dtype=np.int32)
    nv = np.array([5.0, 6.0])    # patched values OUTSIDE the base bounds
    delta = se.encode_update_delta(abi.T_DOUBLE, pos, n, nv)
    t = eng.table_define("tsk", [(abi.T_DOUBLE, False), (abi.T_INT32, False)])
    stats = po.encode_stats([po.T_DOUBLE, po.T_INT32], n,
                            [float(f64.min()), int(i32.min())],
                            [float(f64.max()), int(i32.max())])
    eng.batch_put(t, 0, 0, n,
                  [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64),
                   po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, i32)],
                  stats=stats, deltas=[(delta, None), (None, None)])
    # predicate selects ONLY the patched values (> 2.0); base stats would skip
    q = eng.query(abi.make_plan(table=t,
                                preds=[dict(col=0, is_double=True, lo=2.0)],
                                aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])]))
    rows = q.rows()
    assert rows[0][1][1] == 2.0
    assert abs(rows[0][1][0] - 11.0) <= 1e-9 * 11.0


def test_batch_mutate_after_put(eng):
    """UPDATE/DELETE after the batch exists (sn_batch_mutate): cumulative
    delta + delete state replaces the old, descriptor caches invalidate,
    and repeated identical plans see each new state."""
    n = 40_000
    rng = np.random.default_rng(31)
    f64 = np.round(rng.random(n), 3)
    t = eng.table_define("tmut", [(abi.T_DOUBLE, False)])
    eng.batch_put(t, 77, 0, n, [po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)])
    plan = abi.make_plan(table=t, aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])
    r0 = eng.query(plan).rows()
    assert abs(r0[0][1][0] - f64.sum()) <= 1e-9 * f64.sum()

    # UPDATE rows 3 and 5
    pos = np.array([3, 5], dtype=np.int32)
    nv = np.array([10.0, 20.0])
    d1 = se.encode_update_delta(abi.T_DOUBLE, pos, n, nv)
    eng.batch_mutate(t, 77, 0, deltas=[(d1, None)])
    r1 = eng.query(plan).rows()
    exp1 = f64.sum() - f64[pos].sum() + nv.sum()
    assert r1[0][1][1] == float(n)
    assert abs(r1[0][1][0] - exp1) <= 1e-9 * exp1

    # later, a LARGER cumulative delta (includes the first updates) + DELETE
    pos2 = np.array([3, 5, 9], dtype=np.int32)
    nv2 = np.array([10.0, 20.0, 30.0])
    d2 = se.encode_update_delta(abi.T_DOUBLE, pos2, n, nv2)
    dmask = po.encode_delete(np.array([5], dtype=np.int32), n)
    eng.batch_mutate(t, 77, 0, deltas=[(d2, None)], delete_mask=dmask)
    r2 = eng.query(plan).rows()
    ref = f64.copy(); ref[pos2] = nv2
    keep = np.ones(n, bool); keep[5] = False
    assert r2[0][1][1] == float(n - 1)
    exp2 = ref[keep].sum()
    assert abs(r2[0][1][0] - exp2) <= 1e-9 * exp2


def test_fullsize_checksum_of_checksums(eng):
    """size-independent property at scale (SURVEY §8 contract): the grouped
    sums roll up to the keyless totals on a 10M-row table."""
    n = 10_000_000
    t = eng.table_define("li_cs", [(abi.T_DOUBLE, False)] * 4 +
                         [(abi.T_STRING, False)] * 2 + [(abi.T_INT32, False)])
    eng.datagen_lineitem(t, n, seed=7, batch_rows=600_000)
    g = eng.query(abi.make_plan(table=t, group_cols=[tu.COL_RF, tu.COL_LS],
                                aggs=[("sum", [(tu.COL_EP, 0.0, 1.0)]),
                                      ("count", [])]))
    grows = g.rows()
    k = eng.query(abi.make_plan(table=t,
                                aggs=[("sum", [(tu.COL_EP, 0.0, 1.0)]),
                                      ("count", [])]))
    krows = k.rows()
    assert g.used_jit() and k.used_jit()
    gsum = sum(v[0] for _, v in grows)
    gcnt = sum(v[1] for _, v in grows)
    assert gcnt == krows[0][1][1] == float(n)
    assert abs(gsum - krows[0][1][0]) <= 1e-9 * abs(gsum)


def test_concurrent_raw_ingest_and_scan(eng):
    """Config-5 concurrency over the f2 RAW ingest path: device-computed
    stats are resolved lazily (sync_pending_stats under the table lock)
    while another thread queries with a stats-skippable predicate — every
    result must still be a consistent batch prefix."""
    import threading
    n_batches, rows = 30, 20_000
    rng = np.random.default_rng(19)
    data = [np.round(rng.random(rows), 3) + bi for bi in range(n_batches)]
    t = eng.table_define("tconcraw", [(abi.T_DOUBLE, False)])
    # predicate (col >= 0) exercises the stats path on every submit
    plan = abi.make_plan(table=t, preds=[dict(col=0, is_double=True, lo=0.0)],
                         aggs=[("sum", [(0, 0.0, 1.0)]), ("count", [])])
    stop = threading.Event()
    errs = []

    def ingest():
        try:
            for bi in range(n_batches):
                eng.ingest_columns(t, [{"data": data[bi]}], rows,
                                   batch_rows=rows, first_bucket=bi)
        except Exception as ex:  # pragma: no cover
            errs.append(ex)
        finally:
            stop.set()

    prefix_sums = np.cumsum([d.sum() for d in data])

    def scan():
        try:
            seen_any = False
            while not stop.is_set() or not seen_any:
                res = eng.query(plan).rows()
                cnt = res[0][1][1]
                if cnt == 0.0:
                    continue
                seen_any = True
                k = int(cnt // rows)
                assert cnt == k * float(rows), "partial batch visible"
                assert abs(res[0][1][0] - prefix_sums[k - 1]) <= \
                    1e-9 * prefix_sums[k - 1]
        except Exception as ex:  # pragma: no cover
            errs.append(ex)

    ti = threading.Thread(target=ingest)
    ts = threading.Thread(target=scan)
    ti.start(); ts.start()
    ti.join(timeout=120); ts.join(timeout=120)
    assert not errs, errs
    final = eng.query(plan).rows()
    assert final[0][1][1] == float(n_batches * rows)
    # stats landed: a selective predicate skips provably-excluded batches
    hi = eng.query(abi.make_plan(
        table=t, preds=[dict(col=0, is_double=True, lo=float(n_batches + 5))],
        aggs=[("count", [])]))
    res = hi.result()
    assert res.batches_skipped == res.batches_seen  # all excluded by bounds


@pytest.mark.gpu
def test_concurrent_submits_different_tables():
    """Two threads submitting queries on DIFFERENT tables of one engine:
    the per-engine submit lock keeps the shared stream/scratch/hash
    workspaces from interleaving (pre-fix, sparse workspaces and the
    block-partial scratch could be clobbered between a scan and its
    reduce)."""
    import threading
    e = se.Engine(device=0)
    try:
        rng = np.random.default_rng(431)
        tables, expect = [], []
        for i in range(2):
            n = 400_000
            keys = rng.integers(0, 30_000, n).astype(np.int64) * (1 << 25) + i
            w = rng.random(n)
            t = e.table_define(f"tconc{i}", [(abi.T_INT64, False),
                                             (abi.T_DOUBLE, False)])
            e.ingest_columns(t, [{"data": keys}, {"data": w}], n,
                             batch_rows=100_000)
            tables.append(t)
            expect.append((len(np.unique(keys)), float(w.sum())))
        errs = []

        def worker(i):
            try:
                for _ in range(6):
                    q = e.query(abi.make_plan(
                        table=tables[i], group_cols=[0],
                        aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])]))
                    q.wait()
                    ng = q.num_groups()
                    assert ng == expect[i][0], (i, ng, expect[i][0])
                    qa = e.query(abi.make_plan(
                        table=tables[i], aggs=[("sum", [(1, 0.0, 1.0)])]))
                    s = qa.rows()[0][1][0]
                    assert abs(s - expect[i][1]) <= 1e-6 * expect[i][1], (i, s)
            except Exception as ex:   # noqa: BLE001
                errs.append((i, repr(ex)))

        th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
    finally:
        e.close()


def test_count_star_unaffected_by_nonfinite_column_values(eng):
    """COUNT(*) has no input factor, so an infinite value in a column the
    plan merely filters on must not reach it: the interpreted kernels used
    to evaluate the unused factors as (1 + 0*x), which is NaN for x = inf.
    The nullable column keeps the plan on the interpreted kernels."""
    n = 5000
    rng = np.random.default_rng(61)
    x = rng.random(n)
    x[::7] = np.inf
    x[3::11] = np.nan
    y = rng.integers(0, 100, n).astype(np.int32)
    valid = (rng.random(n) > 0.2).astype(np.uint8)
    t = eng.table_define("tinf", [(abi.T_DOUBLE, False), (abi.T_INT32, True)])
    assert eng.ingest_columns(t, [{"data": x}, {"data": y, "valid": valid}],
                              n, batch_rows=2000) == n
    rows = eng.query(abi.make_plan(
        table=t, preds=[dict(col=0, is_double=True, lo=0.5), dict(col=1, hi=50)],
        aggs=[("count", []), ("sum", [(1, 0.0, 1.0)])])).rows()
    with np.errstate(invalid="ignore"):
        m = (x >= 0.5) & (valid == 1) & (y <= 50)      # NaN and NULL fail
    assert np.isinf(x[m]).any()
    assert rows[0][1][0] == float(m.sum())
    assert rows[0][1][1] == float(y[m].sum())
