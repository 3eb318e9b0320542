"""The three ways a submit obtains its batch descriptor set, per launch
route: built and cached (first submit of a plan), taken from the table's
cache (same plan again), and built uncached and query-owned (a stats-skipping
predicate removes a batch).  Every route must compute the same thing from
each, and the cached set must survive an uncached submit in between.

Table: 3 batches x 2,000 rows — one 16,384-row tile per batch.  The date
column's per-batch ranges are disjoint so `date >= 10000` stats-skips exactly
batch 0.  Doubles are multiples of 1/64 below 100, so every sum is exact in
f64 whatever order the device adds in: miss and hit can be compared bit for
bit and the numpy reference is exact too.  The int64 key column (~500 wide-
spread values) takes the sparse hash route with a table of 2^14 entries or
fewer, far below the 2^17 radix threshold.  The decimal route reads a
fifth, int64 column declared DECIMAL(15,2); the reference for it is Python
int arithmetic.
"""
import numpy as np
import pytest

from snappydata_amd import abi, engine as se

pytestmark = pytest.mark.gpu

REL = 1e-6
NB, BR = 3, 2000
N = NB * BR
C_DATE, C_DBL, C_STR, C_KEY, C_DEC = range(5)
STRS = [b"AIR", b"MAIL", b"RAIL", b"SHIP", b"TRUCK"]
SKIP_PRED = dict(col=C_DATE, lo=10_000)          # batch 0 holds dates < 1000


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20261020)
    universe = rng.integers(-2**62, 2**62, 500).astype(np.int64)
    return dict(
        date=(np.repeat(np.arange(NB), BR) * 10_000 +
              rng.integers(0, 1000, N)).astype(np.int32),
        dbl=rng.integers(0, 6400, N).astype(np.float64) / 64.0,
        s=[STRS[i] for i in rng.integers(0, len(STRS), N)],
        key=universe[rng.integers(0, len(universe), N)],
        dec=rng.integers(-10**9, 10**9, N).astype(np.int64))


@pytest.fixture
def table(data):
    eng = se.Engine(device=0)
    t = eng.table_define("paths", [(abi.T_INT32, False), (abi.T_DOUBLE, False),
                                   (abi.T_STRING, False), (abi.T_INT64, False),
                                   (abi.T_INT64, False)])
    for b in range(NB):
        sl = slice(b * BR, (b + 1) * BR)
        ss = data["s"][sl]
        cols = [{"data": data["date"][sl]}, {"data": data["dbl"][sl]},
                {"data": b"".join(ss),
                 "lens": np.array([len(v) for v in ss], dtype=np.int32)},
                {"data": data["key"][sl]}, {"data": data["dec"][sl]}]
        assert eng.ingest_columns(t, cols, BR, batch_rows=BR, first_bucket=b) == BR
    eng.table_set_decimal(t, C_DEC, 15, 2)
    yield eng, t
    eng.close()


def ref_groups(data, mask, keys):
    """{key tuple: (sum(dbl), count)} over the masked rows (numpy)."""
    if keys is None:
        return {(): (float(data["dbl"][mask].sum()), float(mask.sum()))}
    out = {}
    keys = np.asarray(keys)
    for k in np.unique(keys[mask]):
        m = mask & (keys == k)
        name = k.decode() if isinstance(k, bytes) else str(k)
        out[(name,)] = (float(data["dbl"][m].sum()), float(m.sum()))
    return out


AGGS = [("sum", [(C_DBL, 0.0, 1.0)]), ("count", [])]
DBL_PRED = dict(col=C_DBL, is_double=True, lo=25.0)

# route -> (base predicates, group columns, reference key column)
ROUTES = {
    "dense_keyless": ([DBL_PRED], [], None),
    "dense_grouped": ([], [C_STR], "s"),
    "sparse": ([], [C_KEY], "key"),
}


def metrics(q):
    res = q.result()
    return int(res.batches_skipped), int(res.rows_scanned)


def check_sequence(submit, reference):
    """miss, hit, uncached (skipping), hit again — the assertions every
    route shares.  submit(skip) -> (query, comparable rows);
    reference(rows, skip) asserts rows against the host-computed result."""
    q_miss, miss = submit(False)
    q_hit, hit = submit(False)
    q_skip, skipped = submit(True)
    q_again, again = submit(False)
    for q in (q_miss, q_hit, q_again):
        assert metrics(q) == (0, N)
    assert metrics(q_skip) == (1, N - BR)
    assert hit == miss and again == miss          # bit-identical
    assert q_hit.used_jit() == q_miss.used_jit() == q_again.used_jit()
    reference(miss, False)
    reference(skipped, True)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_double_routes(table, data, route):
    eng, t = table
    preds, group_cols, keyname = ROUTES[route]

    def submit(skip):
        q = eng.query(abi.make_plan(
            table=t, preds=preds + ([SKIP_PRED] if skip else []),
            group_cols=group_cols, aggs=AGGS))
        return q, q.rows()

    def reference(rows, skip):
        mask = np.ones(N, dtype=bool)
        if preds:
            mask &= data["dbl"] >= 25.0
        if skip:
            mask &= data["date"] >= 10_000
        ref = ref_groups(data, mask, None if keyname is None else data[keyname])
        assert len(rows) == len(ref)
        for keys, (gsum, gcount) in rows:
            rsum, rcount = ref[keys]
            assert gcount == rcount, (keys, gcount, rcount)
            assert abs(gsum - rsum) <= REL * max(1.0, abs(rsum)), (keys, gsum, rsum)

    check_sequence(submit, reference)


def test_decimal_route(table, data):
    eng, t = table
    aggs = [("sum", [(C_DEC, 0, 1)]), ("count", [])]

    def submit(skip):
        plan, arr = abi.make_dec_plan(
            table=t, preds=[SKIP_PRED] if skip else [], aggs=aggs)
        q = eng.query_dec(plan, arr)
        return q, q.dec_rows()

    def reference(rows, skip):
        mask = data["date"] >= (10_000 if skip else 0)
        total = sum(int(v) for v in data["dec"][mask])
        assert rows == [((), [total, int(mask.sum())], [2, 0])]

    check_sequence(submit, reference)
