"""One exact test per interpreted (non-query-compiled) kernel route.

Which hand-written kernel a plan reaches is decided by its shape; every case
below is the smallest shape that reaches one route, over one shared table:

  batch 0: 2*1024 + 37 rows, clean   -> two staged full chunks, then a
                                        ragged tail through convert_chunk
  batch 1: 1024 + 1 rows, one real NULL in a nullable column that every plan
           only FILTERS on -> the whole scan stays on the interpreted
           kernels (a null batch is never query-compiled) without turning on
           per-aggregate counts

All values are small integers held in doubles / ints, so every sum is exact
in a double whatever order the atomics land in: every assertion is exact
equality against a numpy (decimal: Python int) reference computed here."""
import numpy as np
import pytest

from snappydata_amd import abi, engine as se

pytestmark = pytest.mark.gpu

SIZES = [2 * 1024 + 37, 1024 + 1]
N = sum(SIZES)

(C_F, C_D0, C_D1, C_D2, C_D3, C_I, C_G6, C_G12, C_G40, C_G3, C_N, C_G1500,
 C_K64, C_JK, C_DA, C_DB) = range(16)

SCHEMA = [(abi.T_DOUBLE, True)] + [(abi.T_DOUBLE, False)] * 4 + \
         [(abi.T_INT32, False)] * 5 + [(abi.T_DOUBLE, True),
                                       (abi.T_INT32, False),
                                       (abi.T_INT64, True),
                                       (abi.T_INT32, False),
                                       (abi.T_INT64, False),
                                       (abi.T_INT64, False)]

NULL_F_ROW = SIZES[0] + 500            # the one NULL of the filter column
SPARSE_KEYS = 48                       # + the -1 key + the NULL key = 50


def _make_data():
    rng = np.random.default_rng(2085)
    i = np.arange(N)
    cols, valid = {}, {c: np.ones(N, dtype=bool) for c in range(len(SCHEMA))}
    cols[C_F] = rng.integers(1, 4, N).astype(np.float64)
    valid[C_F][NULL_F_ROW] = False
    for c in (C_D0, C_D1, C_D2, C_D3):
        cols[c] = rng.integers(0, 8, N).astype(np.float64)
    cols[C_I] = rng.integers(0, 10, N).astype(np.int32)
    cols[C_G6] = (i % 6).astype(np.int32)
    cols[C_G12] = (i * 5 % 12).astype(np.int32)
    cols[C_G40] = (i * 7 % 40).astype(np.int32)
    cols[C_G3] = (i * 2 % 3).astype(np.int32)
    cols[C_N] = rng.integers(0, 8, N).astype(np.float64)
    valid[C_N][SIZES[0] + 3::97] = False          # real NULLs, batch 1 only
    cols[C_G1500] = (i * 7 % 1500).astype(np.int32)
    kidx = i * 13 % (SPARSE_KEYS + 2)
    k64 = kidx.astype(np.int64) * (1 << 33) + 12345
    k64[kidx == SPARSE_KEYS] = -1
    valid[C_K64][kidx == SPARSE_KEYS + 1] = False
    cols[C_K64] = k64
    cols[C_JK] = rng.integers(0, 100, N).astype(np.int32)
    cols[C_DA] = rng.integers(-10 ** 6, 10 ** 6, N).astype(np.int64)
    cols[C_DB] = rng.integers(0, 100, N).astype(np.int64)
    for c in cols:                                 # NULL slots hold a 0
        cols[c] = np.where(valid[c], cols[c], 0).astype(cols[c].dtype)
    return cols, valid


COLS, VALID = _make_data()


@pytest.fixture(scope="module")
def loaded():
    eng = se.Engine(device=0)
    t = eng.table_define("routes", SCHEMA)
    s = 0
    for bi, n in enumerate(SIZES):
        part = []
        for c, (_dt, nullable) in enumerate(SCHEMA):
            col = {"data": np.ascontiguousarray(COLS[c][s:s + n])}
            if nullable and not VALID[c][s:s + n].all():
                col["valid"] = VALID[c][s:s + n].astype(np.uint8)
            part.append(col)
        assert eng.ingest_columns(t, part, n, batch_rows=n, first_bucket=bi) == n
        s += n
    eng.table_set_decimal(t, C_DA, 15, 2)
    eng.table_set_decimal(t, C_DB, 15, 2)
    yield eng, t
    eng.close()


# ------------------------------------------------------------- reference


F_PRED = dict(col=C_F, is_double=True, lo=0.0)


def pred_mask(preds):
    m = np.ones(N, dtype=bool)
    for p in preds:
        x = COLS[p["col"]]
        m &= VALID[p["col"]]
        if "lo" in p:
            m &= x >= p["lo"]
        if "hi" in p:
            m &= x <= p["hi"]
    return m


def agg_values(aggs, m):
    """numpy value of each aggregate over the rows of mask m (NULL inputs
    skipped, Spark semantics)."""
    out = []
    for kind, factors in aggs:
        if kind == "count":
            out.append(float(m.sum()))
            continue
        ok = m.copy()
        v = np.ones(N)
        for col, add, mul in factors:
            ok &= VALID[col]
            v = v * (add + mul * COLS[col].astype(np.float64))
        x = v[ok]
        assert len(x) > 0
        out.append(float({"sum": x.sum(), "avg": x.sum() / len(x),
                          "min": x.min(), "max": x.max()}[kind]))
    return out


def ref_groups(mask, keycols, aggs):
    """{key tuple: [agg values]}; keycols are per-row object arrays."""
    out = {}
    for key in sorted({tuple(k[r] for k in keycols)
                       for r in np.nonzero(mask)[0]}, key=repr):
        m = mask.copy()
        for k, kv in zip(keycols, key):
            m &= np.array([x == kv for x in k]) if kv is None else (k == kv)
        out[key] = agg_values(aggs, m)
    return out


def int_keys(col):
    return np.array([str(int(v)) if ok else None
                     for v, ok in zip(COLS[col], VALID[col])], dtype=object)


SUM = lambda c: ("sum", [(c, 0.0, 1.0)])            # noqa: E731
AVG = lambda c: ("avg", [(c, 0.0, 1.0)])            # noqa: E731
COUNT = ("count", [])

# dimension for the join cases: the even keys, four attribute values
DIM_KEYS = np.arange(0, 100, 2, dtype=np.int64)
DIM_ATTRS = [b"A%d" % (int(k) // 2 % 4) for k in DIM_KEYS]
# build-side column table of the colocated join: 1100 rows (one full chunk
# and a ragged one), of which the even keys below 100 meet the fact table
BUILD_KEYS = np.arange(0, 2200, 2, dtype=np.int32)
BUILD_ATTRS = [b"B%d" % (int(k) // 2 % 5) for k in BUILD_KEYS]


def dim_semi(eng, name):
    d = eng.dim_define(name)
    eng.dim_put(d, DIM_KEYS)
    return d


def dim_attr(eng, name):
    d = eng.dim_define(name)
    eng.dim_put(d, DIM_KEYS, DIM_ATTRS)
    return d


def dim_colocated(eng, name):
    bt = eng.table_define(name + "_build", [(abi.T_INT32, False), (abi.T_STRING, False)])
    n = len(BUILD_KEYS)
    assert eng.ingest_columns(
        bt, [{"data": BUILD_KEYS},
             {"data": b"".join(BUILD_ATTRS),
              "lens": np.array([len(a) for a in BUILD_ATTRS], dtype=np.int32)}],
        n, batch_rows=n) == n
    d = eng.dim_define(name)
    eng.dim_from_table(d, bt, key_col=0, attr_col=1)
    return d


def attr_keys(keys, attrs):
    lut = {int(k): a.decode() for k, a in zip(keys, attrs)}
    return np.array([lut.get(int(k)) for k in COLS[C_JK]], dtype=object)


JOINED = np.isin(COLS[C_JK], DIM_KEYS)

# id -> (preds beyond the F filter, group cols, aggs, join or None)
# join: (dimension builder, group-by-attr?, per-row attr keys)
CASES = {
    # k_keyless<2,4>, sweep row phase on batch 1, fused on batch 0
    "keyless_2aggs": ([], [], [SUM(C_D0), COUNT], None),
    # k_keyless<12,8>; 5..8 aggregates share the 8-wide result row, which
    # the 12-wide kernel instance has to honour when it writes its partials
    "keyless_5aggs_5cols": (
        [], [], [SUM(C_D0), SUM(C_D1), SUM(C_D2), SUM(C_D3),
                 ("sum", [(C_D0, 0.0, 1.0), (C_D1, 1.0, 1.0)])], None),
    "keyless_3dpreds_fused": (
        [dict(col=C_D0, is_double=True, hi=5.0),
         dict(col=C_D1, is_double=True, lo=1.0)],
        [], [SUM(C_D2), COUNT], None),
    "keyless_3dpreds_ipred_sweep": (
        [dict(col=C_D0, is_double=True, hi=5.0),
         dict(col=C_D1, is_double=True, lo=1.0), dict(col=C_I, hi=7)],
        [], [SUM(C_D2), COUNT], None),
    # k_grouped_reg<8,6,*>
    "grouped_reg_6slots": ([], [C_G6], [SUM(C_D0), SUM(C_D1), AVG(C_D2), COUNT],
                           None),
    # k_grouped<16,*>
    "grouped_12slots": ([], [C_G12], [SUM(C_D0), SUM(C_D1), AVG(C_D2), COUNT],
                        None),
    # k_grouped_lds
    "grouped_lds_40slots": ([], [C_G40], [SUM(C_D0), AVG(C_D1), COUNT], None),
    # pac rows through k_grouped_lds
    "grouped_pac_null_input": ([], [C_G3], [SUM(C_N), AVG(C_N), SUM(C_D0), COUNT],
                               None),
    # one-slot pac route
    "keyless_min_max": ([], [], [("min", [(C_D0, 3.0, 1.0)]),
                                 ("max", [(C_D1, 0.0, 2.0)]), COUNT], None),
    # k_grouped_global
    "grouped_global_1500keys": ([], [C_G1500], [SUM(C_D0), COUNT], None),
    # k_grouped_hash
    "sparse_int64_keys": ([], [C_K64], [SUM(C_D0), AVG(C_D1), COUNT], None),
    "semi_join": ([], [], [SUM(C_D0), COUNT], (dim_semi, False, None)),
    "join_group_attr": ([], [], [SUM(C_D0), COUNT],
                        (dim_attr, True, attr_keys(DIM_KEYS, DIM_ATTRS))),
    "join_group_attr_x_fact": ([], [C_G3], [SUM(C_D0), COUNT],
                               (dim_attr, True, attr_keys(DIM_KEYS, DIM_ATTRS))),
    # k_join_build, then the probe
    "colocated_join": ([], [], [SUM(C_D0), COUNT],
                       (dim_colocated, True,
                        attr_keys(BUILD_KEYS, BUILD_ATTRS))),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_interpreted_route(loaded, case):
    eng, t = loaded
    preds, group_cols, aggs, join = CASES[case]
    preds = [F_PRED] + preds
    mask = pred_mask(preds)
    keycols = []
    jspec = None
    if join is not None:
        mkdim, by_attr, akeys = join
        jspec = dict(dim=mkdim(eng, case), fact_col=C_JK, group=by_attr)
        if akeys is None:
            mask &= JOINED
        else:
            mask &= np.array([a is not None for a in akeys])
            keycols.append(akeys)
    keycols += [int_keys(c) for c in group_cols]
    exp = ref_groups(mask, keycols, aggs)

    q = eng.query(abi.make_plan(table=t, preds=preds, group_cols=group_cols,
                                aggs=aggs, join=jspec))
    rows = q.rows()
    assert not q.used_jit()
    got = {keys: vals for keys, vals in rows}
    assert len(rows) == len(got) == len(exp) > 0
    # a sparse row that met a full table is retried, never dropped
    assert q.num_groups() == len(exp)
    assert got == exp
    q.close()


# ---------------------------------------------------------------- decimal


def py_avg(total, count):
    """Python-int avg at scale + 4, HALF_UP."""
    q, r = divmod(abs(total) * 10 ** 4, count)
    if 2 * r >= count:
        q += 1
    return -q if total < 0 else q


DEC_AGGS = [("sum", [(C_DA, 0, 1)]),
            ("sum", [(C_DA, 0, 1), (C_DB, 100, -1)]),
            ("min", [(C_DA, 0, 1)]),
            ("max", [(C_DA, 0, 1)]),
            ("avg", [(C_DA, 0, 1)]),
            ("count", [])]


def dec_values(m):
    a = [int(v) for v in COLS[C_DA][m]]
    b = [int(v) for v in COLS[C_DB][m]]
    return [sum(a), sum(x * (100 - y) for x, y in zip(a, b)), min(a), max(a),
            py_avg(sum(a), len(a)), len(a)]


@pytest.mark.parametrize("group_cols", [[], [C_G3]],
                         ids=["dec_keyless", "dec_grouped"])
def test_interpreted_route_decimal(loaded, group_cols):
    """k_dec_keyless / k_dec_grouped (never query-compiled)."""
    eng, t = loaded
    mask = pred_mask([F_PRED])
    plan, aggs = abi.make_dec_plan(table=t, preds=[F_PRED],
                                   group_cols=group_cols, aggs=DEC_AGGS)
    q = eng.query_dec(plan, aggs)
    rows = q.dec_rows()
    assert not q.used_jit()
    if group_cols:
        g = COLS[C_G3]
        exp = {(str(k),): dec_values(mask & (g == k)) for k in range(3)}
    else:
        exp = {(): dec_values(mask)}
    assert {keys: vals for keys, vals, _ in rows} == exp
    assert len(rows) == len(exp)
    for _, _, scales in rows:
        assert scales == [2, 4, 2, 2, 6, 0]
    q.close()
