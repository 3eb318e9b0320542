"""Row scans over a dimension join (sn_scan_submit_join) on the device: inner,
left outer and left anti, against the numpy reference of
tests/select_join_cases.py over tests/join_cases.py's data.  Every assertion
is `==` on bytes: ROWID, the projected fact columns, the attribute bytes
(through sn_dim_attr_value) and the validity arrays."""
import ctypes as C

import numpy as np
import pytest

from snappydata_amd import abi, engine as se
from tests import join_cases as jc
from tests import select_join_cases as sj
from tests.test_join_probe_routes import build_table, load_fact

pytestmark = pytest.mark.gpu

INNER, OUTER, ANTI = sj.INNER, sj.OUTER, sj.ANTI
A = abi.PROJ_DIM_ATTR

DIMSETS = [jc.HASH_WIDE, jc.HASH_CHAIN, jc.EXTREME, jc.ATTR15,
           jc.LUT_EDGES[(204800, -100000)], jc.LUT_EDGES[((1 << 24) + 1, 0)]]
assert [d.lut for d in DIMSETS] == [False, False, False, True, True, False]
COL_NAMES = {jc.C_K32: "k32", jc.C_K64: "k64", jc.C_KN64: "kn64",
             jc.C_KN32: "kn32"}
ROUTE_CASES = [(d, kc, interp) for d in DIMSETS for kc in d.key_cols()
               for interp in (False, True)]
BUILD_CASES = [(b, kc, interp) for b in ("null_keys", "stale_bounds")
               for kc in jc.BUILD_FACT[b].key_cols() for interp in (False, True)]


def case_id(c):
    d, kc, interp = c
    return "%s-%s-%s" % (d if isinstance(d, str) else d.name, COL_NAMES[kc],
                         "general" if interp else "clean")


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        a.tobytes() == b.tobytes()


class Shared:
    """one engine; fact tables and dimensions made once, read-only after"""

    def __init__(self):
        self.eng = se.Engine(device=0)
        self.tables, self.dims = {}, {}

    def fact(self, dimset, interp):
        key = (dimset.name, interp)
        if key not in self.tables:
            fx = jc.fact(dimset, interp)
            t = load_fact(self.eng, fx, "sj_%s_%d" % key)
            self.tables[key] = (t, sj.Table.from_fact(fx))
        return self.tables[key]

    def put_dim(self, dimset):
        """(handle, keys, attrs) of a sn_dim_put dimension with attributes"""
        if dimset.name not in self.dims:
            d = self.eng.dim_define("sjd_" + dimset.name)
            attrs = dimset.attrs()
            self.eng.dim_put(d, np.array(dimset.keys, dtype=np.int64), attrs)
            self.dims[dimset.name] = (d, dimset.keys, attrs)
        return self.dims[dimset.name]

    def built_dim(self, name):
        """... of a sn_dim_from_table dimension, attribute column included"""
        if name not in self.dims:
            b = jc.BUILDS[name]
            bt = build_table(self.eng, b, "sjb_" + name)
            d = self.eng.dim_define("sjd_" + name)
            self.eng.dim_from_table(d, bt, key_col=0, attr_col=1)
            keys, attrs = b.effective()
            self.dims[name] = (d, keys, attrs)
        return self.dims[name]


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.eng.close()


def run(eng, t, d, key_col, jtype, cols=None, preds=(jc.F_PRED,), **kw):
    plan = abi.make_plan(table=t, preds=list(preds),
                         join=dict(dim=d, fact_col=key_col))
    return eng.select(plan, sj.projection(jtype, key_col) if cols is None
                      else cols, join_type=jtype, **kw)


def check(rs, exp, jtype, passed_rows=None):
    """rs projects sj.projection(jtype, key): compare every column with exp"""
    assert rs.count() == len(exp)
    assert rs.rows_passed() == (len(exp) if passed_rows is None
                                else passed_rows)
    rowid, v = rs.column(0)
    assert v.all() and same_bytes(rowid, exp.rowid)
    d0, v = rs.column(1)
    assert v.all() and same_bytes(d0, exp.d0)
    key, kv = rs.column(2)
    assert same_bytes(kv, exp.key_valid) and same_bytes(key, exp.key)
    if jtype == ANTI:
        assert len(rs.cols) == 3
        return
    ids, av = rs.column(3)
    assert ids.dtype == np.int32
    assert same_bytes(av, exp.attr_valid)
    assert not ids[~av].any()                   # a NULL's value bytes are 0
    assert rs.strings(3) == exp.attr


def check_three(eng, t, tb, d, keys, attrs, key_col):
    """all three types of one (table, dimension, key column), and what must
    hold between them"""
    exp = {jt: sj.Rows(tb, key_col, keys, attrs, jt) for jt in sj.TYPES}
    got = {}
    for jt in sj.TYPES:
        rs = run(eng, t, d, key_col, jt)
        check(rs, exp[jt], jt)
        got[jt] = rs.column(0)[0]
        if jt == INNER:
            assert rs.column(3)[1].all()        # no NULL attribute
            assert len(exp[jt]) > 0
        if jt == OUTER:
            passed, joined = exp[jt].passed, exp[jt].joined
            assert rs.count() == int(passed.sum())
            assert same_bytes(rs.column(3)[1], joined[passed])
        rs.close()
    inner, anti = set(got[INNER].tolist()), set(got[ANTI].tolist())
    assert not inner & anti
    assert sorted(inner | anti) == got[OUTER].tolist()
    assert len(got[ANTI]) > 0


@pytest.mark.parametrize("case", ROUTE_CASES, ids=case_id)
def test_route_type_key(case, shared):
    dimset, key_col, interp = case
    d, keys, attrs = shared.put_dim(dimset)
    t, tb = shared.fact(dimset, interp)
    check_three(shared.eng, t, tb, d, keys, attrs, key_col)


@pytest.mark.parametrize("case", BUILD_CASES, ids=case_id)
def test_device_built_dimension(case, shared):
    name, key_col, interp = case
    d, keys, attrs = shared.built_dim(name)
    assert shared.eng.dim_num_attrs(d) >= len(set(attrs))
    t, tb = shared.fact(jc.BUILD_FACT[name], interp)
    check_three(shared.eng, t, tb, d, keys, attrs, key_col)


def test_int64_min_fact_value_never_joins(shared):
    """HASH_WIDE's fact draws INT64_MIN, the table's empty mark"""
    d, keys, attrs = shared.put_dim(jc.HASH_WIDE)
    t, tb = shared.fact(jc.HASH_WIDE, False)
    at = np.nonzero(tb.cols[jc.C_K64] == jc.I64_MIN)[0]
    assert len(at) > 0
    rowids = set(tb.rowid[at].tolist())
    got = {jt: set(run(shared.eng, t, d, jc.C_K64, jt).column(0)[0].tolist())
           for jt in sj.TYPES}
    assert not rowids & got[INNER]
    assert rowids <= got[ANTI] and rowids <= got[OUTER]


@pytest.mark.parametrize("key_col", [jc.C_K64, jc.C_KN64],
                         ids=["k64", "kn64"])
def test_both_passes_read_the_patched_key(shared, key_col):
    """an update delta on the key column and a delete mask on batch 0: rows
    move from a dimension key to a near miss and back, and pass 2's attribute
    is the one of the key pass 1 probed"""
    eng = shared.eng
    dimset = jc.ATTR15
    d, keys, attrs = shared.put_dim(dimset)
    fx = jc.fact(dimset, True)
    t = load_fact(eng, fx, "sj_patched_%d" % key_col)
    tb = sj.Table.from_fact(fx)
    n0 = jc.SIZES[0]
    col, ok = tb.cols[key_col], tb.valid[key_col]
    hit = np.isin(col[:n0], np.array(keys, dtype=np.int64)) & ok[:n0]
    away = np.nonzero(hit)[0][3:43]              # key -> key + 1: a near miss
    back = np.nonzero(~hit & ok[:n0])[0][2:42]   # near miss -> a key
    assert len(away) == 40 and len(back) == 40
    newv = col.copy()
    newv[away] = col[away] + 1
    newv[back] = np.array(keys, dtype=np.int64)[np.arange(40) % len(keys)]
    assert not np.isin(newv[away], np.array(keys, dtype=np.int64)).any()
    pos = np.sort(np.concatenate([away, back])).astype(np.int32)
    deltas = [(None, None)] * len(jc.SCHEMA)
    deltas[key_col] = (se.encode_update_delta(abi.T_INT64, pos, n0, newv[pos]),
                       None)
    dels = np.array(sorted({int(away[0]), int(back[0]), 0, 63, 64, n0 - 1}),
                    dtype=np.int32)
    eng.batch_mutate(t, *eng.batch_id(t, 0), delete_mask=se.encode_delete_mask(
        dels, n0), deltas=deltas)
    tb.cols[key_col] = newv
    tb.deleted[dels] = True
    check_three(eng, t, tb, d, keys, attrs, key_col)


@pytest.mark.parametrize("jtype", [INNER, OUTER], ids=["inner", "outer"])
def test_limit_is_a_prefix(shared, jtype):
    eng = shared.eng
    d, keys, attrs = shared.put_dim(jc.HASH_WIDE)
    t, tb = shared.fact(jc.HASH_WIDE, True)
    exp = sj.Rows(tb, jc.C_KN64, keys, attrs, jtype)
    total = len(exp)
    in0 = int((exp.index < jc.SIZES[0]).sum())
    assert 2 < in0 < total - 2
    for limit in (1, in0 - 1, in0, in0 + 1, total - 1, total + 5):
        rs = run(eng, t, d, jc.C_KN64, jtype, limit=limit)
        check(rs, exp.take(np.arange(min(limit, total))), jtype,
              passed_rows=total)
        rs.close()


@pytest.mark.parametrize("order_col", [jc.C_D0, jc.C_KN64], ids=["d0", "kn64"])
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("jtype", [INNER, OUTER], ids=["inner", "outer"])
def test_ordered(shared, jtype, desc, order_col):
    """ORDER BY a fact column LIMIT 100 over the join; C_D0 has eight values,
    so ties (kept in scan order) are everywhere; the nullable key column puts
    NULLs first ascending and last descending"""
    eng = shared.eng
    d, keys, attrs = shared.put_dim(jc.ATTR15)
    t, tb = shared.fact(jc.ATTR15, True)
    exp = sj.Rows(tb, jc.C_KN64, keys, attrs, jtype)
    assert len(exp) > 100
    ix = exp.index
    order = sj.stable_order(tb.cols[order_col][ix], tb.valid[order_col][ix],
                            desc)
    rs = run(eng, t, d, jc.C_KN64, jtype, order_by=order_col, descending=desc,
             limit=100)
    check(rs, exp.take(order[:100]), jtype, passed_rows=len(exp))
    rs.close()


def test_two_tiles(shared):
    """one batch of 16384 + 1024 + 5 rows (two tiles), no predicate: the
    per-tile counts and offsets after the join"""
    eng = shared.eng
    n = 16384 + 1024 + 5
    key = (np.arange(n) % 7).astype(np.int32)
    t = eng.table_define("sj_tiles", [(abi.T_INT32, False)])
    assert eng.ingest_columns(t, [{"data": key}], n, batch_rows=n) == n
    d = eng.dim_define("sjd_tiles")
    dkeys, dattrs = [0, 3, 6], [b"zero", b"three", b"six"]
    eng.dim_put(d, np.array(dkeys, dtype=np.int64), dattrs)
    joined = np.isin(key, dkeys)
    attr_of = dict(zip(dkeys, dattrs))
    first_tile = int(joined[:16384].sum())
    for jtype, keep, limit in [(INNER, joined, 0), (OUTER, joined | True, 0),
                               (ANTI, ~joined, 0),
                               (INNER, joined, first_tile + 10)]:
        ix = np.nonzero(keep)[0]
        total = len(ix)
        if limit:
            ix = ix[:limit]
        cols = [abi.PROJ_ROWID, 0] + ([] if jtype == ANTI else [A])
        rs = eng.select(abi.make_plan(table=t, join=dict(dim=d, fact_col=0)),
                        cols, join_type=jtype, limit=limit)
        assert rs.count() == len(ix) and rs.rows_passed() == total
        rowid, v = rs.column(0)
        assert v.all() and same_bytes(rowid, ix.astype(np.int64))
        k, v = rs.column(1)
        assert v.all() and same_bytes(k, key[ix])
        if jtype != ANTI:
            assert same_bytes(rs.column(2)[1], joined[ix])
            assert rs.strings(2) == [attr_of.get(int(x)) for x in key[ix]]
        rs.close()


def test_semi_join_on_a_dimension_without_attributes(shared):
    """INNER with no attribute projected is the left semi join; it needs no
    attributes on the dimension"""
    eng = shared.eng
    dimset = jc.EXTREME
    t, tb = shared.fact(dimset, False)
    d = eng.dim_define("sjd_noattr")
    eng.dim_put(d, np.array(dimset.keys, dtype=np.int64))
    assert eng.dim_num_attrs(d) == 0
    for jtype in (INNER, ANTI):
        exp = sj.Rows(tb, jc.C_K64, dimset.keys, [None] * 3, jtype)
        rs = run(eng, t, d, jc.C_K64, jtype,
                 cols=[abi.PROJ_ROWID, jc.C_D0, jc.C_K64])
        check(rs, exp, ANTI)                    # three columns, no attribute
        rs.close()


def test_handle_contract(shared):
    eng = shared.eng
    d, keys, attrs = shared.put_dim(jc.ATTR15)
    t, tb = shared.fact(jc.ATTR15, False)
    rs = run(eng, t, d, jc.C_K32, INNER)
    assert rs.count() == len(sj.Rows(tb, jc.C_K32, keys, attrs, INNER))
    assert rs.kernel_ms() > 0
    assert all(ms > 0 for ms in rs.kernel_ms_parts())
    assert rs.used_jit() is False and rs.late_cols() == []
    res = rs.result()
    assert res.nrows == 0 and res.naggs == 0 and res.rows_scanned == jc.N
    L_ = se.lib()
    res = abi.SnResult()
    dv = abi.SnDecVal()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    U = abi.ERR_UNSUPPORTED
    assert L_.sn_query_result_page(rs._h, 0, C.byref(res)) == U
    assert L_.sn_query_order_by(rs._h, 0, 0, 0) == U
    assert L_.sn_query_partial_bytes(rs._h) == U
    assert L_.sn_query_partial_bytes2(rs._h, 4) == U
    assert L_.sn_query_partials(rs._h, buf.ctypes.data, 0) == U
    assert L_.sn_query_partials2(rs._h, buf.ctypes.data, 0, 4) == U
    assert L_.sn_query_partials_sharded(rs._h, 2, buf.ctypes.data) == U
    assert L_.sn_query_merge(rs._h, buf.ctypes.data, 8, 1) == U
    assert L_.sn_query_result_dec(rs._h, 0, 0, C.byref(dv)) == U
    assert L_.sn_query_wait(rs._h) == 0
    # a fetch outside the rows is refused, the attribute column like any other
    n = rs.count()
    vals = np.zeros(4, dtype=np.int32)
    assert L_.sn_rows_fetch(rs._h, 3, n - 1, 2, vals.ctypes.data, None, 0) == \
        abi.ERR_BADARG
    rs.close()
    # the plain scans on the same table still refuse the join plan, and a
    # plain select of the same columns is not served the join's descriptors
    plan = abi.make_plan(table=t, preds=[jc.F_PRED],
                         join=dict(dim=d, fact_col=jc.C_K32))
    with pytest.raises(se.EngineError) as ei:
        eng.select(plan, [jc.C_D0])
    assert ei.value.code == abi.ERR_UNSUPPORTED
    ps = eng.select(abi.make_plan(table=t, preds=[jc.F_PRED]),
                    [abi.PROJ_ROWID, jc.C_D0, jc.C_K32])
    check(ps, sj.Rows(tb, jc.C_K32, keys, attrs, OUTER), ANTI)
    ps.close()
