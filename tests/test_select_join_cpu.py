"""Row scans over a dimension join (sn_scan_submit_join), host side (no GPU):
the new symbols resolve, every submit-time rejection fires with its own status
code, in the header's order, before the engine asks for a device — a
well-formed plan then fails with SN_ERR_NOGPU — and the two dimension
attribute calls answer from host state alone."""
import ctypes as C

import numpy as np
import pytest

from snappydata_amd import abi, engine as se

NEW_SYMBOLS = ["sn_scan_submit_join", "sn_dim_num_attrs", "sn_dim_attr_value",
               "sn_launch_select_mark_join"]
INNER, OUTER, ANTI = abi.RJOIN_INNER, abi.RJOIN_LEFT_OUTER, abi.RJOIN_LEFT_ANTI


@pytest.fixture
def eng():
    e = se.Engine(device=-1)
    yield e
    e.close()


def define(eng, ncols=11):
    """col 0 int32, 1 double, 2 string, 3 int64, the rest int32"""
    schema = [(abi.T_INT32, False), (abi.T_DOUBLE, False),
              (abi.T_STRING, True), (abi.T_INT64, True)] + \
        [(abi.T_INT32, False)] * (ncols - 4)
    return eng.table_define("selj_t", schema)


def dims(eng):
    """(with attributes, without, empty)"""
    da = eng.dim_define("with_attrs")
    eng.dim_put(da, np.array([1, 2, 3, 4], dtype=np.int64),
                [b"x", b"yy", b"x", b"zzz"])
    dn = eng.dim_define("no_attrs")
    eng.dim_put(dn, np.array([1, 2], dtype=np.int64))
    return da, dn, eng.dim_define("empty")


def plan_of(t, dim, fact_col=0, preds=(dict(col=0, lo=1, hi=2),), **kw):
    return abi.make_plan(table=t, preds=list(preds),
                         join=dict(dim=dim, fact_col=fact_col), **kw)


def code(eng, plan, cols, join_type=INNER, **kw):
    with pytest.raises(se.EngineError) as ei:
        eng.select(plan, cols, join_type=join_type, **kw)
    assert se.last_error()
    return ei.value.code


def raw_code(eng, plan, join_type, cols, order_col, flags, limit):
    arr = (C.c_int32 * max(len(cols), 1))(*cols)
    L = se.lib()
    assert not L.sn_scan_submit_join(eng._h, C.byref(plan), join_type,
                                     len(cols), arr, order_col, flags, limit)
    return L.sn_last_error_code()


def test_new_symbols_resolve():
    lib = se.lib()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name, None) is not None, name
    assert abi.PROJ_DIM_ATTR == -2 and abi.ORDER_NONE == -1
    assert (INNER, OUTER, ANTI) == (0, 1, 2)
    for attr in ("dim_num_attrs", "dim_attr_value"):
        assert callable(getattr(se.Engine, attr))


def test_rejections_in_order_then_nogpu(eng):
    t = define(eng)
    da, dn, dempty = dims(eng)
    A = abi.PROJ_DIM_ATTR
    L = se.lib()
    one = (C.c_int32 * 1)(1)
    good = plan_of(t, da)
    # 1. sn_scan_submit's checks, with their codes.  Each plan below is also
    # wrong further down the list (join type 7), so the code shows the order.
    assert not L.sn_scan_submit_join(None, C.byref(good), 7, 1, one, -1, 0, 0)
    assert L.sn_last_error_code() == abi.ERR_BADARG
    assert not L.sn_scan_submit_join(eng._h, None, 7, 1, one, -1, 0, 0)
    assert L.sn_last_error_code() == abi.ERR_BADARG
    assert not L.sn_scan_submit_join(eng._h, C.byref(good), 7, 1, None, -1, 0, 0)
    assert L.sn_last_error_code() == abi.ERR_BADARG
    p = plan_of(t, da)
    p.table = 5
    assert code(eng, p, [1]) == abi.ERR_BADARG
    assert code(eng, plan_of(t, da, aggs=[("count", [])]), [1]) == abi.ERR_BADARG
    assert code(eng, plan_of(t, da, group_cols=[2]), [1]) == abi.ERR_BADARG
    p = plan_of(t, da)
    p.npreds = abi.SN_MAX_PREDS + 1
    assert code(eng, p, [1], join_type=7) == abi.ERR_BADARG
    assert code(eng, good, [], join_type=7) == abi.ERR_BADARG
    assert code(eng, good, [0] * 9, join_type=7) == abi.ERR_BADARG
    # 2. join type (the dimension below is also unknown)
    p = plan_of(t, 9)
    assert code(eng, p, [1], join_type=3) == abi.ERR_BADARG
    assert code(eng, p, [1], join_type=-1) == abi.ERR_BADARG
    # 3. no join, or an unknown dimension (the mode below is also wrong)
    p = abi.make_plan(table=t, preds=[dict(col=0, lo=1)])
    assert p.join_dim == -1
    p.join_mode = 1
    assert code(eng, p, [1]) == abi.ERR_BADARG
    for bad_dim in (9, -3):
        p = plan_of(t, bad_dim)
        p.join_mode = 1
        assert code(eng, p, [1]) == abi.ERR_BADARG
    # 4. join mode (the dimension below is also empty): the UNSUPPORTED of a
    # later check would show a wrong order
    p = plan_of(t, dempty, fact_col=1)
    p.join_mode = 1
    assert code(eng, p, [1]) == abi.ERR_BADARG
    # 5. empty dimension (the key column is also a double)
    assert code(eng, plan_of(t, dempty, fact_col=1), [1]) == abi.ERR_BADARG
    # 6. key column outside the schema
    assert code(eng, plan_of(t, da, fact_col=11), [1]) == abi.ERR_BADARG
    assert code(eng, plan_of(t, da, fact_col=-1), [1]) == abi.ERR_BADARG
    assert code(eng, plan_of(t, da, fact_col=64), [1]) == abi.ERR_BADARG
    # 7. key column type (the projection is also bad)
    for c in (1, 2):
        assert code(eng, plan_of(t, da, fact_col=c), [77]) == abi.ERR_UNSUPPORTED
    # 8. columns: a bad ordinal; the attribute under LEFT_ANTI or on a
    # dimension without attributes; a ninth distinct column, the key counting
    # (each also has a bad order column behind it)
    assert code(eng, good, [1, 11], order_by=99, limit=5) == abi.ERR_BADARG
    assert code(eng, good, [-3], order_by=99, limit=5) == abi.ERR_BADARG
    bad = plan_of(t, da, preds=[dict(col=11, lo=1)])
    assert code(eng, bad, [1], order_by=99, limit=5) == abi.ERR_BADARG
    assert code(eng, good, [1, A], join_type=ANTI, order_by=99, limit=5) == \
        abi.ERR_BADARG
    assert code(eng, plan_of(t, dn), [1, A], order_by=99, limit=5) == \
        abi.ERR_BADARG
    assert code(eng, plan_of(t, dn), [1, A], join_type=OUTER) == abi.ERR_BADARG
    # predicate and key column 0, then 1..8: nine
    assert code(eng, good, list(range(1, 9)), order_by=99, limit=5) == \
        abi.ERR_UNSUPPORTED
    # predicate column 0, key column 3, then seven others: nine
    p3 = plan_of(t, da, fact_col=3)
    for jt in (INNER, OUTER, ANTI):
        assert code(eng, p3, [1, 2, 4, 5, 6, 7, 8], join_type=jt) == \
            abi.ERR_UNSUPPORTED
    # 9. the order checks, as in sn_scan_submit_ordered
    assert code(eng, good, [1], order_by=abi.PROJ_DIM_ATTR, limit=5) == \
        abi.ERR_BADARG
    assert code(eng, good, [1], order_by=11, limit=5) == abi.ERR_BADARG
    assert raw_code(eng, good, INNER, [1], 1, 8, 5) == abi.ERR_BADARG
    assert raw_code(eng, good, INNER, [1], 1, abi.ORDER_NULLS_FIRST |
                    abi.ORDER_NULLS_LAST, 5) == abi.ERR_BADARG
    assert code(eng, good, [1], order_by=1, limit=0) == abi.ERR_BADARG
    assert code(eng, good, [1], order_by=1,
                limit=abi.ORDER_MAX_LIMIT + 1) == abi.ERR_UNSUPPORTED
    # the key is the ninth: predicate/key 0, projections 1..7, order key 8
    assert code(eng, good, list(range(1, 8)), order_by=8, limit=5) == \
        abi.ERR_UNSUPPORTED
    # SN_ORDER_NONE takes no flags
    assert raw_code(eng, good, INNER, [1], abi.ORDER_NONE, abi.ORDER_DESC, 5) == \
        abi.ERR_BADARG
    # 10. well-formed: no device
    for plan, cols, kw in [
            (good, [1], {}),
            (good, [abi.PROJ_ROWID, 1, 0, A], dict(limit=7)),
            (good, [A], dict(join_type=OUTER)),
            (good, [abi.PROJ_ROWID, 0], dict(join_type=ANTI)),
            (plan_of(t, dn), [1], {}),                       # semi join
            (plan_of(t, dn), [1], dict(join_type=ANTI)),
            (p3, [1, 2, 4, 5, 6, 7, A, 3], dict(join_type=OUTER)),   # eight
            (plan_of(t, da, preds=()), [A], dict(join_type=OUTER)),
            (good, [1, A], dict(order_by=1, limit=5, descending=True)),
            (good, [A], dict(order_by=3, limit=abi.ORDER_MAX_LIMIT,
                             nulls_first=False, join_type=OUTER)),
            (good, list(range(1, 7)), dict(order_by=9, limit=1))]:
        kw = dict(kw)
        jt = kw.pop("join_type", INNER)
        assert code(eng, plan, cols, join_type=jt, **kw) == abi.ERR_NOGPU, \
            (cols, kw)


def test_plain_scans_still_refuse_a_join(eng):
    t = define(eng)
    da, _dn, _de = dims(eng)
    p = plan_of(t, da)
    for kw in (dict(), dict(order_by=1, limit=5)):
        with pytest.raises(se.EngineError) as ei:
            eng.select(p, [1], **kw)
        assert ei.value.code == abi.ERR_UNSUPPORTED
    # and the attribute pseudo-column is no column of theirs
    with pytest.raises(se.EngineError) as ei:
        eng.select(abi.make_plan(table=t), [abi.PROJ_DIM_ATTR])
    assert ei.value.code == abi.ERR_BADARG


def test_dim_attrs(eng):
    da, dn, dempty = dims(eng)
    assert eng.dim_num_attrs(da) == 3
    assert [eng.dim_attr_value(da, i) for i in range(3)] == [b"x", b"yy", b"zzz"]
    assert eng.dim_num_attrs(dn) == 0
    assert eng.dim_num_attrs(dempty) == 0
    L = se.lib()
    # the length alone, a buffer that is too small, an exact fit, room for NUL
    assert L.sn_dim_attr_value(eng._h, da, 2, None, 0) == 3
    buf = C.create_string_buffer(b"????", 4)
    assert L.sn_dim_attr_value(eng._h, da, 2, buf, 2) == abi.ERR_BADARG
    assert L.sn_last_error_code() == abi.ERR_BADARG
    assert buf.raw == b"????"
    assert L.sn_dim_attr_value(eng._h, da, 2, buf, -1) == abi.ERR_BADARG
    assert L.sn_dim_attr_value(eng._h, da, 2, buf, 3) == 3
    assert buf.raw == b"zzz?"
    assert L.sn_dim_attr_value(eng._h, da, 1, buf, 4) == 2
    assert buf.raw == b"yy\0?"
    for dim, aid in [(9, 0), (-1, 0), (da, 3), (da, -1), (dn, 0), (dempty, 0)]:
        with pytest.raises(se.EngineError) as ei:
            eng.dim_attr_value(dim, aid)
        assert ei.value.code == abi.ERR_BADARG, (dim, aid)
    for dim in (9, -1):
        with pytest.raises(se.EngineError) as ei:
            eng.dim_num_attrs(dim)
        assert ei.value.code == abi.ERR_BADARG
    assert L.sn_dim_num_attrs(None, 0) == abi.ERR_BADARG
    assert L.sn_dim_attr_value(None, 0, 0, None, 0) == abi.ERR_BADARG
    # a later put extends the dictionary; earlier ids keep their meaning
    eng.dim_put(da, np.array([9], dtype=np.int64), [b"new"])
    assert eng.dim_num_attrs(da) == 4
    assert eng.dim_attr_value(da, 3) == b"new"
    assert eng.dim_attr_value(da, 0) == b"x"
