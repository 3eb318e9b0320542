"""Row-returning filter scan (sn_scan_submit), host side (no GPU): the new
entry points resolve, and every submit-time rejection fires with its own
status code before the engine asks for a device — a well-formed plan then
fails with SN_ERR_NOGPU, never a CPU fallback."""
import ctypes as C

import numpy as np
import pytest

from snappydata_amd import abi, engine as se

NEW_SYMBOLS = ["sn_scan_submit", "sn_rows_count", "sn_rows_fetch",
               "sn_table_dict_value", "sn_table_batch_id",
               "sn_launch_tile_offsets"]


@pytest.fixture
def eng():
    e = se.Engine(device=-1)
    yield e
    e.close()


def define(eng, ncols=10):
    """col 0 int32, 1 double, 2 string, the rest int32"""
    schema = [(abi.T_INT32, False), (abi.T_DOUBLE, False),
              (abi.T_STRING, True)] + [(abi.T_INT32, False)] * (ncols - 3)
    return eng.table_define("sel_t", schema)


def put_one_batch(eng, t, uuid=77, bucket=3):
    n = 4
    cols = [se.encode_column(abi.T_INT32, np.arange(n, dtype=np.int32)),
            se.encode_column(abi.T_DOUBLE, np.arange(n, dtype=np.float64))]
    s = [b"aa", b"b", b"aa", b"ccc"]
    cols.append(se.encode_column(abi.T_STRING, b"".join(s),
                                 lens=np.array([len(x) for x in s], np.int32)))
    cols += [se.encode_column(abi.T_INT32, np.zeros(n, dtype=np.int32))] * 7
    eng.batch_put(t, uuid, bucket, n, cols)
    return s


def select_code(eng, plan, cols, limit=0):
    with pytest.raises(se.EngineError) as ei:
        eng.select(plan, cols, limit)
    assert se.last_error()
    return ei.value.code


def test_new_symbols_resolve():
    lib = se.lib()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name, None) is not None, name
    assert abi.PROJ_ROWID == -1
    for attr in ("select", "batch_id", "dict_value"):
        assert callable(getattr(se.Engine, attr))
    for attr in ("count", "column", "strings", "rowids", "wait", "kernel_ms",
                 "close"):
        assert callable(getattr(se.RowSet, attr))


def test_select_rejections_then_nogpu(eng):
    t = define(eng)
    pred = [dict(col=0, lo=1, hi=2)]
    # aggregates or group columns do not belong in a row-returning plan
    p = abi.make_plan(table=t, preds=pred, aggs=[("count", [])])
    assert select_code(eng, p, [1]) == abi.ERR_BADARG
    p = abi.make_plan(table=t, preds=pred, group_cols=[2])
    assert select_code(eng, p, [1]) == abi.ERR_BADARG
    # a join
    p = abi.make_plan(table=t, preds=pred)
    p.join_dim = 0
    p.join_fact_col = 0
    assert select_code(eng, p, [1]) == abi.ERR_UNSUPPORTED
    # nproj outside 1..8
    p = abi.make_plan(table=t, preds=pred)
    assert select_code(eng, p, []) == abi.ERR_BADARG
    assert select_code(eng, p, [0] * 9) == abi.ERR_BADARG
    # a column ordinal that is neither a column nor ROWID
    assert select_code(eng, p, [1, 10]) == abi.ERR_BADARG
    assert select_code(eng, p, [-2]) == abi.ERR_BADARG
    bad = abi.make_plan(table=t, preds=[dict(col=10, lo=1)])
    assert select_code(eng, bad, [1]) == abi.ERR_BADARG
    # predicate column 0 plus eight others: nine distinct columns
    assert select_code(eng, p, list(range(1, 9))) == abi.ERR_UNSUPPORTED
    # an unknown table
    p.table = 5
    assert select_code(eng, p, [1]) == abi.ERR_BADARG
    # well-formed: eight distinct columns, duplicates and ROWID on top
    for plan, cols in [
            (abi.make_plan(table=t, preds=pred), [1, 2, abi.PROJ_ROWID]),
            (abi.make_plan(table=t, preds=pred), list(range(0, 8))),
            (abi.make_plan(table=t, preds=pred), [1, 1, 0, abi.PROJ_ROWID,
                                                  abi.PROJ_ROWID, 2, 3, 1]),
            (abi.make_plan(table=t), [0]),
            (abi.make_plan(table=t, preds=[dict(col=2, eq=b"aa")]), [2]),
            (abi.make_plan(table=t, preds=[dict(col=0, **{"in": [1, 3]})]),
             [0])]:
        assert select_code(eng, plan, cols, limit=5) == abi.ERR_NOGPU


def test_null_arguments(eng):
    t = define(eng)
    L = se.lib()
    p = abi.make_plan(table=t)
    one = (C.c_int32 * 1)(0)
    assert not L.sn_scan_submit(None, C.byref(p), 1, one, 0)
    assert L.sn_last_error_code() == abi.ERR_BADARG
    assert not L.sn_scan_submit(eng._h, None, 1, one, 0)
    assert L.sn_last_error_code() == abi.ERR_BADARG
    assert not L.sn_scan_submit(eng._h, C.byref(p), 1, None, 0)
    assert L.sn_last_error_code() == abi.ERR_BADARG
    assert L.sn_rows_count(None) == abi.ERR_BADARG
    assert L.sn_rows_fetch(None, 0, 0, 0, None, None, 0) == abi.ERR_BADARG


def test_dict_value_and_batch_id(eng):
    t = define(eng)
    strs = put_one_batch(eng, t, uuid=77, bucket=3)
    assert eng.batch_id(t, 0) == (77, 3)
    got = sorted(eng.dict_value(t, 2, g) for g in range(3))
    assert got == sorted(set(strs))
    L = se.lib()
    # the length alone, a buffer that is too small, an exact fit
    lens = sorted(L.sn_table_dict_value(eng._h, t, 2, g, None, 0)
                  for g in range(3))
    assert lens == [1, 2, 3]
    g3 = [g for g in range(3) if eng.dict_value(t, 2, g) == b"ccc"][0]
    buf = C.create_string_buffer(3)
    assert L.sn_table_dict_value(eng._h, t, 2, g3, buf, 2) == abi.ERR_BADARG
    assert L.sn_table_dict_value(eng._h, t, 2, g3, buf, 3) == 3
    assert buf.raw == b"ccc"
    for table, col, gid in [(9, 2, 0), (-1, 2, 0),      # table
                            (t, 0, 0), (t, 10, 0), (t, -1, 0),   # column
                            (t, 2, 3), (t, 2, -1)]:     # dictionary id
        with pytest.raises(se.EngineError) as ei:
            eng.dict_value(table, col, gid)
        assert ei.value.code == abi.ERR_BADARG, (table, col, gid)
    for table, batch in [(9, 0), (t, 1), (t, -1)]:
        with pytest.raises(se.EngineError) as ei:
            eng.batch_id(table, batch)
        assert ei.value.code == abi.ERR_BADARG, (table, batch)
