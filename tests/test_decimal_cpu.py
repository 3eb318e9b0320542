"""Exact DECIMAL aggregation, host side (no GPU): the formatter and the
HALF_UP average against Python's decimal module, the column declaration
rules, and the submit-time rejections that fire before any device work.

The reference everywhere is Python int / decimal.Decimal arithmetic."""
import decimal
from decimal import Decimal

import pytest

from snappydata_amd import abi, engine as se

SN_ERR_BADARG = -2
SN_ERR_UNSUPPORTED = -5

decimal.getcontext().prec = 120

SPREAD = [0, 1, -1, 10 ** 38 - 1, -(10 ** 38 - 1),
          2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, -(2 ** 64) - 1,
          2 ** 127 - 1, -(2 ** 127 - 1), 2 ** 127 - 2,
          5, -5, 12345, -12345, 100, -100, 999999, 10 ** 6, 10 ** 18]


@pytest.mark.parametrize("scale", [0, 2, 6])
def test_to_string_round_trips(scale):
    for v in SPREAD:
        s = se.dec_to_string(v, scale)
        exp = Decimal(v).scaleb(-scale)
        assert Decimal(s) == exp, (v, scale, s)
        # canonical plain form: exactly `scale` fraction digits, no exponent
        assert s == format(exp, "f"), (v, scale, s)
        if scale:
            assert len(s.split(".")[1]) == scale


def test_to_string_examples_and_null():
    assert se.dec_to_string(-1234500, 4) == "-123.4500"
    assert se.dec_to_string(5, 6) == "0.000005"
    assert se.dec_to_string(-5, 2) == "-0.05"
    assert se.dec_to_string(None, 2) == "NULL"


def test_to_string_small_buffer_is_an_error():
    import ctypes as C
    v = abi.dec_val(123456, 2)
    buf = C.create_string_buffer(4)
    assert se.lib().sn_dec_to_string(C.byref(v), buf, 4) == SN_ERR_BADARG


AVG_CASES = [
    (10, 3), (-10, 3), (1, 3), (2, 3), (-2, 3),
    (1, 20000), (-1, 20000),          # exact half at the 4th extra digit
    (3, 20000), (-3, 20000), (1, 2), (-1, 2), (5, 8), (-5, 8),
    (10 ** 38 - 1, 1), (-(10 ** 38 - 1), 7), (2 ** 64 + 12345, 10503),
    (37734107, 1478493), (0, 5), (189203 * 100, 7482),
]


@pytest.mark.parametrize("scale", [0, 2, 6])
def test_avg_matches_decimal_half_up(scale):
    for total, count in AVG_CASES:
        got, gscale = se.dec_avg(total, count, scale)
        assert gscale == scale + 4
        q = Decimal(1).scaleb(-(scale + 4))
        exp = (Decimal(total).scaleb(-scale) / Decimal(count)).quantize(
            q, rounding=decimal.ROUND_HALF_UP)
        exp_int = int(exp.scaleb(scale + 4))
        if abs(exp_int) >= 10 ** 38:
            assert got is None, (total, count)
        else:
            assert got == exp_int, (total, count, scale, got, exp_int)


def test_avg_null_inputs():
    assert se.dec_avg(None, 3, 2) == (None, 6)
    assert se.dec_avg(100, 0, 2) == (None, 6)


@pytest.fixture
def eng():
    e = se.Engine(device=-1)
    yield e
    e.close()


def define(eng):
    t = eng.table_define("dec_t", [(abi.T_INT64, False), (abi.T_INT64, True),
                                   (abi.T_DOUBLE, False), (abi.T_INT32, False)])
    return t


def test_set_decimal_rules(eng):
    t = define(eng)
    eng.table_set_decimal(t, 0, 15, 2)
    eng.table_set_decimal(t, 1, 18, 18)
    eng.table_set_decimal(t, 1, 1, 0)
    for col, prec, scale in [(2, 15, 2),      # DOUBLE column
                             (3, 9, 0),       # INT32 column
                             (0, 19, 2),      # beyond the long-decimal range
                             (0, 0, 0),
                             (0, 5, 6),       # scale > precision
                             (0, 5, -1),
                             (9, 5, 2)]:      # no such column
        with pytest.raises(se.EngineError) as ei:
            eng.table_set_decimal(t, col, prec, scale)
        assert ei.value.code == SN_ERR_BADARG, (col, prec, scale)
        assert se.last_error()


def submit_code(eng, plan, aggs):
    with pytest.raises(se.EngineError) as ei:
        eng.query_dec(plan, aggs)
    assert se.last_error()
    return ei.value.code


def test_submit_dec_rejections(eng):
    t = define(eng)
    eng.table_set_decimal(t, 0, 15, 2)
    eng.table_set_decimal(t, 1, 18, 0)
    # a column that was never declared decimal (INT32) and a DOUBLE one
    for col in (3, 2):
        p, a = abi.make_dec_plan(table=t, aggs=[("sum", [(col, 0, 1)])])
        assert submit_code(eng, p, a) == SN_ERR_BADARG
    # a join
    p, a = abi.make_dec_plan(table=t, aggs=[("sum", [(0, 0, 1)])])
    p.join_dim = 0
    p.join_fact_col = 3
    assert submit_code(eng, p, a) == SN_ERR_UNSUPPORTED
    # plan->naggs must be 0
    p, a = abi.make_dec_plan(table=t, aggs=[("sum", [(0, 0, 1)])])
    p.naggs = 1
    assert submit_code(eng, p, a) == SN_ERR_BADARG
    # |add| + |mul| * 10^18 exceeds int64
    p, a = abi.make_dec_plan(table=t, aggs=[("sum", [(1, 0, 10)])])
    assert submit_code(eng, p, a) == SN_ERR_UNSUPPORTED
    p, a = abi.make_dec_plan(table=t, aggs=[("sum", [(1, 2 ** 63 - 1, 1)])])
    assert submit_code(eng, p, a) == SN_ERR_UNSUPPORTED
    # MIN/MAX take exactly one factor
    p, a = abi.make_dec_plan(table=t,
                             aggs=[("min", [(0, 0, 1), (0, 0, 1)])])
    assert submit_code(eng, p, a) == SN_ERR_BADARG
    # a well-formed decimal plan passes validation and then fails loudly for
    # lack of a device — never a CPU fallback
    p, a = abi.make_dec_plan(table=t, aggs=[("sum", [(0, 100, -1)]),
                                            ("count", [])])
    assert submit_code(eng, p, a) == abi.ERR_NOGPU
