"""Ordered row scan (sn_scan_submit_ordered), host side (no GPU): the new
symbols resolve, every submit-time rejection fires with its own status code
before the engine asks for a device, the host twin of the device key image
orders every type as the numpy reference does, and the string rank table
equals sorted() over the byte strings."""
import ctypes as C

import numpy as np
import pytest

from snappydata_amd import abi, engine as se

NEW_SYMBOLS = ["sn_scan_submit_ordered", "sn_order_key_h",
               "sn_order_dict_ranks", "sn_launch_order_sort",
               "sn_launch_order_select", "sn_launch_order_gather"]


@pytest.fixture
def eng():
    e = se.Engine(device=-1)
    yield e
    e.close()


def define(eng, ncols=10):
    """col 0 int32, 1 double, 2 string, the rest int32"""
    schema = [(abi.T_INT32, False), (abi.T_DOUBLE, False),
              (abi.T_STRING, True)] + [(abi.T_INT32, False)] * (ncols - 3)
    return eng.table_define("ord_t", schema)


def code(eng, plan, cols, **kw):
    with pytest.raises(se.EngineError) as ei:
        eng.select(plan, cols, **kw)
    assert se.last_error()
    return ei.value.code


def raw_code(eng, plan, cols, order_col, flags, limit):
    arr = (C.c_int32 * len(cols))(*cols)
    L = se.lib()
    assert not L.sn_scan_submit_ordered(eng._h, C.byref(plan), len(cols), arr,
                                        order_col, flags, limit)
    return L.sn_last_error_code()


def test_new_symbols_resolve():
    lib = se.lib()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name, None) is not None, name
    assert (abi.ORDER_DESC, abi.ORDER_NULLS_FIRST, abi.ORDER_NULLS_LAST) == \
        (1, 2, 4)
    assert abi.ORDER_MAX_LIMIT == 8192


def test_rejections_then_nogpu(eng):
    t = define(eng)
    pred = [dict(col=0, lo=1, hi=2)]
    p = abi.make_plan(table=t, preds=pred)
    # sn_scan_submit's own checks come first, with their codes
    pa = abi.make_plan(table=t, preds=pred, aggs=[("count", [])])
    assert code(eng, pa, [1], limit=5, order_by=1) == abi.ERR_BADARG
    pj = abi.make_plan(table=t, preds=pred)
    pj.join_dim = 0
    pj.join_fact_col = 0
    assert code(eng, pj, [1], limit=5, order_by=1) == abi.ERR_UNSUPPORTED
    assert code(eng, p, [], limit=5, order_by=1) == abi.ERR_BADARG
    assert code(eng, p, [1, 10], limit=5, order_by=1) == abi.ERR_BADARG
    assert code(eng, p, list(range(1, 9)), limit=5, order_by=1) == \
        abi.ERR_UNSUPPORTED
    # order_col: a table column
    assert code(eng, p, [1], limit=5, order_by=abi.PROJ_ROWID) == abi.ERR_BADARG
    assert code(eng, p, [1], limit=5, order_by=10) == abi.ERR_BADARG
    assert code(eng, p, [1], limit=5, order_by=-2) == abi.ERR_BADARG
    # flags: outside the three bits, or both NULLS bits
    assert raw_code(eng, p, [1], 1, 8, 5) == abi.ERR_BADARG
    assert raw_code(eng, p, [1], 1, -1, 5) == abi.ERR_BADARG
    assert raw_code(eng, p, [1], 1, abi.ORDER_NULLS_FIRST |
                    abi.ORDER_NULLS_LAST, 5) == abi.ERR_BADARG
    assert raw_code(eng, p, [1], 1, 7, 5) == abi.ERR_BADARG
    # limit
    assert code(eng, p, [1], limit=0, order_by=1) == abi.ERR_BADARG
    assert code(eng, p, [1], limit=-3, order_by=1) == abi.ERR_BADARG
    assert code(eng, p, [1], limit=abi.ORDER_MAX_LIMIT + 1, order_by=1) == \
        abi.ERR_UNSUPPORTED
    # the key is the ninth distinct column: predicate 0, projections 1..7, key 8
    assert code(eng, p, list(range(1, 8)), limit=5, order_by=8) == \
        abi.ERR_UNSUPPORTED
    # well-formed calls reach the GPU check
    for cols, kw in [
            ([1], dict(order_by=1)),
            ([1], dict(order_by=3)),                  # key not projected
            ([abi.PROJ_ROWID], dict(order_by=2, descending=True)),
            (list(range(1, 8)), dict(order_by=7)),    # eight columns, key among
            (list(range(1, 7)), dict(order_by=9)),    # ... and key the eighth
            ([0], dict(order_by=0, nulls_first=True)),
            ([0], dict(order_by=0, nulls_first=False, descending=True)),
            ([0, 2], dict(order_by=2, limit=abi.ORDER_MAX_LIMIT)),
            ([0], dict(order_by=1, limit=1))]:
        kw.setdefault("limit", 5)
        assert code(eng, p, cols, **kw) == abi.ERR_NOGPU, (cols, kw)
    # order_by=None is sn_scan_submit, limit 0 and all
    assert code(eng, p, [1], limit=0) == abi.ERR_NOGPU
    # null arguments
    L = se.lib()
    one = (C.c_int32 * 1)(0)
    assert not L.sn_scan_submit_ordered(None, C.byref(p), 1, one, 0, 0, 5)
    assert L.sn_last_error_code() == abi.ERR_BADARG
    assert not L.sn_scan_submit_ordered(eng._h, None, 1, one, 0, 0, 5)
    assert L.sn_last_error_code() == abi.ERR_BADARG
    assert not L.sn_scan_submit_ordered(eng._h, C.byref(p), 1, None, 0, 0, 5)
    assert L.sn_last_error_code() == abi.ERR_BADARG


# ---- sn_order_key_h: the device's key image, on the host ----

def image(dtype, bits, desc=0):
    L = se.lib()
    return np.array([L.sn_order_key_h(dtype, int(b), desc) for b in bits],
                    dtype=np.uint64)


def as_bits(a):
    """what sn_order_key_h takes: integers sign-extended to 64 bits, float
    patterns zero-extended"""
    if a.dtype == np.float64:
        return a.view(np.uint64)
    if a.dtype == np.float32:
        return a.view(np.uint32).astype(np.uint64)
    return a.astype(np.int64).view(np.uint64)


def bits64(x):
    return np.array(x, dtype=np.uint64).view(np.float64)


def bits32(x):
    return np.array(x, dtype=np.uint32).view(np.float32)


def float_reference_order(v):
    """stable order on (isnan, value with -0.0 folded)"""
    nan = np.isnan(v)
    folded = np.where(nan | (v == 0), 0, v).astype(v.dtype)
    return np.lexsort((np.arange(len(v)), folded, nan))


INT_VECTORS = {
    abi.T_INT64: np.array([-2 ** 63, -2 ** 63 + 1, 2 ** 63 - 1, 2 ** 63 - 2,
                           0, -1, 1, 2, 3, 2 ** 53, 2 ** 53 + 1, -2 ** 53 - 1,
                           -2 ** 53, 2 ** 62, -2 ** 62, 2 ** 62 + 1, 0, -1],
                          dtype=np.int64),
    abi.T_INT32: np.array([-2 ** 31, 2 ** 31 - 1, 0, -1, 1, 2, 3, 2 ** 31 - 2,
                           -2 ** 31 + 1, 65536, 65537, -65536, 0],
                          dtype=np.int32),
    abi.T_INT16: np.array([-32768, 32767, 0, -1, 1, 2, 3, 2047, 2048, 2049,
                           -2048, -2049, 0], dtype=np.int16),
    abi.T_INT8: np.array([-128, 127, 0, -1, 1, 2, 3, 64, -64, 0],
                         dtype=np.int8),
    abi.T_BOOL: np.array([1, 0, 0, 1, 1], dtype=np.uint8),
}
F64 = np.concatenate([
    bits64([0x7FF8000000000001, 0xFFF4000000ABCDEF]),       # two NaN payloads
    np.array([-0.0, 0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-310,
              2.2250738585072014e-308, 1.0, np.nextafter(1.0, 2.0), -1.0,
              np.nextafter(-1.0, -2.0), 1.7976931348623157e308,
              -1.7976931348623157e308, 0.0, -0.0])])
F32 = np.concatenate([
    bits32([0x7FC00001, 0xFFA00123]),
    np.array([-0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 1.0,
              np.nextafter(np.float32(1.0), np.float32(2.0)), -1.0,
              3.4028235e38, -3.4028235e38, 0.0, -0.0], dtype=np.float32)])


@pytest.mark.parametrize("dtype", sorted(INT_VECTORS))
def test_key_image_orders_integers(dtype):
    v = INT_VECTORS[dtype]
    img = image(dtype, as_bits(v))
    ref = np.lexsort((np.arange(len(v)), v))
    got = np.lexsort((np.arange(len(v)), img))
    assert (got == ref).all(), dtype
    # equal values have equal images, different values different ones
    assert ((img[:, None] == img[None, :]) == (v[:, None] == v[None, :])).all()
    if dtype == abi.T_INT64:
        assert img[0] == 0 and img[2] == np.uint64(2 ** 64 - 1)   # full range
        assert img[7] + np.uint64(1) == img[8]       # differ in bit 0 only


@pytest.mark.parametrize("dtype,v", [(abi.T_DOUBLE, F64), (abi.T_FLOAT, F32)])
def test_key_image_orders_floats(dtype, v):
    img = image(dtype, as_bits(v))
    ref = float_reference_order(v)
    got = np.lexsort((np.arange(len(v)), img))
    assert (got == ref).all()
    assert img[0] == img[1]                          # every NaN is one key
    assert img[2] == img[3]                          # -0.0 == 0.0
    assert img[0] > img[4] > img[2] > img[5]         # NaN > +inf > 0 > -inf
    fin = ~np.isnan(v)
    a, b = v[fin], img[fin]
    assert ((b[:, None] < b[None, :]) == (a[:, None] < a[None, :])).all()
    width = 64 if dtype == abi.T_DOUBLE else 32
    assert int(img.max()) < 2 ** width


def test_key_image_desc_is_the_complement():
    for dtype, v, width in [(abi.T_DOUBLE, F64, 64), (abi.T_FLOAT, F32, 32),
                            (abi.T_INT64, INT_VECTORS[abi.T_INT64], 64),
                            (abi.T_INT32, INT_VECTORS[abi.T_INT32], 32),
                            (abi.T_INT16, INT_VECTORS[abi.T_INT16], 16),
                            (abi.T_INT8, INT_VECTORS[abi.T_INT8], 8),
                            (abi.T_BOOL, INT_VECTORS[abi.T_BOOL], 1)]:
        asc = image(dtype, as_bits(v), 0)
        desc = image(dtype, as_bits(v), 1)
        mask = np.uint64(2 ** width - 1)
        assert (desc == (asc ^ mask)).all(), dtype
        assert int(asc.max()) <= int(mask), dtype
    # a string's image is its rank, complemented within 32 bits for DESC
    assert list(image(abi.T_STRING, np.array([0, 5], np.uint64))) == [0, 5]
    assert list(image(abi.T_STRING, np.array([0, 5], np.uint64), 1)) == \
        [2 ** 32 - 1, 2 ** 32 - 6]


# ---- sn_order_dict_ranks ----

def ranks_of(values):
    offs = np.zeros(len(values) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(v) for v in values])
    blob = np.frombuffer(b"".join(values) + b"\0", dtype=np.uint8).copy()
    out = np.full(len(values), -1, dtype=np.int32)
    rc = se.lib().sn_order_dict_ranks(len(values), blob.ctypes.data,
                                      offs.ctypes.data, out.ctypes.data)
    assert rc == 0
    return out


def test_dict_ranks_equal_sorted_bytes():
    values = [b"TRUCK", b"AIRX", b"", b"AIR", b"\xc3\xa9t\xc3\xa9", b"zebra",
              b"\x80", b"A", b"AIR ", b"\xff\xff", b"a", b"MAIL", b"\x7f"]
    assert any(v[:1] >= b"\x80" for v in values if v)
    ranks = ranks_of(values)
    order = sorted(values)                      # bytes compare unsigned
    assert [order[r] for r in ranks] == values
    assert sorted(ranks) == list(range(len(values)))     # a bijection
    at = {v: int(r) for v, r in zip(values, ranks)}
    assert at[b""] == 0
    assert at[b"AIR"] < at[b"AIR "] < at[b"AIRX"]        # a prefix sorts first
    assert at[b"zebra"] < at[b"\x80"] < at[b"\xc3\xa9t\xc3\xa9"] < \
        at[b"\xff\xff"]                                  # unsigned bytes
    rng = np.random.default_rng(3)
    many = list({bytes(rng.integers(0, 256, rng.integers(0, 6)).astype(np.uint8))
                 for _ in range(500)})
    r = ranks_of(many)
    order = sorted(many)
    assert [order[i] for i in r] == many
    assert len(ranks_of([])) == 0
