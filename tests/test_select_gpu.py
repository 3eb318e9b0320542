"""Row-returning filter scan on the GPU: Engine.select against numpy over the
arrays the test generated (never the engine, never the oracle; the oracle
module only encodes the input blobs).  Every comparison is on raw bytes,
tolerance zero, and every case asserts that its reference mask keeps some but
not all rows unless it is named "none" or "all".

The base table's batches are 17445 rows (a full 16 K tile, one full chunk, a
37-row tail), the same again, 63 rows (less than a wave), 1 row and 16384 rows
(exactly one tile)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se
from tests import devmem as dm

pytestmark = pytest.mark.gpu

SIZES = (17445, 17445, 63, 1, 16384)
KEY, F, L, N, S, STR = range(6)
DTYPES = [po.T_INT32, po.T_DOUBLE, po.T_INT64, po.T_DOUBLE, po.T_INT16,
          po.T_STRING]
WORDS = [b"AIR", b"MAIL", b"RAIL", b"SHIP", b"TRUCK", b"REG AIR", b"FOB"]
NAN_A, NAN_B = 0x7FF8000000000001, 0xFFF4000000ABCDEF
BOUNDARY = (0, 63, 64, 255, 256, 1023, 1024, 16383, 16384)


def bits(x):
    return np.array(x, dtype=np.uint64).view(np.float64)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        bool((a.view(np.uint8) == b.view(np.uint8)).all())


def make_base():
    """per batch: [key, f, l, n, s, str] (str as an index into WORDS)"""
    rng = np.random.default_rng(20240611)
    out, start = [], 0
    special = np.concatenate([bits([NAN_A, NAN_B]),
                              np.array([-0.0, 0.0, np.inf, -np.inf, 5e-324])])
    nvals = np.concatenate([np.arange(11) / 128.0, np.array([-0.0]),
                            bits([NAN_A])])
    for n in SIZES:
        key = np.arange(start, start + n, dtype=np.int32)
        f = rng.standard_normal(n) * 1e6
        f[rng.integers(0, n, max(1, n // 9))] = \
            special[rng.integers(0, len(special), max(1, n // 9))]
        f[:min(n, len(special))] = special[:min(n, len(special))]
        ll = rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)
        ll[::3] += np.int64(2 ** 62)
        ll[1::3] -= np.int64(2 ** 62)
        nn = nvals[rng.integers(0, len(nvals), n)]
        s = rng.integers(0, 100, n).astype(np.int16)
        w = rng.integers(0, len(WORDS), n)
        out.append([key, f, ll, nn, s, w])
        start += n
    return out


def base_blobs(cols):
    key, f, ll, nn, s, w = cols
    return [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, key),
            po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f),
            po.encode(po.T_INT64, po.ENC_UNCOMPRESSED, ll),
            po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, nn),
            po.encode(po.T_INT16, po.ENC_UNCOMPRESSED, s),
            po.encode(po.T_STRING, po.ENC_DICT, [WORDS[i] for i in w])]


def base_stats(cols):
    key, f, ll, nn, s, w = cols
    n = len(key)
    lo = [int(key.min()), -np.inf, int(ll.min()), -np.inf, int(s.min()), 0]
    hi = [int(key.max()), np.inf, int(ll.max()), np.inf, int(s.max()), 0]
    return po.encode_stats(DTYPES, n, lo, hi, null_counts=[0] * 6,
                           has_bounds=[1, 0, 1, 0, 1, 0])


class Base:
    pass


@pytest.fixture(scope="module")
def base():
    b = Base()
    b.batches = make_base()
    b.eng = se.Engine(device=0)
    b.t = b.eng.table_define("sel_base", [
        (abi.T_INT32, False), (abi.T_DOUBLE, False), (abi.T_INT64, False),
        (abi.T_DOUBLE, False), (abi.T_INT16, False), (abi.T_STRING, False)])
    for bi, cols in enumerate(b.batches):
        b.eng.batch_put(b.t, 1000 + bi, 3 * bi, len(cols[0]), base_blobs(cols),
                        stats=base_stats(cols))
    b.col = [np.concatenate([c[i] for c in b.batches]) for i in range(6)]
    b.batch = np.concatenate([np.full(len(c[0]), bi, dtype=np.int64)
                              for bi, c in enumerate(b.batches)])
    b.ordinal = np.concatenate([np.arange(len(c[0]), dtype=np.int64)
                                for c in b.batches])
    b.nrows = len(b.batch)
    b.starts = np.cumsum((0,) + SIZES)[:-1]
    yield b
    b.eng.close()


def check_rows(b, rs, mask, cols, name=""):
    """Every projected column of RowSet rs equals the reference rows `mask`
    keeps, in scan order, byte for byte."""
    kept = int(mask.sum())
    if name not in ("none", "all"):
        assert 0 < kept < b.nrows, (name, kept)
    assert rs.count() == kept, (name, rs.count(), kept)
    for p, c in enumerate(cols):
        vals, valid = rs.column(p)
        assert valid.dtype == np.bool_ and valid.all(), (name, p)
        if c == abi.PROJ_ROWID:
            gb, go = rs.rowids(p)
            assert same_bytes(gb, b.batch[mask]), (name, "rowid batch")
            assert same_bytes(go, b.ordinal[mask]), (name, "rowid ordinal")
        elif c == STR:
            exp = [WORDS[i] for i in b.col[STR][mask]]
            assert rs.strings(p) == exp, (name, "strings")
        else:
            assert same_bytes(vals, b.col[c][mask]), (name, c)


def select(b, preds, cols, limit=0):
    return b.eng.select(abi.make_plan(table=b.t, preds=preds), cols, limit)


ALL_COLS = [KEY, F, L, N, S, STR, abi.PROJ_ROWID]


def test_narrowing_engaged(base):
    assert base.eng.narrowed_batches(base.t, N) == len(SIZES) > 0


def test_boundary_rows_in_list(base):
    b = base
    keys = []
    for start, n in zip(b.starts, SIZES):
        keys += [int(start + o) for o in BOUNDARY if o < n] + [int(start + n - 1)]
    keys = sorted(set(keys))
    mask = np.isin(b.col[KEY], keys)
    assert int(mask.sum()) == len(keys)
    rs = select(b, [dict(col=KEY, **{"in": keys})], ALL_COLS)
    check_rows(b, rs, mask, ALL_COLS, "boundary-in")
    assert same_bytes(rs.column(0)[0], np.array(keys, dtype=np.int32))


@pytest.mark.parametrize("lo,hi", [(16380, 16390), (17444, 17445 + 64),
                                   (2 * 17445 + 62, 2 * 17445 + 64 + 1023)])
def test_boundary_rows_range(base, lo, hi):
    b = base
    mask = (b.col[KEY] >= lo) & (b.col[KEY] <= hi)
    rs = select(b, [dict(col=KEY, lo=lo, hi=hi)], ALL_COLS)
    check_rows(b, rs, mask, ALL_COLS, "boundary-range")


@pytest.mark.parametrize("name", ["2pct", "50pct", "all", "none"])
def test_selectivities(base, name):
    b = base
    s = b.col[S]
    preds, mask = {
        "2pct": ([dict(col=S, hi=1)], s <= 1),
        "50pct": ([dict(col=S, hi=50, hi_strict=True)], s < 50),
        "all": ([], np.ones(b.nrows, dtype=bool)),
        # (a column without stats bounds, so no batch is skipped)
        "none": ([dict(col=N, is_double=True, lo=0.5, hi=0.6)],
                 (b.col[N] >= 0.5) & (b.col[N] <= 0.6)),
    }[name]
    rs = select(b, preds, ALL_COLS)
    check_rows(b, rs, mask, ALL_COLS, name)
    res = rs.result()
    assert (res.nrows, res.naggs) == (0, 0)
    assert res.rows_passed == int(mask.sum())
    assert res.rows_scanned == b.nrows and res.batches_seen == len(SIZES)
    if name == "none":
        assert not mask.any()
        vals, valid = rs.column(0, 0, 0)          # n == 0 is fine
        assert len(vals) == 0 and len(valid) == 0
        assert rs.kernel_ms() > 0                 # mark + offsets still ran
    frac = mask.mean()
    if name == "2pct":
        assert 0.01 < frac < 0.03
    if name == "50pct":
        assert 0.45 < frac < 0.55


def test_narrowed_predicate_and_projection(base):
    b = base
    nn = b.col[N]
    mask = (nn >= 5 / 128) & (nn <= 7 / 128)
    rs = select(b, [dict(col=N, is_double=True, lo=5 / 128, hi=7 / 128)],
                [N, F, abi.PROJ_ROWID])
    check_rows(b, rs, mask, [N, F, abi.PROJ_ROWID], "narrow-pred")
    # projection alone: -0.0 and the NaN payload come back from the codes
    m2 = b.col[S] < 30
    rs = select(b, [dict(col=S, hi=30, hi_strict=True)], [N])
    check_rows(b, rs, m2, [N], "narrow-proj")
    got = rs.column(0)[0].view(np.uint64)
    assert (got == np.uint64(NAN_A)).any() and \
        (got == np.uint64(0x8000000000000000)).any()


def test_strings(base):
    b = base
    w = b.col[STR]
    rs = select(b, [dict(col=STR, eq=b"MAIL")], [STR, KEY])
    check_rows(b, rs, w == WORDS.index(b"MAIL"), [STR, KEY], "str-eq")
    rs = select(b, [dict(col=STR, **{"in": [b"AIR", b"RAIL", b"absent"]})],
                [KEY, STR])
    check_rows(b, rs, np.isin(w, [WORDS.index(b"AIR"), WORDS.index(b"RAIL")]),
               [KEY, STR], "str-in")
    rs = select(b, [dict(col=STR, eq=b"absent")], [STR])
    check_rows(b, rs, np.zeros(b.nrows, dtype=bool), [STR], "none")


def test_limit_is_a_prefix(base):
    b = base
    mask = b.col[S] < 50
    total = int(mask.sum())
    second_tile = int(mask[:16384].sum())        # output offset of tile 1
    assert 0 < second_tile < total
    preds = [dict(col=S, hi=50, hi_strict=True)]
    cols = [KEY, F, STR, abi.PROJ_ROWID]
    full = select(b, preds, cols)
    check_rows(b, full, mask, cols, "limit-full")
    ref = [full.column(p)[0] for p in range(len(cols))]
    for limit in (1, second_tile, second_tile + 1, total, total + 5):
        rs = select(b, preds, cols, limit=limit)
        k = min(limit, total)
        assert rs.count() == k, limit
        assert rs.rows_passed() == total, limit   # the count before the limit
        for p in range(len(cols)):
            vals, valid = rs.column(p)
            assert valid.all()
            assert same_bytes(vals, ref[p][:k]), (limit, p)


def test_fetch_ranges_and_device_destination(base):
    b = base
    mask = b.col[S] <= 1
    rs = select(b, [dict(col=S, hi=1)], [L])
    exp = b.col[L][mask]
    n = rs.count()
    assert n == len(exp) > 10
    vals, valid = rs.column(0, 3, 5)
    assert same_bytes(vals, exp[3:8]) and valid.all()
    vals, _ = rs.column(0, n, 0)                  # empty range at the end
    assert len(vals) == 0
    L_ = se.lib()
    buf = np.zeros(8, dtype=np.int64)
    for off, cnt in [(-1, 1), (0, n + 1), (n, 1), (1, -1), (n + 1, 0)]:
        assert L_.sn_rows_fetch(rs._h, 0, off, cnt, buf.ctypes.data, None, 0) \
            == abi.ERR_BADARG, (off, cnt)
    assert L_.sn_rows_fetch(rs._h, 1, 0, 1, buf.ctypes.data, None, 0) \
        == abi.ERR_BADARG
    # valid may be NULL; a device destination
    assert L_.sn_rows_fetch(rs._h, 0, 0, 8, buf.ctypes.data, None, 0) == 0
    assert same_bytes(buf, exp[:8])
    gv, gn = dm.guarded(8 * n), dm.guarded(n)
    try:
        assert L_.sn_rows_fetch(rs._h, 0, 0, n, C.c_void_p(gv.ptr),
                                C.c_void_p(gn.ptr), 1) == 0
        dm.sync()
        assert gv.read() == exp.tobytes()
        assert gn.read() == b"\x01" * n
        gv.check_bands()
        gn.check_bands()
    finally:
        gv.free()
        gn.free()


def test_stats_skipping_keeps_table_batch_indices(base):
    b = base
    lo = int(b.starts[1])                          # batch 0 lies below
    mask = b.col[KEY] >= lo
    rs = select(b, [dict(col=KEY, lo=lo), dict(col=S, hi=50, hi_strict=True)],
                [abi.PROJ_ROWID, KEY])
    m = mask & (b.col[S] < 50)
    check_rows(b, rs, m, [abi.PROJ_ROWID, KEY], "skip")
    res = rs.result()
    assert res.batches_skipped == 1 and res.batches_seen == len(SIZES)
    assert res.rows_scanned == b.nrows - SIZES[0]
    gb, _ = rs.rowids()
    assert set(np.unique(gb)) == {1, 2, 3, 4}
    for bi in range(len(SIZES)):
        assert b.eng.batch_id(b.t, bi) == (1000 + bi, 3 * bi)
    # two leading and one trailing batch skipped: scan-set slots 0 and 1 are
    # the table's batches 2 and 3
    lo, hi = int(b.starts[2]) + 1, int(b.starts[3])
    rs = select(b, [dict(col=KEY, lo=lo, hi=hi)], [abi.PROJ_ROWID, KEY])
    check_rows(b, rs, (b.col[KEY] >= lo) & (b.col[KEY] <= hi),
               [abi.PROJ_ROWID, KEY], "skip-both-ends")
    assert rs.result().batches_skipped == 3
    gb, go = rs.rowids()
    assert list(gb) == [2] * 62 + [3] and list(go) == list(range(1, 63)) + [0]


def test_handle_contract(base):
    b = base
    rs = select(b, [], [KEY], limit=1)
    assert rs.count() == 1 and rs.rows_passed() == b.nrows
    assert same_bytes(rs.column(0)[0], b.col[KEY][:1])
    assert rs.used_jit() is False and rs.late_cols() == []
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
    # the aggregate route on the same engine is untouched: Q6's shape
    key, nn, s = b.col[KEY], b.col[N], b.col[S]
    lo, hi = 1000, 45000
    m = (key >= lo) & (key < hi) & (nn >= 5 / 128) & (nn <= 7 / 128) & (s < 24)
    assert 0 < m.sum() < b.nrows
    q = b.eng.query(abi.make_plan(
        table=b.t,
        preds=[dict(col=KEY, lo=lo, hi=hi, hi_strict=True),
               dict(col=N, is_double=True, lo=5 / 128, hi=7 / 128),
               dict(col=S, hi=24, hi_strict=True)],
        aggs=[("sum", [(N, 0.0, 1.0), (S, 0.0, 1.0)]), ("count", [])]))
    (_, (gsum, gcount)), = q.rows()
    exp = float((nn[m] * s[m].astype(np.float64)).sum())
    assert gcount == float(m.sum())
    assert abs(gsum - exp) <= 1e-6 * max(1.0, abs(exp))
    # ... and the row calls refuse an aggregate handle
    assert L_.sn_rows_count(q._h) == abi.ERR_BADARG
    assert L_.sn_rows_fetch(q._h, 0, 0, 0, None, None, 0) == abi.ERR_BADARG
    # the select that follows an aggregate is not served its descriptor set
    rs = select(b, [dict(col=KEY, lo=lo, hi=hi, hi_strict=True),
                    dict(col=N, is_double=True, lo=5 / 128, hi=7 / 128),
                    dict(col=S, hi=24, hi_strict=True)], [N, S])
    check_rows(b, rs, m, [N, S], "after-agg")


# ---- the general path: nulls, deletes, deltas, RLE, bitset, int8, float ----

GKEY, GPN, GQN, GU, GR, GB, GI8, GFL = range(8)
GSIZES = (2500, 1100, 1030)


def make_general():
    rng = np.random.default_rng(77)
    out, start = [], 0
    for bi, n in enumerate(GSIZES):
        nulls = bi < 2                     # the last batch is null-free: clean
        key = np.arange(start, start + n, dtype=np.int32)
        pn = rng.standard_normal(n)
        pn[:3] = bits([NAN_A, NAN_B, 0x8000000000000000])
        pn_valid = (rng.random(n) > 0.2).astype(np.uint8) if nulls else None
        qn = rng.integers(0, 100, n).astype(np.int32)
        qn_valid = (rng.random(n) > 0.1).astype(np.uint8) if nulls else None
        u = rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64)
        r = np.repeat(rng.integers(-5, 5, n // 7 + 1), 7)[:n].astype(np.int32)
        bo = (rng.random(n) > 0.5).astype(np.uint8)
        i8 = rng.integers(-128, 128, n).astype(np.int8)
        fl = (rng.standard_normal(n) * 100).astype(np.float32)
        fl[:4] = np.array([np.inf, -0.0, np.nan, -np.inf], dtype=np.float32)
        out.append(dict(key=key, pn=pn, pn_valid=pn_valid, qn=qn,
                        qn_valid=qn_valid, u=u, r=r, bo=bo, i8=i8, fl=fl))
        start += n
    return out


def general_blobs(g, bool_bitset):
    U = po.ENC_UNCOMPRESSED
    return [po.encode(po.T_INT32, U, g["key"]),
            po.encode(po.T_DOUBLE, U, g["pn"], g["pn_valid"]),
            po.encode(po.T_INT32, U, g["qn"], g["qn_valid"]),
            po.encode(po.T_INT64, U, g["u"]),
            po.encode(po.T_INT32, po.ENC_RLE, g["r"]),
            po.encode(po.T_BOOL, po.ENC_BOOLBITSET if bool_bitset else U,
                      g["bo"]),
            po.encode(po.T_INT8, U, g["i8"].view(np.uint8)),
            po.encode(po.T_FLOAT, U, g["fl"])]


@pytest.fixture(scope="module")
def general():
    g = Base()
    g.batches = make_general()
    g.eng = se.Engine(device=0)
    g.t = g.eng.table_define("sel_general", [
        (abi.T_INT32, False), (abi.T_DOUBLE, True), (abi.T_INT32, True),
        (abi.T_INT64, True), (abi.T_INT32, False), (abi.T_BOOL, False),
        (abi.T_INT8, False), (abi.T_FLOAT, False)])
    n0 = GSIZES[0]
    g.deleted = np.array([0, 63, 64, 1500], dtype=np.int32)
    # two deltas deep on the i64 column: delta1 overrides delta2 at row 5,
    # writes NULL at row 129 and a value beyond 2^53 at the last row
    d2_pos = np.array([5, 64, 700], dtype=np.int32)
    d2_val = np.array([111, 222, 2 ** 61 + 3], dtype=np.int64)
    d1_pos = np.array([5, 129, n0 - 1], dtype=np.int32)
    d1_val = np.array([-(2 ** 60) - 1, 0, 2 ** 53 + 1], dtype=np.int64)
    d1_ok = np.array([1, 0, 1], dtype=np.uint8)
    deltas = [(None, None)] * 8
    deltas[GU] = (po.encode_delta(po.T_INT64, po.ENC_UNCOMPRESSED, d1_pos, n0,
                                  d1_val, d1_ok),
                  po.encode_delta(po.T_INT64, po.ENC_UNCOMPRESSED, d2_pos, n0,
                                  d2_val))
    g.eng.batch_put(g.t, 50, 0, -n0, general_blobs(g.batches[0], True),
                    delete_mask=po.encode_delete(g.deleted, n0), deltas=deltas)
    # bool as a bitset in batch 0, as bytes in the others; batch 2 is clean
    g.eng.batch_put(g.t, 51, 1, GSIZES[1], general_blobs(g.batches[1], False))
    g.eng.batch_put(g.t, 52, 2, GSIZES[2], general_blobs(g.batches[2], False))
    # the reference: values with NULL rows zeroed, validity, liveness
    u0 = g.batches[0]["u"].copy()
    u0_ok = np.ones(n0, dtype=bool)
    u0[d2_pos] = d2_val
    u0[d1_pos] = d1_val
    u0_ok[129] = False
    u0[129] = 0

    def cat(name, dtype=None):
        return np.concatenate([b[name] for b in g.batches])

    def cat_valid(name):
        return np.concatenate([
            np.ones(len(b["key"]), dtype=bool) if b[name] is None
            else b[name].astype(bool) for b in g.batches])

    g.val = {GKEY: cat("key"), GPN: cat("pn"), GQN: cat("qn"),
             GU: np.concatenate([u0, g.batches[1]["u"], g.batches[2]["u"]]),
             GR: cat("r"), GB: cat("bo"), GI8: cat("i8"), GFL: cat("fl")}
    g.ok = {c: np.ones(sum(GSIZES), dtype=bool) for c in range(8)}
    g.ok[GPN] = cat_valid("pn_valid")
    g.ok[GQN] = cat_valid("qn_valid")
    g.ok[GU] = np.concatenate([u0_ok, np.ones(GSIZES[1] + GSIZES[2], bool)])
    for c in (GPN, GQN, GU):
        g.val[c] = np.where(g.ok[c], g.val[c], 0).astype(g.val[c].dtype)
    g.live = np.ones(sum(GSIZES), dtype=bool)
    g.live[g.deleted] = False
    g.batch = np.concatenate([np.full(n, bi, dtype=np.int64)
                              for bi, n in enumerate(GSIZES)])
    g.ordinal = np.concatenate([np.arange(n, dtype=np.int64) for n in GSIZES])
    yield g
    g.eng.close()


def check_general(g, rs, mask, cols):
    assert 0 < mask.sum() < len(mask)
    assert rs.count() == int(mask.sum())
    for p, c in enumerate(cols):
        vals, valid = rs.column(p)
        if c == abi.PROJ_ROWID:
            gb, go = rs.rowids(p)
            assert same_bytes(gb, g.batch[mask])
            assert same_bytes(go, g.ordinal[mask])
            assert valid.all()
            continue
        assert same_bytes(valid, g.ok[c][mask]), c
        exp = g.val[c][mask]
        if c == GFL:
            # a FLOAT NaN compares as NaN only; its payload is not pinned
            nan = np.isnan(exp)
            assert same_bytes(np.isnan(vals), nan)
            assert same_bytes(vals[~nan], exp[~nan])
        else:
            assert same_bytes(vals, exp), c


def test_general_path_nullable_predicate(general):
    g = general
    cols = [GKEY, GPN, GU, GR, GB, GI8, GFL, abi.PROJ_ROWID]
    mask = g.live & g.ok[GQN] & (g.val[GQN] >= 10) & (g.val[GQN] <= 60)
    assert (~g.ok[GQN] & g.live).any()          # NULLs that the predicate drops
    rs = g.eng.select(abi.make_plan(table=g.t,
                                    preds=[dict(col=GQN, lo=10, hi=60)]), cols)
    check_general(g, rs, mask, cols)
    # the patched rows are among the kept ones
    kept = set(zip(g.batch[mask], g.ordinal[mask]))
    assert {(0, 5), (0, 700), (0, 129), (0, GSIZES[0] - 1)} & kept


def test_general_path_everything_alive(general):
    g = general
    cols = [GQN, GU, GPN, GB, GFL, GI8, GR, abi.PROJ_ROWID]
    rs = g.eng.select(abi.make_plan(table=g.t), cols)
    check_general(g, rs, g.live, cols)          # the delete mask alone
    vals, valid = rs.column(1)
    at = {(int(bb), int(oo)): i for i, (bb, oo) in
          enumerate(zip(g.batch[g.live], g.ordinal[g.live]))}
    assert not valid[at[(0, 129)]] and vals[at[(0, 129)]] == 0
    assert vals[at[(0, 5)]] == -(2 ** 60) - 1    # delta1 over delta2
    assert vals[at[(0, 700)]] == 2 ** 61 + 3
    assert vals[at[(0, GSIZES[0] - 1)]] == 2 ** 53 + 1
    assert (0, 64) not in at                     # deleted, though patched


def test_general_path_predicate_on_rle_and_bool(general):
    g = general
    cols = [GKEY, GR, GB]
    mask = g.live & (g.val[GR] >= 0) & (g.val[GB] == 1)
    rs = g.eng.select(abi.make_plan(
        table=g.t, preds=[dict(col=GR, lo=0), dict(col=GB, lo=1, hi=1)]), cols)
    check_general(g, rs, mask, cols)


def test_round_trip_through_the_mutation_seam():
    eng = se.Engine(device=0)
    try:
        t = eng.table_define("sel_mut", [(abi.T_INT32, False),
                                         (abi.T_INT32, False)])
        sizes, start, keys, vals = (1000, 70), 0, [], []
        rng = np.random.default_rng(5)
        for bi, n in enumerate(sizes):
            k = np.arange(start, start + n, dtype=np.int32)
            v = rng.integers(0, 10, n).astype(np.int32)
            eng.batch_put(t, 900 + bi, 7 + bi, n,
                          [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, k),
                           po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, v)])
            keys.append(k)
            vals.append(v)
            start += n
        v_all = np.concatenate(vals)
        mask = v_all == 3
        assert 0 < mask.sum() < len(mask)
        plan = dict(table=t, preds=[dict(col=1, lo=3, hi=3)])
        rs = eng.select(abi.make_plan(**plan), [abi.PROJ_ROWID, 0])
        assert rs.count() == int(mask.sum())
        assert same_bytes(rs.column(1)[0], np.concatenate(keys)[mask])
        count = abi.make_plan(aggs=[("count", [])], **plan)
        assert eng.query(count).rows()[0][1][0] == float(mask.sum())
        gb, go = rs.rowids()
        for bi in np.unique(gb):
            uuid, bucket = eng.batch_id(t, int(bi))
            assert (uuid, bucket) == (900 + bi, 7 + bi)
            pos = go[gb == bi].astype(np.int32)
            eng.batch_mutate(t, uuid, bucket,
                             delete_mask=po.encode_delete(pos, sizes[bi]))
        rs = eng.select(abi.make_plan(**plan), [abi.PROJ_ROWID, 0])
        assert rs.count() == 0 and rs.rows_passed() == 0
        assert eng.query(count).rows()[0][1][0] == 0.0
        # the other rows are all still there
        rs = eng.select(abi.make_plan(table=t), [0])
        assert same_bytes(rs.column(0)[0], np.concatenate(keys)[~mask])
    finally:
        eng.close()


def test_many_tiles():
    """300 batches of 7 rows: more tiles than k_tile_offsets has lanes."""
    eng = se.Engine(device=0)
    try:
        t = eng.table_define("sel_tiles", [(abi.T_INT32, False),
                                           (abi.T_INT32, False)])
        nb, n = 300, 7
        key = np.arange(nb * n, dtype=np.int32)
        m3 = (key % 3).astype(np.int32)
        for bi in range(nb):
            sl = slice(bi * n, (bi + 1) * n)
            eng.batch_put(t, bi, bi, n,
                          [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, key[sl]),
                           po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, m3[sl])])
        mask = m3 == 0
        assert 0 < mask.sum() < len(mask)
        rs = eng.select(abi.make_plan(table=t, preds=[dict(col=1, lo=0, hi=0)]),
                        [0, abi.PROJ_ROWID])
        assert rs.count() == int(mask.sum())
        assert same_bytes(rs.column(0)[0], key[mask])
        gb, go = rs.rowids()
        assert same_bytes(gb, (key[mask] // n).astype(np.int64))
        assert same_bytes(go, (key[mask] % n).astype(np.int64))
        rs = eng.select(abi.make_plan(table=t, preds=[dict(col=1, lo=0, hi=0)]),
                        [0], limit=257)
        assert same_bytes(rs.column(0)[0], key[mask][:257])
    finally:
        eng.close()
