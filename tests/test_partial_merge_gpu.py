"""sn_query_merge reads blocks that other ranks produced: a block that does
not fit its stride is refused before the query changes, and a NULL group key
is not the text "\\x01".  The byte format itself is covered on the CPU by
test_partial_format_cpu.py; these run it behind a real query handle."""
import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se

pytestmark = pytest.mark.gpu

SLOT = 304          # bytes of one grouped slot; the header is 8


@pytest.fixture(scope="module")
def eng():
    e = se.Engine(device=0)
    yield e
    e.close()


def put(eng, name, keys, vals):
    t = eng.table_define(name, [(abi.T_STRING, True), (abi.T_DOUBLE, False)])
    eng.batch_put(t, 1, 0, len(keys),
                  [po.encode(po.T_STRING, po.ENC_DICT, keys),
                   po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, vals)])
    return t


def refused(q, twin_rows, block, stride):
    with pytest.raises(se.EngineError) as ei:
        q.merge_host(np.ascontiguousarray(block), stride, 1)
    assert ei.value.code == abi.ERR_BADARG
    assert se.last_error()
    assert q.rows() == twin_rows


def test_merge_refuses_bad_blocks(eng):
    n = 64
    keys = [(b"red", b"green", b"blue", None)[i % 4] for i in range(n)]
    # multiples of 0.5: every sum is exact in any order, so the twin query's
    # rows are equal bit for bit
    vals = (np.arange(n, dtype=np.float64) - 20.0) * 0.5
    t = put(eng, "pm_bad", keys, vals)
    aggs = [("sum", [(1, 0.0, 1.0)]), ("min", [(1, 0.0, 1.0)])]

    q = eng.query(abi.make_plan(table=t, group_cols=[0], aggs=aggs))
    twin_rows = eng.query(abi.make_plan(table=t, group_cols=[0], aggs=aggs)).rows()
    assert [k for k, _ in twin_rows] == [("blue",), ("green",), ("red",), (None,)]
    for i, name in enumerate((b"blue", b"green", b"red", None)):
        m = np.array([k == name for k in keys])
        assert twin_rows[i][1] == [float(vals[m].sum()), float(vals[m].min())]
    block = q.partials_host()
    assert int(block[:4].view(np.int32)[0]) == 4
    assert len(block) == 8 + abi.SN_MAX_GROUP_SLOTS * SLOT

    refused(q, twin_rows, block[:8 + SLOT].copy(), 8 + SLOT)   # n is 4
    bad = block.copy()
    bad[:4] = np.array([-1], dtype=np.int32).view(np.uint8)
    refused(q, twin_rows, bad, len(bad))
    bad = block.copy()
    bad[8:8 + 48] = ord("A")                 # slot 0, key 0: no NUL in 48 bytes
    refused(q, twin_rows, bad, len(bad))

    q.merge_host(block, len(block), 1)
    assert q.rows() == twin_rows

    # the keyless form, one byte short
    q = eng.query(abi.make_plan(table=t, aggs=aggs))
    twin_rows = eng.query(abi.make_plan(table=t, aggs=aggs)).rows()
    assert twin_rows == [((), [float(vals.sum()), float(vals.min())])]
    block = q.partials_host()
    assert len(block) == (2 * 2 + 1) * 8
    refused(q, twin_rows, block[:-1].copy(), len(block) - 1)
    q.merge_host(block, len(block), 1)
    assert q.rows() == twin_rows


def test_null_key_is_not_the_text_01(eng):
    keys = [b"\x01", b"b", None, b"\x01", None, b"b", b"\x01", None]
    vals = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0])
    t = put(eng, "pm_ctl", keys, vals)
    plan = dict(table=t, group_cols=[0],
                aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
    want = [(("\x01",), [73.0, 3.0]), (("b",), [34.0, 2.0]),
            ((None,), [148.0, 3.0])]

    q = eng.query(abi.make_plan(**plan))
    assert q.rows() == want
    block = q.partials_host()
    q.merge_host(block, len(block), 1)
    assert q.rows() == want

    q = eng.query(abi.make_plan(**plan))
    shards = q.partials_sharded(2)
    assert sum(int(s[:4].view(np.int32)[0]) for s in shards) == 3
    q.merge_host(np.ascontiguousarray(shards.reshape(-1)), shards.shape[1], 2)
    assert q.rows() == want
