"""Every branch of the put path in one small table, scanned on the GPU.

Three 130-row batches (three null words, the last one partial) of
(k INT32, d DOUBLE, v INT64, s STRING):
  batch 0  ingest_columns: k, d, v down the raw route (device min/max, d with
           3 distinct values gets a code sidecar), s dictionary-encoded;
  batch 1  k LZ4-wrapped (decoded on the device), d Snappy-wrapped, v an
           int dictionary whose nulls are sentinel indices, s a var-width
           string body with nulls;
  batch 2  v run-length encoded, put with a delete mask and a two-deep delta
           on d (value-only: written into the body, sidecar rebuilt) and a
           string delta on s; then changed again through batch_mutate: a new
           mask, a new value-only patch on the narrowed d, a patch with a
           NULL on v.
Values are small integers and dyadic fractions, so every sum is exact and the
results are compared with the CPU oracle for equality, before and after the
mutation.  The oracle cannot read sentinel nulls of an int dictionary, so it
is given the same values of that one column as a plain body with null words
(tests/test_put_stages_cpu.py pins that the engine stores exactly that)."""
import os
import struct

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se
from tests.test_compression import wrap_lz4, wrap_snappy

pytestmark = pytest.mark.gpu

N = 130
K, D, V, S = range(4)
DTYPES = [po.T_INT32, po.T_DOUBLE, po.T_INT64, po.T_STRING]
POOL = [b"A", b"N", b"R", b"xy"]


def columns(b):
    i = np.arange(N)
    k = ((i * 7 + b) % 50).astype(np.int32)
    d = np.array([0.25, 0.5, 1.5])[(i + b) % 3]
    v = ((i // 10) * 3 - 5 + b).astype(np.int64)
    s = [POOL[(j * 3 + b) % 4] for j in range(N)]
    return k, d, v, s


def sentinel_int_dict(vals, valid):
    """BIG_DICTIONARY blob, no null words, nulls as index == dictionary size"""
    dv = sorted(set(int(x) for x, ok in zip(vals, valid) if ok))
    idx = [dv.index(int(x)) if ok else len(dv) for x, ok in zip(vals, valid)]
    return (struct.pack("<3i", po.ENC_BIGDICT, 0, len(dv)) +
            struct.pack(f"<{len(dv)}q", *dv) + struct.pack(f"<{N}i", *idx))


def plans():
    return {
        "keyless": dict(
            preds=[dict(col=K, hi=40)],
            aggs=[("sum", [(D, 0.0, 1.0)]), ("sum", [(K, 0.0, 1.0)]),
                  ("count", []), ("min", [(V, 0.0, 1.0)]),
                  ("max", [(V, 0.0, 1.0)]), ("min", [(D, 0.0, 1.0)])]),
        "by_string": dict(
            group_cols=[S],
            aggs=[("sum", [(D, 0.0, 1.0)]), ("sum", [(K, 0.0, 1.0)]),
                  ("max", [(V, 0.0, 1.0)]), ("count", [])]),
    }


def new_engine():
    old = os.environ.pop("SN_NARROW", None)     # the default: narrowing on
    try:
        return se.Engine(device=0)
    finally:
        if old is not None:
            os.environ["SN_NARROW"] = old


def sorted_rows(rows):
    return sorted(rows, key=lambda r: tuple((x is None, x) for x in r[0]))


def test_every_put_branch_matches_the_oracle():
    k0, d0, v0, s0 = columns(0)
    k1, d1, v1, s1 = columns(1)
    k2, d2, v2, s2 = columns(2)
    v1_valid = (np.arange(N) % 11 != 5).astype(np.uint8)
    s1 = [None if j % 13 == 6 else x for j, x in enumerate(s1)]

    b1 = [wrap_lz4(po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, k1)),
          wrap_snappy(po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, d1)),
          sentinel_int_dict(v1, v1_valid),
          po.encode(po.T_STRING, po.ENC_UNCOMPRESSED, s1)]
    b1_oracle = b1[:V] + [po.encode(po.T_INT64, po.ENC_UNCOMPRESSED, v1,
                                    v1_valid)] + b1[V + 1:]
    b2 = [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, k2),
          po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, d2),
          po.encode(po.T_INT64, po.ENC_RLE, v2),
          po.encode(po.T_STRING, po.ENC_DICT, s2)]

    def i32(*x):
        return np.array(x, dtype=np.int32)

    mask_a = po.encode_delete(i32(3, 64, 129), N)
    deltas_a = [(None, None),
                (po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED,
                                 i32(0, 65, 128), N, np.array([0.5, 0.25, 1.5])),
                 po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED,
                                 i32(0, 7, 66), N, np.array([8.0, 0.25, 0.5]))),
                (None, None),
                (po.encode_delta(po.T_STRING, po.ENC_DICT, i32(1, 70), N,
                                 [b"new", b"A"]), None)]
    # masks and deltas are cumulative: the later state covers every row the
    # earlier one touched
    mask_b = po.encode_delete(i32(3, 5, 64, 100, 129), N)
    deltas_b = [(None, None),
                (po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED,
                                 i32(0, 7, 9, 65, 66, 127, 128), N,
                                 np.array([0.75, 0.25, 0.75, 0.25, 0.5, 0.5,
                                           1.5])), None),
                (po.encode_delta(po.T_INT64, po.ENC_UNCOMPRESSED, i32(2, 67), N,
                                 np.array([1000, 0], dtype=np.int64),
                                 np.array([1, 0], dtype=np.uint8)), None),
                (po.encode_delta(po.T_STRING, po.ENC_DICT, i32(1, 70), N,
                                 [b"new", b"A"]), None)]

    def oracle(mask, deltas):
        ot = po.OracleTable(DTYPES)
        ot.add_batch(N, [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, k0),
                         po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, d0),
                         po.encode(po.T_INT64, po.ENC_UNCOMPRESSED, v0),
                         po.encode(po.T_STRING, po.ENC_DICT, s0)])
        ot.add_batch(N, b1_oracle)
        ot.add_batch(-N, b2, delete_mask=mask, deltas=deltas)
        return {name: sorted_rows(po.result_rows(ot.query(po.make_plan(**p))))
                for name, p in plans().items()}

    eng = new_engine()
    try:
        t = eng.table_define("put_stages", [(abi.T_INT32, False),
                                            (abi.T_DOUBLE, False),
                                            (abi.T_INT64, True),
                                            (abi.T_STRING, True)])
        assert eng.ingest_columns(t, [
            {"data": k0}, {"data": d0}, {"data": v0},
            {"data": b"".join(s0),
             "lens": np.array([len(x) for x in s0], dtype=np.int32)}],
            N, batch_rows=N) == N
        eng.batch_put(t, 1, 1, N, b1)
        eng.batch_put(t, 2, 2, -N, b2, delete_mask=mask_a, deltas=deltas_a)

        def engine_rows():
            return {name: sorted_rows(eng.query(abi.make_plan(table=t, **p)).rows())
                    for name, p in plans().items()}

        before, want = engine_rows(), oracle(mask_a, deltas_a)
        assert before == want
        assert eng.narrowed_batches(t, D) == 3
        assert eng.narrowed_batches(t, K) == 0

        eng.batch_mutate(t, 2, 2, delete_mask=mask_b, deltas=deltas_b)
        after, want = engine_rows(), oracle(mask_b, deltas_b)
        assert after == want
        assert after != before
        assert eng.narrowed_batches(t, D) == 3
    finally:
        eng.close()
