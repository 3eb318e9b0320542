"""The put path's stages on a host-only engine (no GPU needed).

Two groups.  The byte-exact group pins what the put-time re-encodings store:
a var-width string column becomes the BIG_DICTIONARY blob the oracle's encoder
writes for the same values, an int-dictionary column becomes its plain
UNCOMPRESSED blob, and a raw-route column sits next to an encoded one with
one stored blob per column.  The rejection group feeds the smallest corrupt
blob of each kind and checks that the put fails with SN_ERR_BADFORMAT and a
message, appends nothing, changes nothing, and leaves the table usable.
"""
import struct

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se

SN_ERR_BADFORMAT = -4


@pytest.fixture()
def eng():
    e = se.Engine(device=-1)
    yield e
    e.close()


def i32s(*v):
    return struct.pack(f"<{len(v)}i", *v)


def valid_of(vals):
    return np.array([0 if v is None else 1 for v in vals], dtype=np.uint8)


def filled(vals, dtype):
    return np.array([0 if v is None else v for v in vals], dtype=dtype)


def null_words(vals):
    words = [0] * ((len(vals) + 63) // 64)
    for i, v in enumerate(vals):
        if v is None:
            words[i >> 6] |= 1 << (i & 63)
    return struct.pack(f"<{len(words)}Q", *words)


def put_one(eng, dtype, blob, rows, name="t"):
    t = eng.table_define(name, [(dtype, True)])
    eng.batch_put(t, 1, 0, rows, [blob])
    return eng.get_blob(t, 0, 0)


# ---------------------------------------------------------------- byte-exact

def strings_130():
    pool = [b"bb", None, b"a", b"bb", b"ccc", b"", b"dddd"]
    return [pool[(i * 5 + i // 7) % len(pool)] for i in range(130)]


def ints_130():
    pool = [5, 6, None, 7, 9, -3, 1 << 20]
    return [pool[(i * 3 + i // 11) % len(pool)] for i in range(130)]


@pytest.mark.parametrize("vals", [[b"bb", None, b"a", b"bb", b"ccc"],
                                  strings_130()], ids=["5rows", "130rows"])
def test_varwidth_strings_become_big_dictionary(eng, vals):
    blob = po.encode(po.T_STRING, po.ENC_UNCOMPRESSED, vals)
    assert put_one(eng, abi.T_STRING, blob, len(vals)) == \
        po.encode(po.T_STRING, po.ENC_BIGDICT, vals)


@pytest.mark.parametrize("dtype,enc,np_t", [
    (po.T_INT64, po.ENC_DICT, np.int64), (po.T_INT32, po.ENC_BIGDICT, np.int32),
    (po.T_INT64, po.ENC_BIGDICT, np.int64), (po.T_INT32, po.ENC_DICT, np.int32)],
    ids=["i64_dict", "i32_bigdict", "i64_bigdict", "i32_dict"])
@pytest.mark.parametrize("vals", [[5, 6, None, 7, 9], ints_130()],
                         ids=["5rows", "130rows"])
def test_int_dictionary_stored_as_plain_body(eng, dtype, enc, np_t, vals):
    arr, valid = filled(vals, np_t), valid_of(vals)
    blob = po.encode(dtype, enc, arr, valid)
    assert put_one(eng, dtype, blob, len(vals)) == \
        po.encode(dtype, po.ENC_UNCOMPRESSED, arr, valid)


def sentinel_blob(vals, type_id, value_fmt):
    """int dictionary blob whose nulls are sentinel indices (== dictionary
    size), with no null bitset at all"""
    dict_vals = sorted({v for v in vals if v is not None})
    idx = [len(dict_vals) if v is None else dict_vals.index(v) for v in vals]
    ifmt = "h" if type_id == po.ENC_DICT else "i"
    return (i32s(type_id, 0, len(dict_vals)) +
            struct.pack(f"<{len(dict_vals)}{value_fmt}", *dict_vals) +
            struct.pack(f"<{len(idx)}{ifmt}", *idx))


@pytest.mark.parametrize("type_id", [po.ENC_DICT, po.ENC_BIGDICT],
                         ids=["dict", "bigdict"])
@pytest.mark.parametrize("vals", [[5, 6, None, 7, 9], ints_130()],
                         ids=["5rows", "130rows"])
def test_sentinel_nulls_fold_into_the_null_words(eng, type_id, vals):
    blob = sentinel_blob(vals, type_id, "q")
    assert put_one(eng, abi.T_INT64, blob, len(vals)) == po.encode(
        po.T_INT64, po.ENC_UNCOMPRESSED, filled(vals, np.int64), valid_of(vals))


def test_sentinel_nulls_merge_with_bitset_nulls(eng):
    """130 rows: rows 0 and 129 are null in the bitset (three words, the last
    one partial), every seventh other row is a sentinel index"""
    vals = [None if i in (0, 129) or i % 7 == 3 else i % 5 for i in range(130)]
    in_bitset = [None if i in (0, 129) else 1 for i in range(130)]
    idx = [5 if v is None else v for i, v in enumerate(vals)
           if in_bitset[i] is not None]
    blob = (i32s(po.ENC_BIGDICT, 24) + null_words(in_bitset) +
            i32s(5, 0, 1, 2, 3, 4) + i32s(*idx))
    assert put_one(eng, abi.T_INT32, blob, 130) == po.encode(
        po.T_INT32, po.ENC_UNCOMPRESSED, filled(vals, np.int32), valid_of(vals))


def test_raw_column_next_to_encoded_string_column(eng):
    """ingest_columns sends the null-free int column down the raw route and
    the string column as an encoded blob; each keeps its own stored blob, in
    column order"""
    n, rows = 300, 130
    i32 = (np.arange(n, dtype=np.int32) * 7) % 1000
    svals = [strings_130()[i % 130] for i in range(n)]
    f64 = np.arange(n) / 8.0
    t = eng.table_define("t_mix", [(abi.T_INT32, False), (abi.T_STRING, True),
                                   (abi.T_DOUBLE, False)])
    lens = np.array([len(v or b"") for v in svals], dtype=np.int32)
    got = eng.ingest_columns(t, [
        {"data": i32},
        {"data": b"".join(v or b"" for v in svals), "lens": lens,
         "valid": valid_of(svals)},
        {"data": f64}], n, batch_rows=rows)
    assert got == n and eng.num_batches(t) == 3
    for b in range(3):
        s, e_ = b * rows, min(n, (b + 1) * rows)
        assert eng.get_blob(t, b, 0) == po.encode(
            po.T_INT32, po.ENC_UNCOMPRESSED, i32[s:e_])
        assert eng.get_blob(t, b, 1) == po.encode(
            po.T_STRING, po.ENC_DICT, svals[s:e_])
        assert eng.get_blob(t, b, 2) == po.encode(
            po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64[s:e_])


# ---------------------------------------------------------------- rejections

def expect_badformat(call):
    with pytest.raises(se.EngineError) as ex:
        call()
    assert ex.value.code == SN_ERR_BADFORMAT, ex.value
    assert se.last_error()


def delta_blob(type_id, positions, body, nulls=b"", num_base_rows=1000):
    head = i32s(type_id, len(nulls)) + nulls + \
        i32s(num_base_rows, len(positions)) + i32s(*positions)
    return head + b"\0" * (-len(head) % 8) + body


F64 = lambda *v: struct.pack(f"<{len(v)}d", *v)          # noqa: E731
SDICT = i32s(2) + i32s(1) + b"x" + i32s(2) + b"yz"       # 2 entries: x, yz

# column-blob cases: (id, dtype, rows, good blob, [bad blobs])
SHORT_BODY = [
    ("f64_100rows_50values", abi.T_DOUBLE, 100,
     lambda: po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, np.arange(100.0)),
     lambda g: [g[:8 + 50 * 8], g[:-1], g[:8]]),
    ("i32_nulls_one_value_short", abi.T_INT32, 5,
     lambda: po.encode(po.T_INT32, po.ENC_UNCOMPRESSED,
                       filled([1, None, 3, 4, 5], np.int32),
                       valid_of([1, None, 3, 4, 5])),
     lambda g: [g[:-4], g[:-1]]),
    ("i16_one_byte_short", abi.T_INT16, 3,
     lambda: po.encode(po.T_INT16, po.ENC_UNCOMPRESSED,
                       np.array([1, 2, 3], dtype=np.int16)),
     lambda g: [g[:-1]]),
    ("bool_one_byte_short", abi.T_BOOL, 3,
     lambda: po.encode(po.T_BOOL, po.ENC_UNCOMPRESSED,
                       np.array([1, 0, 1], dtype=np.uint8)),
     lambda g: [g[:-1]]),
    ("i64_dictionary_entries_cut", abi.T_INT64, 2,
     lambda: i32s(po.ENC_BIGDICT, 0, 2) + struct.pack("<2q", 7, 8) + i32s(0, 1),
     # count says 2 entries, bytes for one and a half; count far past the blob
     lambda g: [g[:12 + 12], i32s(po.ENC_BIGDICT, 0, 0x7fffffff) + g[12:]]),
    ("string_dictionary_negative_size", abi.T_STRING, 2,
     lambda: i32s(po.ENC_BIGDICT, 0) + SDICT + i32s(0, 1),
     lambda g: [g[:12] + i32s(-1) + g[16:], g[:12] + i32s(-2**31) + g[16:]]),
    ("varwidth_string_negative_size", abi.T_STRING, 2,
     lambda: po.encode(po.T_STRING, po.ENC_UNCOMPRESSED, [b"ab", b"c"]),
     lambda g: [g[:8] + i32s(-1) + g[12:], g[:-1]]),
]


@pytest.mark.parametrize("case", SHORT_BODY, ids=[c[0] for c in SHORT_BODY])
def test_short_or_corrupt_column_blob_rejected(eng, case):
    _, dtype, rows, make_good, make_bad = case
    good = make_good()
    t = eng.table_define("t_rej", [(dtype, True)])
    eng.batch_put(t, 1, 0, rows, [good])
    stored = eng.get_blob(t, 0, 0)
    for i, bad in enumerate(make_bad(good)):
        expect_badformat(lambda: eng.batch_put(t, 10 + i, 0, rows, [bad]))
        assert eng.num_rows(t) == rows and eng.num_batches(t) == 1
        assert eng.get_blob(t, 0, 0) == stored
    eng.batch_put(t, 2, 0, rows, [good])
    assert eng.num_rows(t) == 2 * rows


GOOD_F64_DELTA = delta_blob(po.ENC_UNCOMPRESSED, [1, 5, 9], F64(1.0, 2.0, 3.0))
GOOD_SDICT_DELTA = delta_blob(po.ENC_BIGDICT, [1, 5, 9], SDICT + i32s(0, 1, 2))
GOOD_SVAR_DELTA = delta_blob(po.ENC_UNCOMPRESSED, [1, 5],
                             i32s(1) + b"x" + i32s(2) + b"yz")
GOOD_IDICT_DELTA = delta_blob(po.ENC_DICT, [1, 5], i32s(2) +
                              struct.pack("<2q", 70, 80) +
                              struct.pack("<2h", 1, 0))

# delta cases: (id, dtype, good delta, [bad deltas])
BAD_DELTAS = [
    ("f64_56_bytes_cut_to_40", abi.T_DOUBLE, GOOD_F64_DELTA,
     [GOOD_F64_DELTA[:40], GOOD_F64_DELTA[:55]]),
    ("positions_cut", abi.T_DOUBLE, GOOD_F64_DELTA,
     [GOOD_F64_DELTA[:24], GOOD_F64_DELTA[:12],
      i32s(po.ENC_UNCOMPRESSED, 0, 1000, 0x7fffffff) + GOOD_F64_DELTA[16:],
      i32s(po.ENC_UNCOMPRESSED, 0, 1000, -1) + GOOD_F64_DELTA[16:]]),
    ("null_words_past_the_end", abi.T_DOUBLE, GOOD_F64_DELTA,
     [i32s(po.ENC_UNCOMPRESSED, 1 << 20) + GOOD_F64_DELTA[8:]]),
    ("dictionary_count_missing", abi.T_STRING, GOOD_SDICT_DELTA,
     [GOOD_SDICT_DELTA[:32], GOOD_SDICT_DELTA[:34]]),
    ("dictionary_entries_cut", abi.T_STRING, GOOD_SDICT_DELTA,
     [GOOD_SDICT_DELTA[:38], GOOD_SDICT_DELTA[:41], GOOD_SDICT_DELTA[:46],
      GOOD_SDICT_DELTA[:32] + i32s(0x7fffffff) + GOOD_SDICT_DELTA[36:]]),
    ("dictionary_negative_string_size", abi.T_STRING, GOOD_SDICT_DELTA,
     [GOOD_SDICT_DELTA[:36] + i32s(-1) + GOOD_SDICT_DELTA[40:]]),
    ("dictionary_indices_cut", abi.T_STRING, GOOD_SDICT_DELTA,
     [GOOD_SDICT_DELTA[:-1], GOOD_SDICT_DELTA[:-8]]),
    ("dictionary_index_negative", abi.T_STRING, GOOD_SDICT_DELTA,
     [GOOD_SDICT_DELTA[:-4] + i32s(-1)]),
    ("dictionary_index_above_size", abi.T_STRING, GOOD_SDICT_DELTA,
     [GOOD_SDICT_DELTA[:-4] + i32s(3), GOOD_SDICT_DELTA[:-4] + i32s(0x7fffffff)]),
    ("int_dictionary_index_above_size", abi.T_INT64, GOOD_IDICT_DELTA,
     [GOOD_IDICT_DELTA[:-2] + struct.pack("<h", 3),
      GOOD_IDICT_DELTA[:-2] + struct.pack("<h", -1)]),
    ("int_dictionary_entries_cut", abi.T_INT64, GOOD_IDICT_DELTA,
     [GOOD_IDICT_DELTA[:36], GOOD_IDICT_DELTA[:-1]]),
    ("varwidth_string_size", abi.T_STRING, GOOD_SVAR_DELTA,
     [GOOD_SVAR_DELTA[:24] + i32s(-1) + GOOD_SVAR_DELTA[28:],
      GOOD_SVAR_DELTA[:-1], GOOD_SVAR_DELTA[:30]]),
]


def base_column(dtype):
    if dtype == abi.T_STRING:
        return po.encode(po.T_STRING, po.ENC_DICT, [b"a", b"b"] * 500)
    np_t = np.float64 if dtype == abi.T_DOUBLE else np.int64
    return po.encode(dtype, po.ENC_UNCOMPRESSED, np.arange(1000, dtype=np_t))


@pytest.mark.parametrize("case", BAD_DELTAS, ids=[c[0] for c in BAD_DELTAS])
def test_corrupt_delta_rejected_by_put_and_mutate(eng, case):
    _, dtype, good, bads = case
    n = 1000
    base = base_column(dtype)
    t = eng.table_define("t_delta", [(dtype, True)])
    eng.batch_put(t, 1, 0, n, [base])
    stored = eng.get_blob(t, 0, 0)
    for i, bad in enumerate(bads):
        for slot in ((bad, None), (None, bad)):
            expect_badformat(
                lambda: eng.batch_put(t, 10 + i, 0, -n, [base], deltas=[slot]))
            expect_badformat(lambda: eng.batch_mutate(t, 1, 0, deltas=[slot]))
            assert eng.num_rows(t) == n and eng.num_batches(t) == 1
            assert eng.get_blob(t, 0, 0) == stored
    eng.batch_mutate(t, 1, 0, deltas=[(good, None)])
    eng.batch_put(t, 2, 0, -n, [base], deltas=[(good, good)])
    assert eng.num_rows(t) == 2 * n and eng.get_blob(t, 1, 0) == stored


def test_delta_null_sentinel_index_still_accepted(eng):
    """an index equal to the dictionary size is the NULL sentinel of a string
    delta, not an error"""
    t = eng.table_define("t_sent", [(abi.T_STRING, True)])
    eng.batch_put(t, 1, 0, 1000, [base_column(abi.T_STRING)])
    eng.batch_mutate(t, 1, 0, deltas=[
        (GOOD_SDICT_DELTA[:-4] + i32s(2), None)])
    d16 = delta_blob(po.ENC_DICT, [3, 4], SDICT + struct.pack("<2h", 2, 1))
    eng.batch_mutate(t, 1, 0, deltas=[(d16, None)])


def test_project_encoders_still_load(eng):
    """the deltas and masks the project's own encoders write pass the checks"""
    n = 1000
    t = eng.table_define("t_enc", [(abi.T_DOUBLE, True), (abi.T_STRING, True)])
    cols = [base_column(abi.T_DOUBLE), base_column(abi.T_STRING)]
    pos = np.array([2, 3, 900], dtype=np.int32)
    vv = np.array([1, 0, 1], dtype=np.uint8)
    deltas = [
        (po.encode_delta(po.T_DOUBLE, po.ENC_UNCOMPRESSED, pos, n,
                         np.array([1.5, 0.0, 2.5]), vv),
         se.encode_update_delta(abi.T_DOUBLE, pos[:1], n, np.array([9.0]))),
        (po.encode_delta(po.T_STRING, po.ENC_DICT, pos, n, [b"q", None, b"a"]),
         po.encode_delta(po.T_STRING, po.ENC_UNCOMPRESSED, pos, n,
                         [b"zz", b"", b"q"]))]
    eng.batch_put(t, 1, 0, -n, cols, delete_mask=po.encode_delete(pos, n),
                  deltas=deltas)
    eng.batch_mutate(t, 1, 0, deltas=deltas,
                     delete_mask=se.encode_delete_mask(pos, n))
    assert eng.num_rows(t) == n
