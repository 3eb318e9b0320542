"""LZ4 compression wrapper (CompressionUtils.scala:53-61:
[int32 -codecId][int32 uncompressedLen][payload], LZ4 = codec 1).
Compression here is done directly through liblz4 (the same library the
reference's lz4-java binds); engine and oracle must both transparently
decompress on put."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se


def lz4():
    for name in ("liblz4.so.1", "liblz4.so"):
        try:
            lib = C.CDLL(name)
            lib.LZ4_compress_default.restype = C.c_int
            lib.LZ4_compressBound.restype = C.c_int
            return lib
        except OSError:
            continue
    pytest.skip("liblz4 not available")


def wrap_lz4(blob):
    L = lz4()
    bound = L.LZ4_compressBound(len(blob))
    out = C.create_string_buffer(bound)
    n = L.LZ4_compress_default(blob, out, len(blob), bound)
    assert n > 0
    hdr = (-1).to_bytes(4, "little", signed=True) + len(blob).to_bytes(4, "little")
    return hdr + out.raw[:n]


def test_oracle_accepts_lz4_wrapped_blobs():
    n = 50_000
    rng = np.random.default_rng(21)
    i32 = rng.integers(0, 100, n).astype(np.int32)   # repetitive: compresses
    f64 = rng.random(n)
    plain = [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, i32),
             po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)]
    wrapped = [wrap_lz4(b) for b in plain]
    assert len(wrapped[0]) < len(plain[0])   # actually compressed
    plan = po.make_plan(preds=[dict(col=0, hi=50, hi_strict=True)],
                        aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
    t1 = po.OracleTable([po.T_INT32, po.T_DOUBLE])
    t1.add_batch(n, plain)
    t2 = po.OracleTable([po.T_INT32, po.T_DOUBLE])
    t2.add_batch(n, wrapped)
    assert po.result_rows(t1.query(plan)) == po.result_rows(t2.query(plan))


def test_engine_hostonly_decompresses_on_put():
    n = 20_000
    rng = np.random.default_rng(22)
    f64 = np.round(rng.random(n), 2)
    plain = po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)
    e = se.Engine(device=-1)
    t = e.table_define("tz", [(abi.T_DOUBLE, False)])
    e.batch_put(t, 0, 0, n, [wrap_lz4(plain)])
    assert e.get_blob(t, 0, 0) == plain    # stored decompressed
    e.close()


@pytest.mark.gpu
def test_engine_gpu_lz4_parity():
    n = 500_000
    rng = np.random.default_rng(23)
    i32 = rng.integers(0, 1000, n).astype(np.int32)
    f64 = np.round(rng.random(n), 3)
    plain = [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, i32),
             po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)]
    eng = se.Engine(device=0)
    t = eng.table_define("tz", [(abi.T_INT32, False), (abi.T_DOUBLE, False)])
    eng.batch_put(t, 0, 0, n, [wrap_lz4(b) for b in plain])
    plan = abi.make_plan(table=t, preds=[dict(col=0, hi=500, hi_strict=True)],
                         aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
    rows = eng.query(plan).rows()
    m = i32 < 500
    assert rows[0][1][1] == float(m.sum())
    assert abs(rows[0][1][0] - f64[m].sum()) <= 1e-6 * abs(f64[m].sum())
    eng.close()


# ---- Snappy (codec 2) ----

def snappy_compress(data: bytes) -> bytes:
    """Minimal valid raw-Snappy compressor (greedy 4-byte hash matching) for
    test-vector generation; the product/oracle only DECODE (the reference's
    snappy-java compresses on the JVM side)."""
    out = bytearray()
    n = len(data)
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            break

    def emit_literal(lit):
        while lit:
            chunk, lit = lit[:0x10000], lit[0x10000:]
            ln = len(chunk) - 1
            if ln < 60:
                out.append(ln << 2)
            elif ln < 0x100:
                out.append(60 << 2)
                out.append(ln)
            else:
                out.append(61 << 2)
                out.extend(ln.to_bytes(2, "little"))
            out.extend(chunk)

    table = {}
    i = 0
    lit_start = 0
    while i + 4 <= len(data):
        key = data[i:i + 4]
        j = table.get(key)
        table[key] = i
        if j is not None and i - j <= 0xFFFF:
            m = 4
            while i + m < len(data) and m < 64 and data[j + m] == data[i + m]:
                m += 1
            emit_literal(data[lit_start:i])
            off = i - j
            # 2-byte-offset copy: len 1..64
            out.append(((m - 1) << 2) | 2)
            out.extend(off.to_bytes(2, "little"))
            i += m
            lit_start = i
        else:
            i += 1
    emit_literal(data[lit_start:])
    return bytes(out)


def wrap_snappy(blob):
    hdr = (-2).to_bytes(4, "little", signed=True) + len(blob).to_bytes(4, "little")
    return hdr + snappy_compress(blob)


# ---- scripted raw-Snappy streams: every element form, checked against a
# pure-Python decoder written from the format description ----

SN_ERR_BADFORMAT = -4


def sn_varint(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def sn_lit(data, form=0):
    """Literal element; form 0 = inline length (<= 60 bytes), 1/2/3 = that
    many explicit little-endian length bytes (tags 60/61/62)."""
    ln = len(data) - 1
    assert ln >= 0
    if form == 0:
        assert ln < 60
        return bytes([ln << 2]) + data
    assert ln < 1 << (8 * form)
    return bytes([(59 + form) << 2]) + ln.to_bytes(form, "little") + data


def sn_copy(off, n, form):
    """Copy element with a 1-, 2- or 4-byte offset."""
    if form == 1:
        assert 4 <= n <= 11 and 0 <= off < 2048
        return bytes([((off >> 8) << 5) | ((n - 4) << 2) | 1, off & 0xFF])
    assert 1 <= n <= 64 and 0 <= off < 1 << (8 * form)
    return bytes([((n - 1) << 2) | (2 if form == 2 else 3)]) + \
        off.to_bytes(form, "little")


def snappy_decode_py(stream):
    """Reference decoder, straight from the format description: returns
    (bytes, {element form: count}).  Raises ValueError on a bad stream."""
    ip = ulen = shift = 0
    while True:
        b = stream[ip]; ip += 1
        ulen |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    out = bytearray()
    forms = {}
    while ip < len(stream):
        tag = stream[ip]; ip += 1
        kind = tag & 3
        if kind == 0:
            n = tag >> 2
            nb = 0
            if n >= 60:
                nb = n - 59
                if ip + nb > len(stream):
                    raise ValueError("literal length past the end")
                n = int.from_bytes(stream[ip:ip + nb], "little"); ip += nb
            n += 1
            if ip + n > len(stream):
                raise ValueError("literal past the end")
            out += stream[ip:ip + n]; ip += n
            forms["lit%d" % nb] = forms.get("lit%d" % nb, 0) + 1
            continue
        nb = 1 if kind == 1 else 2 if kind == 2 else 4
        if ip + nb > len(stream):
            raise ValueError("copy offset past the end")
        if kind == 1:
            n = ((tag >> 2) & 7) + 4
            off = ((tag >> 5) << 8) | stream[ip]; ip += 1
        else:
            n = (tag >> 2) + 1
            off = int.from_bytes(stream[ip:ip + nb], "little"); ip += nb
        if off == 0 or off > len(out):
            raise ValueError("bad copy offset")
        for _ in range(n):                      # byte by byte: may overlap
            out.append(out[-off])
        key = "copy%d" % (1 if kind == 1 else 2 if kind == 2 else 4)
        forms[key] = forms.get(key, 0) + 1
        if off < n:
            forms["overlap"] = forms.get("overlap", 0) + 1
        if kind == 1 and off >= 256:
            forms["copy1_hi"] = forms.get("copy1_hi", 0) + 1
    if len(out) != ulen:
        raise ValueError("length mismatch")
    return bytes(out), forms


def snappy_elements(data, copy_form, lit_form):
    """Greedy matcher emitting ONLY the requested forms where the format
    allows them (a 1-byte-offset copy needs length 4-11 and offset < 2048;
    anything else falls back to the 2-byte form).  Returns the element list;
    the stream is sn_varint(len(data)) + b"".join(elements)."""
    els = []

    def emit_literal(lit):
        cap = 60 if lit_form == 0 else 1 << (8 * min(lit_form, 2))
        while lit:
            chunk, lit = lit[:cap], lit[cap:]
            els.append(sn_lit(chunk, lit_form))

    table = {}
    i = lit_start = 0
    maxlen = 11 if copy_form == 1 else 64
    while i + 4 <= len(data):
        key = data[i:i + 4]
        j = table.get(key)
        table[key] = i
        if j is None or i - j > 0xFFFF:
            i += 1
            continue
        m = 4
        while i + m < len(data) and m < maxlen and data[j + m] == data[i + m]:
            m += 1
        emit_literal(data[lit_start:i])
        off = i - j
        els.append(sn_copy(off, m, copy_form if (copy_form != 1 or off < 2048)
                           else 2))
        i += m
        lit_start = i
    emit_literal(data[lit_start:])
    return els


def wrap_codec2(plain_len, stream):
    return (-2).to_bytes(4, "little", signed=True) + \
        plain_len.to_bytes(4, "little") + stream


def int32_blob(n=5000, seed=34):
    """~5,000 INT32 rows: runs (overlapping offset-4 copies), values from a
    set of 300 (copies at offsets on both sides of 256 and 2048) and a
    stretch of noise (long literals)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 300, n).astype(np.int32)
    v[1000:1400] = 7
    v[2000:2300] = rng.integers(-2 ** 31, 2 ** 31 - 1, 300)
    return v, po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, v)


def assert_engine_and_oracle_decode(plain, wrapped, n):
    """Host engine stores the plain bytes; the oracle computes the same
    aggregates from the wrapped blob as from the plain one."""
    e = se.Engine(device=-1)
    try:
        t = e.table_define("tsn", [(abi.T_INT32, False)])
        e.batch_put(t, 0, 0, n, [wrapped])
        assert e.get_blob(t, 0, 0) == plain
    finally:
        e.close()
    plan = po.make_plan(aggs=[("sum", [(0, 0.0, 1.0)]), ("min", [(0, 0.0, 1.0)]),
                              ("max", [(0, 0.0, 1.0)]), ("count", [])])
    t1 = po.OracleTable([po.T_INT32])
    t1.add_batch(n, [plain])
    t2 = po.OracleTable([po.T_INT32])
    t2.add_batch(n, [wrapped])
    r1, r2 = po.result_rows(t1.query(plan)), po.result_rows(t2.query(plan))
    assert r1 == r2 and r1[0][1][3] == float(n)


def handcrafted_overlap_stream():
    """A 6-row INT32 column blob written by hand: header and two zero rows
    from one zero byte + copy(off=1, len=15); four rows of b'abcd' from the
    literal + copy(off=4, len=12).  Both copies overlap their own output."""
    els = [sn_lit(b"\0"), sn_copy(1, 15, 2), sn_lit(b"abcd"), sn_copy(4, 12, 2)]
    return sn_varint(32) + b"".join(els), els


def test_snappy_decoder_handcrafted_overlap():
    """Overlapping copy semantics: a copy whose offset is smaller than its
    length repeats the pattern byte by byte."""
    stream, _ = handcrafted_overlap_stream()
    rows = np.array([0, 0] + [int.from_bytes(b"abcd", "little")] * 4,
                    dtype=np.int32)
    plain = po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, rows)
    assert plain == b"\0" * 16 + b"abcd" * 4
    decoded, forms = snappy_decode_py(stream)
    assert decoded == plain and forms["overlap"] == 2
    assert_engine_and_oracle_decode(plain, wrap_codec2(len(plain), stream), 6)


SNAPPY_FORMS = [  # (copy form, literal form, what the walk must find)
    (1, 0, ("copy1", "copy1_hi", "lit0", "overlap")),
    (2, 1, ("copy2", "lit1", "overlap")),
    (4, 2, ("copy4", "lit2", "overlap")),
    (2, 3, ("copy2", "lit3")),
]


@pytest.mark.parametrize("copy_form,lit_form,expect", SNAPPY_FORMS,
                         ids=["copy1_inline", "copy2_len1", "copy4_len2",
                              "copy2_len3"])
def test_snappy_element_forms(copy_form, lit_form, expect):
    v, plain = int32_blob()
    stream = sn_varint(len(plain)) + \
        b"".join(snappy_elements(plain, copy_form, lit_form))
    assert len(sn_varint(len(plain))) == 3            # multi-byte varint
    # the encoder is right independently of the engine
    decoded, forms = snappy_decode_py(stream)
    assert decoded == plain
    for key in expect:
        assert forms.get(key, 0) > 0, (key, forms)
    if copy_form != 4:                  # 5-byte copies of 4-byte matches grow
        assert len(stream) < len(plain)
    assert_engine_and_oracle_decode(plain, wrap_codec2(len(plain), stream),
                                    len(v))


def test_greedy_test_compressor_emits_valid_snappy():
    """snappy_compress above feeds the older parity tests; the reference
    decoder vouches for its streams without the engine."""
    data = b"abcdabcdabcdXYZ" * 9 + bytes(range(256)) * 2
    decoded, forms = snappy_decode_py(snappy_compress(data))
    assert decoded == data and forms["copy2"] > 0


def put_expect_badformat(blob, n=6):
    e = se.Engine(device=-1)
    try:
        t = e.table_define("tbad", [(abi.T_INT32, False)])
        with pytest.raises(se.EngineError) as ei:
            e.batch_put(t, 0, 0, n, [blob])
        assert ei.value.code == SN_ERR_BADFORMAT, ei.value
        assert se.last_error() != ""
        assert e.num_batches(t) == 0
    finally:
        e.close()


def mixed_form_stream():
    """Small valid INT32 blob (16 rows) using every element form once."""
    body = b"\0" * 8 + b"abcdefgh" * 8
    els = [sn_lit(b"\0"), sn_copy(1, 7, 1),           # header: 1-byte-offset
           sn_lit(b"abcd", 1), sn_lit(b"efgh", 2),    # explicit length bytes
           sn_copy(8, 24, 2),                         # overlapping 2-byte copy
           sn_lit(b"abcdefgh", 3),
           sn_copy(16, 16, 4),                        # 4-byte offset
           sn_copy(8, 8, 1)]
    stream = sn_varint(len(body)) + b"".join(els)
    decoded, forms = snappy_decode_py(stream)
    assert decoded == body
    assert set(forms) >= {"lit0", "lit1", "lit2", "lit3", "copy1", "copy2",
                          "copy4", "overlap"}
    return body, els


def test_snappy_mixed_forms_decode():
    body, els = mixed_form_stream()
    stream = sn_varint(len(body)) + b"".join(els)
    assert_engine_and_oracle_decode(body, wrap_codec2(len(body), stream), 16)


def test_snappy_truncated_streams_rejected():
    body, els = mixed_form_stream()
    head = sn_varint(len(body))
    stream = head + b"".join(els)
    cuts = set()
    pos = len(head)
    for el in els:
        for c in (pos - 1, pos, pos + 1):
            if 0 < c < len(stream):
                cuts.add(c)
        pos += len(el)
    cuts.add(len(stream) - 1)
    assert len(cuts) >= 2 * len(els)
    for c in sorted(cuts):
        with pytest.raises(ValueError):
            snappy_decode_py(stream[:c] + b"")        # the reference agrees
        put_expect_badformat(wrap_codec2(len(body), stream[:c]), 16)


def test_snappy_inconsistent_streams_rejected():
    body, els = mixed_form_stream()
    n = len(body)
    data = b"".join(els)
    bad = {
        "wrapper length too long": wrap_codec2(n + 1, sn_varint(n) + data),
        "wrapper length too short": wrap_codec2(n - 1, sn_varint(n) + data),
        "stream length too long": wrap_codec2(n, sn_varint(n + 1) + data),
        "stream length too short": wrap_codec2(n, sn_varint(n - 1) + data),
        "both lengths too long": wrap_codec2(n + 4, sn_varint(n + 4) + data),
        "both lengths too short": wrap_codec2(n - 4, sn_varint(n - 4) + data),
    }
    for form in (1, 2, 4):
        tail = sn_lit(b"\0" * 8 + b"abcd") + b"%s" + sn_lit(b"wxyz" * 5)
        m = 12 + 4 + 20
        bad["copy%d offset 0" % form] = wrap_codec2(
            m, sn_varint(m) + tail % sn_copy(0, 4, form))
        bad["copy%d offset past the output" % form] = wrap_codec2(
            m, sn_varint(m) + tail % sn_copy(13, 4, form))
        ok = wrap_codec2(m, sn_varint(m) + tail % sn_copy(12, 4, form))
        e = se.Engine(device=-1)                # offset == output so far: valid
        try:
            t = e.table_define("tok", [(abi.T_INT32, False)])
            e.batch_put(t, 0, 0, 7, [ok])
            assert e.get_blob(t, 0, 0) == b"\0" * 8 + b"abcd" + b"\0" * 4 + \
                b"wxyz" * 5
        finally:
            e.close()
    for what, blob in bad.items():
        put_expect_badformat(blob, 16)


def test_lz4_truncated_and_mislabelled_rejected():
    v, plain = int32_blob()
    good = wrap_lz4(plain)
    e = se.Engine(device=-1)
    try:
        t = e.table_define("tlz", [(abi.T_INT32, False)])
        e.batch_put(t, 0, 0, len(v), [good])
        assert e.get_blob(t, 0, 0) == plain
    finally:
        e.close()
    n = len(plain)
    put_expect_badformat(good[:-1], len(v))
    put_expect_badformat(good[:4] + (n + 1).to_bytes(4, "little") + good[8:],
                         len(v))
    put_expect_badformat(good[:4] + (n - 1).to_bytes(4, "little") + good[8:],
                         len(v))


def test_oracle_accepts_snappy_wrapped_blobs():
    n = 50_000
    rng = np.random.default_rng(31)
    i32 = rng.integers(0, 50, n).astype(np.int32)    # repetitive: real copies
    f64 = np.repeat(rng.random(n // 100), 100)[:n]   # runs: copies in f64 too
    plain = [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, i32),
             po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)]
    wrapped = [wrap_snappy(b) for b in plain]
    assert len(wrapped[0]) < len(plain[0])           # actually compressed
    plan = po.make_plan(preds=[dict(col=0, hi=25, hi_strict=True)],
                        aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
    t1 = po.OracleTable([po.T_INT32, po.T_DOUBLE])
    t1.add_batch(n, plain)
    t2 = po.OracleTable([po.T_INT32, po.T_DOUBLE])
    t2.add_batch(n, wrapped)
    assert po.result_rows(t1.query(plan)) == po.result_rows(t2.query(plan))


def test_engine_hostonly_snappy_decompresses_on_put():
    n = 20_000
    rng = np.random.default_rng(32)
    f64 = np.repeat(np.round(rng.random(n // 50), 2), 50)[:n]
    plain = po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)
    e = se.Engine(device=-1)
    t = e.table_define("tsz", [(abi.T_DOUBLE, False)])
    e.batch_put(t, 0, 0, n, [wrap_snappy(plain)])
    assert e.get_blob(t, 0, 0) == plain
    e.close()


@pytest.mark.gpu
def test_engine_gpu_snappy_parity():
    n = 500_000
    rng = np.random.default_rng(33)
    i32 = rng.integers(0, 200, n).astype(np.int32)
    f64 = np.repeat(np.round(rng.random(n // 20), 3), 20)[:n]
    plain = [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, i32),
             po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64)]
    eng = se.Engine(device=0)
    t = eng.table_define("tsz", [(abi.T_INT32, False), (abi.T_DOUBLE, False)])
    eng.batch_put(t, 0, 0, n, [wrap_snappy(b) for b in plain])
    plan = abi.make_plan(table=t, preds=[dict(col=0, hi=100, hi_strict=True)],
                         aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
    rows = eng.query(plan).rows()
    m = i32 < 100
    assert rows[0][1][1] == float(m.sum())
    assert abs(rows[0][1][0] - f64[m].sum()) <= 1e-6 * abs(f64[m].sum())
    eng.close()


@pytest.mark.gpu
def test_gpu_lz4_device_decode_stress():
    """f1 compressed-upload: LZ4 blobs now ship compressed over PCIe and
    decode wave-cooperatively on device (k_lz4_decompress).  Stress the
    decoder with highly repetitive data (long matches + overlapping
    offsets + extended length bytes) and a dictionary string column, then
    parity-check the scan against the plain-blob table."""
    n = 400_000
    rng = np.random.default_rng(23)
    # long runs -> matches with small offsets and 15+ extended lengths
    i32 = np.repeat(rng.integers(0, 5, 2000), 200)[:n].astype(np.int32)
    f64 = np.round(rng.random(n), 1)            # repetitive doubles
    keys = [b"K%d" % v for v in rng.integers(0, 3, n)]
    plain = [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, i32),
             po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, f64),
             po.encode(po.T_STRING, po.ENC_DICT, keys)]
    wrapped = [wrap_lz4(b) for b in plain]
    assert sum(map(len, wrapped)) < sum(map(len, plain)) // 2

    eng = se.Engine(device=0)
    try:
        schema = [(abi.T_INT32, False), (abi.T_DOUBLE, False),
                  (abi.T_STRING, False)]
        t1 = eng.table_define("lzplain", schema)
        eng.batch_put(t1, 0, 0, n, plain)
        t2 = eng.table_define("lzwrap", schema)
        eng.batch_put(t2, 0, 0, n, wrapped)
        plan_kw = dict(preds=[dict(col=0, hi=2)],
                       group_cols=[2],
                       aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
        r1 = eng.query(abi.make_plan(table=t1, **plan_kw)).rows()
        r2 = eng.query(abi.make_plan(table=t2, **plan_kw)).rows()
        # two separate runs: counts/keys exact; double sums are subject to
        # the ~1e-13 run-to-run atomicAdd-order wobble DESIGN documents
        # (an exact == here flaked once in a full-suite run)
        assert len(r1) == len(r2) == 3
        for (k1, v1), (k2, v2) in zip(r1, r2):
            assert k1 == k2 and v1[1] == v2[1]
            assert abs(v1[0] - v2[0]) <= 1e-12 * max(1.0, abs(v1[0]))
        m = i32 <= 2
        assert r1[0][1][1] + r1[1][1][1] + r1[2][1][1] == float(m.sum())
    finally:
        eng.close()
