"""Byte-exact checks of the device LZ4 block decoder (k_lz4_decompress),
launched directly through sn_launch_lz4_decompress on small buffers.

Expected bytes never come from the engine: for liblz4-compressed inputs they
are the original buffer, for hand-built blocks the output of liblz4's
LZ4_decompress_safe.  Only valid streams are sent to the GPU (the engine
validates every blob on the host before it launches the device decode)."""
import ctypes as C

import numpy as np
import pytest

from tests import devmem as dm


def _load_lz4():
    for name in ("liblz4.so.1", "liblz4.so"):
        try:
            lib = C.CDLL(name)
        except OSError:
            continue
        lib.LZ4_compressBound.restype = C.c_int
        lib.LZ4_compressBound.argtypes = [C.c_int]
        lib.LZ4_compress_default.restype = C.c_int
        lib.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int,
                                             C.c_int]
        lib.LZ4_compress_fast.restype = C.c_int
        lib.LZ4_compress_fast.argtypes = [C.c_char_p, C.c_char_p, C.c_int,
                                          C.c_int, C.c_int]
        lib.LZ4_decompress_safe.restype = C.c_int
        lib.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int,
                                            C.c_int]
        return lib
    return None


LZ4 = _load_lz4()
if LZ4 is None:
    pytest.skip("liblz4 not available", allow_module_level=True)



def lz4_compress(data, accel=None):
    bound = LZ4.LZ4_compressBound(len(data))
    out = C.create_string_buffer(bound)
    if accel is None:
        n = LZ4.LZ4_compress_default(data, out, len(data), bound)
    else:
        n = LZ4.LZ4_compress_fast(data, out, len(data), bound, accel)
    assert n > 0
    return out.raw[:n]


def lz4_reference(block, dlen):
    out = C.create_string_buffer(max(dlen, 1))
    n = LZ4.LZ4_decompress_safe(block, out, len(block), dlen)
    assert n == dlen, f"liblz4 rejects the block ({n})"
    return out.raw[:dlen]


# ------------------------------------------------------------ block builder

def _ext(x):
    """Length-extension bytes of a nibble that saturated at 15."""
    if x < 15:
        return b""
    x -= 15
    return b"\xff" * (x // 255) + bytes([x % 255])


def seq(literals, offset=None, match_len=None):
    """One LZ4 sequence: token, literal-length extension, literals, then
    (unless literals-only) little-endian offset and match-length extension."""
    ll = len(literals)
    if offset is None:
        return bytes([min(ll, 15) << 4]) + _ext(ll) + literals
    assert 1 <= offset <= 65535 and match_len >= 4
    ml = match_len - 4
    return (bytes([(min(ll, 15) << 4) | min(ml, 15)]) + _ext(ll) + literals +
            offset.to_bytes(2, "little") + _ext(ml))


TAIL = b"TAILTAIL"


def walk(block):
    """Token walk: [(literal_len, offset or None, match_len or None), ...]."""
    out = []
    ip, n = 0, len(block)
    while ip < n:
        tok = block[ip]; ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = block[ip]; ip += 1
                ll += b
                if b != 255:
                    break
        ip += ll
        if ip >= n:
            assert ip == n
            out.append((ll, None, None))
            break
        off = block[ip] | (block[ip + 1] << 8); ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = block[ip]; ip += 1
                ml += b
                if b != 255:
                    break
        out.append((ll, off, ml + 4))
    return out


def rand(n, seed=None):
    seed = 1000 + n if seed is None else seed
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _handbuilt():
    cases = [
        ("off1_len4", [seq(b"a", 1, 4)]),
        ("off1_len19_ext0", [seq(b"a", 1, 19)]),
        ("off1_len274_ext255_0", [seq(b"a", 1, 274)]),
        ("off3_len200", [seq(b"abc", 3, 200)]),
        ("off7_len65", [seq(b"abcdefg", 7, 65)]),
        ("off63_len300", [seq(rand(63), 63, 300)]),
        ("off64_len300", [seq(rand(64), 64, 300)]),
        ("off65_len300", [seq(rand(65), 65, 300)]),
        ("lit15_ext0", [seq(rand(15), 15, 4)]),
        ("lit270_ext255_0", [seq(rand(270), 270, 4)]),
        ("off65535_len70000", [seq(rand(65535), 65535, 70000)]),
        ("zero_literal_seq", [seq(b"abcdefgh", 8, 8), seq(b"", 4, 20)]),
        ("literals_only_1000", [seq(rand(1000))]),
        ("one_byte", [seq(b"x")]),
    ]
    out = []
    for name, seqs in cases:
        block = b"".join(seqs)
        if walk(block)[-1][1] is not None:      # ends in a match: add the tail
            block += seq(TAIL)
        dlen = sum(ll + (ml or 0) for ll, _, ml in walk(block))
        out.append(pytest.param(block, dlen, id=name))
    return out


# ---------------------------------------------------------------- the sweep

LENGTHS = [1, 12, 13, 64, 65, 4095, 4096, 4097, 65536]
PERIODS = [1, 2, 3, 5, 8, 63, 64, 65, 1000]


def sweep_buffers():
    rng = np.random.default_rng(20240611)

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    bufs = []
    for p in PERIODS:                                 # periodic data
        unit = rb(p)
        for n in (65, 4097, 65536):
            bufs.append((unit * (n // p + 1))[:n])
    for n in LENGTHS:                                 # constant runs
        bufs.append(bytes([int(rng.integers(0, 256))]) * n)
    for n in (4095, 4096, 65536):                     # several long runs
        b = b""
        while len(b) < n:
            b += bytes([int(rng.integers(0, 256))]) * int(rng.integers(300, 5000))
        bufs.append(b[:n])
    for n in LENGTHS:                                 # incompressible
        bufs.append(rb(n))
    for n in (4095, 4096, 4097, 20000, 65536, 65536):  # chunks + earlier copies
        b = b""
        chunks = []
        while len(b) < n:
            if chunks and rng.random() < 0.5:
                c = chunks[int(rng.integers(0, len(chunks)))]
                k = int(rng.integers(4, len(c) + 1))
                s = int(rng.integers(0, len(c) - k + 1))
                b += c[s:s + k]
            else:
                c = rb(int(rng.integers(5, 700)))
                chunks.append(c)
                b += c
        bufs.append(b[:n])
    assert len(bufs) >= 40 and max(map(len, bufs)) <= 65536
    assert {len(b) for b in bufs} >= set(LENGTHS)
    return bufs


@pytest.fixture(scope="module")
def sweep():
    return sweep_buffers()


# ------------------------------------------------------------ device decode

@pytest.fixture(scope="module")
def launch():
    return dm.launcher("sn_launch_lz4_decompress",
                       [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                        C.c_void_p, C.c_void_p])


def device_decode(launch, block, dlen):
    """Decode one block on the device into a guarded buffer; returns the
    dlen output bytes after asserting launch status, error word and bands."""
    src = err = dst = None
    try:
        src = dm.upload(block)
        err = dm.malloc(4)
        dm.memset(err, 0, 4)
        dst = dm.guarded(dlen)
        rc = launch(src, len(block), dst.ptr, dlen, err, None)
        dm.sync()
        assert rc == 0
        assert int.from_bytes(dm.from_device(err, 4), "little") == 0
        out = dst.read()
        dst.check_bands()
        return out
    finally:
        if dst is not None:
            dst.free()
        dm.free(err)
        dm.free(src)


def assert_same_bytes(got, expected, what):
    if got != expected:                 # keep the report short on big buffers
        n = min(len(got), len(expected))
        i = next((k for k in range(n) if got[k] != expected[k]), n)
        pytest.fail(f"{what}: first difference at byte {i} of {len(expected)}: "
                    f"got {got[i:i + 16].hex()} expected "
                    f"{expected[i:i + 16].hex()}")


@pytest.mark.parametrize("block,dlen", _handbuilt())
def test_handbuilt_block_is_valid_lz4(block, dlen):
    """liblz4 accepts every hand-built block and yields dlen bytes (CPU)."""
    assert len(lz4_reference(block, dlen)) == dlen


@pytest.mark.gpu
@pytest.mark.parametrize("block,dlen", _handbuilt())
def test_handbuilt_block(launch, block, dlen):
    expected = lz4_reference(block, dlen)
    assert_same_bytes(device_decode(launch, block, dlen), expected, "block")


def test_sweep_covers_the_claimed_paths(sweep):
    """The liblz4-compressed sweep must really contain the shapes it is
    there for (tokens only; no GPU work)."""
    small_off = overlap = long_lit = long_match = False
    for buf in sweep:
        for ll, off, ml in walk(lz4_compress(buf)):
            long_lit |= ll >= 270
            if off is not None:
                small_off |= off < 8
                overlap |= off < ml
                long_match |= ml >= 274
    assert small_off, "no match with offset < 8"
    assert overlap, "no match with offset < match length"
    assert long_lit, "no literal run >= 270"
    assert long_match, "no match >= 274"


@pytest.mark.gpu
@pytest.mark.parametrize("accel", [None, 8], ids=["default", "fast8"])
def test_sweep_roundtrip(launch, sweep, accel):
    for i, buf in enumerate(sweep):
        block = lz4_compress(buf, accel)
        assert lz4_reference(block, len(buf)) == buf
        assert_same_bytes(device_decode(launch, block, len(buf)), buf,
                          f"buffer {i} (len {len(buf)}, accel {accel})")
