"""Bit-exact checks of put-time patch materialisation (k_patch_apply),
launched directly through sn_launch_patch_apply on a 1000-element body.

Patch values always arrive as doubles.  F64 bodies take the bits unchanged,
F32 bodies narrow round-to-nearest-even, I32/I16 bodies round to nearest
(ties to even), and INT64 bodies take the double's raw bit pattern.  numpy
supplies the reference for every kind."""
import ctypes as C

import numpy as np
import pytest

from tests import devmem as dm

pytestmark = pytest.mark.gpu

K_F64, K_I32, K_I64, K_F32, K_I16 = 0, 1, 2, 3, 6
BODY_DTYPE = {K_F64: np.uint64, K_F32: np.uint32, K_I64: np.int64,
              K_I32: np.int32, K_I16: np.int16}   # float bodies as raw bits
KIND_IDS = {K_F64: "f64", K_F32: "f32", K_I64: "i64", K_I32: "i32",
            K_I16: "i16"}
BODY_N = 1000
SIZES = [1, 255, 256, 257]


@pytest.fixture(scope="module")
def launch():
    return dm.launcher("sn_launch_patch_apply",
                       [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                        C.c_void_p])


def body_pattern(kind):
    """The known fill of the body before patching."""
    dt = BODY_DTYPE[kind]
    return ((np.arange(BODY_N, dtype=np.int64) * 37 + 11) % 251 + 1000).astype(dt)


def positions(n, rng):
    """n unique positions; 0 and 999 are always among them (n permitting)."""
    must = [0, BODY_N - 1][:n] if n > 1 else [BODY_N - 1]
    rest = rng.permutation(np.arange(1, BODY_N - 1))[:n - len(must)]
    pos = np.concatenate([np.array(must, dtype=np.int64), rest])
    pos = rng.permutation(pos).astype(np.int32)
    assert len(np.unique(pos)) == n
    return pos


def f64_bits(x):
    return np.array(x, dtype=np.uint64).view(np.float64)


def patch_values(kind, n, rng):
    """(doubles handed to the kernel, expected body elements)."""
    if kind == K_F64:
        special = np.concatenate([
            f64_bits([0x7FF8000000ABCDEF, 0xFFF0000000000001]),   # NaN payloads
            np.array([-0.0, 0.0, np.inf, -np.inf, 5e-324, 1.7976931348623157e308,
                      0.1, -1e-300])])
        v = np.resize(np.concatenate([special, rng.standard_normal(64) * 1e6]), n)
        return v, v.view(np.uint64).copy()
    if kind == K_F32:
        one = 1.0
        special = np.array([
            one + 2.0 ** -24,               # tie -> even: rounds down to 1
            one + 2.0 ** -24 + 2.0 ** -40,  # above the tie: rounds up
            one + 3 * 2.0 ** -24,           # tie -> even: rounds up
            one + 2.0 ** -25,               # below the tie: rounds down
            -(one + 2.0 ** -24 + 2.0 ** -40),
            1e39, -1e39,                    # overflow to +-inf
            3.4028235677973366e38,          # FLT_MAX + half an ulp: tie -> inf
            3.40282356e38,                  # just below that tie: FLT_MAX
            1e-46, 1e-45, -0.0, 0.1, 16777217.0])
        v = np.resize(np.concatenate([special, rng.standard_normal(64) * 1e3]), n)
        with np.errstate(over="ignore"):
            exp = v.astype(np.float32)
        return v, exp.view(np.uint32).copy()
    if kind in (K_I32, K_I16):
        dt = BODY_DTYPE[kind]
        ii = np.iinfo(dt)
        special = np.array([1.5, -1.5, 0.5, -0.5, 2.5, -2.5, 3.5, 0.49999999999999994,
                            float(ii.max), float(ii.min), float(ii.max) - 0.5,
                            float(ii.min) + 0.5, 7.0, -7.0, 0.0, -0.0, 1e-9])
        rnd = np.round(rng.uniform(-1000, 1000, 64), 1)
        v = np.resize(np.concatenate([special, rnd]), n)
        exp = np.rint(v).astype(np.int64)
        assert exp.min() >= ii.min and exp.max() <= ii.max
        return v, exp.astype(dt)
    assert kind == K_I64
    special = np.array([-(1 << 53) - 1, (1 << 53) + 1, (1 << 62) + 12345,
                        -(1 << 63), (1 << 63) - 1, -1, 0, 1,
                        -0x0123456789ABCDEF], dtype=np.int64)
    ints = np.resize(np.concatenate(
        [special, rng.integers(-(1 << 63), (1 << 63) - 1, 64, dtype=np.int64)]), n)
    assert (ints < -(1 << 53)).any()     # beyond 2^53 with the top bit set
    return ints.view(np.float64).copy(), ints.copy()


def apply(launch, kind, pos, val):
    """Patch a fresh pattern body on the device; returns the body after."""
    dt = BODY_DTYPE[kind]
    n = len(pos)
    body = dpos = dval = None
    try:
        body = dm.guarded(BODY_N * np.dtype(dt).itemsize)
        body.write(body_pattern(kind))
        dpos = dm.upload(np.ascontiguousarray(pos, dtype=np.int32))
        dval = dm.upload(np.ascontiguousarray(val, dtype=np.float64))
        rc = launch(body.ptr, dpos, dval, n, kind, None)
        dm.sync()
        assert rc == 0
        out = np.frombuffer(body.read(), dtype=dt).copy()
        body.check_bands()
        return out
    finally:
        if body is not None:
            body.free()
        dm.free(dval)
        dm.free(dpos)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", [K_F64, K_F32, K_I64, K_I32, K_I16],
                         ids=lambda k: KIND_IDS[k])
def test_patch_apply(launch, kind, n):
    rng = np.random.default_rng(900 + 17 * kind + n)
    pos = positions(n, rng)
    val, exp = patch_values(kind, n, rng)
    assert len(val) == len(exp) == n
    if n > 1:
        assert 0 in pos and BODY_N - 1 in pos
    out = apply(launch, kind, pos, val)
    want = body_pattern(kind)
    want[pos] = exp
    bad = np.nonzero(out != want)[0]
    for i in bad[:8]:
        k = np.nonzero(pos == i)[0]
        print("element", i, "got", out[i], "want", want[i],
              "patch value", val[k[0]].hex() if len(k) else "(unpatched)")
    assert out.tobytes() == want.tobytes()


@pytest.mark.parametrize("kind", [K_F64, K_F32, K_I64, K_I32, K_I16],
                         ids=lambda k: KIND_IDS[k])
def test_patch_apply_n0_is_noop(launch, kind):
    out = apply(launch, kind, np.zeros(0, dtype=np.int32),
                np.zeros(0, dtype=np.float64))
    assert out.tobytes() == body_pattern(kind).tobytes()
