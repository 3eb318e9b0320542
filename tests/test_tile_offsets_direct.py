"""k_tile_offsets, launched directly through sn_launch_tile_offsets on guarded
device buffers: int32 tile counts in, int64 exclusive offsets and the total
out, byte for byte against np.cumsum.  The sizes straddle the 256 counts one
step of the single workgroup takes, so the carry between steps is exercised;
counts include 0 and 16384 (an empty and a full tile)."""
import ctypes as C

import numpy as np
import pytest

from tests import devmem as dm

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1000]


@pytest.fixture(scope="module")
def launch():
    return dm.launcher("sn_launch_tile_offsets",
                       [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                        C.c_void_p])


def counts_for(n):
    rng = np.random.default_rng(n)
    c = rng.integers(0, 16385, n).astype(np.int32)
    c[rng.integers(0, n, max(1, n // 5))] = 0
    c[rng.integers(0, n, max(1, n // 5))] = 16384
    c[0] = 16384 if n > 1 else 0
    c[-1] = 0 if n > 1 else 16384
    return c


@pytest.mark.parametrize("n", SIZES)
def test_offsets_match_cumsum(launch, n):
    counts = counts_for(n)
    assert (counts == 0).any() or n == 1
    assert (counts == 16384).any()
    inc = np.cumsum(counts.astype(np.int64))
    exp_off = (inc - counts).astype(np.int64)
    exp_total = np.array([inc[-1]], dtype=np.int64)
    src = dm.upload(counts)
    off, tot = dm.guarded(8 * n), dm.guarded(8)
    try:
        assert launch(src, n, off.ptr, tot.ptr, None) == 0
        dm.sync()
        assert off.read() == exp_off.tobytes()
        assert tot.read() == exp_total.tobytes()
        off.check_bands()
        tot.check_bands()
    finally:
        dm.free(src)
        off.free()
        tot.free()


def test_totals_beyond_int32(launch):
    """1000 counts of 2^31 - 1: offsets and carry are 64-bit."""
    n = 1000
    counts = np.full(n, 2 ** 31 - 1, dtype=np.int32)
    inc = np.cumsum(counts.astype(np.int64))
    src = dm.upload(counts)
    off, tot = dm.guarded(8 * n), dm.guarded(8)
    try:
        assert launch(src, n, off.ptr, tot.ptr, None) == 0
        dm.sync()
        assert off.read() == (inc - counts).astype(np.int64).tobytes()
        assert tot.read() == inc[-1:].tobytes()
        assert inc[-1] > 2 ** 40
        off.check_bands()
        tot.check_bands()
    finally:
        dm.free(src)
        off.free()
        tot.free()
