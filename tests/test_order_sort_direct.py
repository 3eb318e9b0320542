"""k_order_sort, launched directly through sn_launch_order_sort on guarded
device buffers: entries (key u64, class << 62 | scan position) in, the same
entries sorted by (class, key, scan position) out, byte for byte against
np.lexsort.  Keys are drawn from three values (0 and 2^64 - 1 among them), so
the scan position decides most comparisons; the sizes straddle a wave, the
1,024-lane workgroup and the powers of two the bitonic network pads to."""
import ctypes as C

import numpy as np
import pytest

from tests import devmem as dm

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 1000, 8191, 8192]
KEYS = np.array([0, 0x8000000000000000, 2 ** 64 - 1], dtype=np.uint64)


@pytest.fixture(scope="module")
def launch():
    return dm.launcher("sn_launch_order_sort",
                       [C.c_void_p, C.c_int32, C.c_void_p])


def entries_for(n):
    rng = np.random.default_rng(1000 + n)
    key = KEYS[rng.integers(0, 3, n)]
    if n >= 2:
        key[0], key[-1] = KEYS[2], KEYS[0]
    cls = rng.integers(0, 3, n).astype(np.uint64)
    batch = rng.integers(0, 5, n).astype(np.uint64)
    row = rng.permutation(1 << 20)[:n].astype(np.uint64)    # distinct positions
    cp = (cls << np.uint64(62)) | (batch << np.uint64(32)) | row
    ents = np.empty((n, 2), dtype=np.uint64)
    ents[:, 0], ents[:, 1] = key, cp
    return ents, cls


@pytest.mark.parametrize("n", SIZES)
def test_sort_matches_lexsort(launch, n):
    ents, cls = entries_for(n)
    order = np.lexsort((ents[:, 1], ents[:, 0], cls))
    exp = np.ascontiguousarray(ents[order])
    if n >= 64:
        assert not (order == np.arange(n)).all()
        assert (ents[:, 0] == 0).any() and (ents[:, 0] == KEYS[2]).any()
    buf = dm.guarded(16 * n)
    try:
        buf.write(np.ascontiguousarray(ents))
        assert launch(buf.ptr, n, None) == 0
        dm.sync()
        assert buf.read() == exp.tobytes()
        buf.check_bands()
    finally:
        buf.free()


def test_bad_sizes_are_refused(launch):
    assert launch(None, -1, None) != 0
    assert launch(None, 8193, None) != 0
    assert launch(None, 0, None) == 0
