"""Byte-exact checks of the put-time narrowing kernels (k_f64_distinct,
k_f64_dict, k_f64_encode), launched through sn_launch_f64_narrow on guarded
device buffers and compared with sn_f64_narrow_host: codes, the whole
256-entry dictionary and ndict are equal byte for byte, the guard bands stay
intact, and on overflow the code buffer keeps its fill pattern.  The cases
are those of the CPU test plus one 70,001-row column, so every phase runs
more than one workgroup (a workgroup step covers 1,024 rows), and one
1,100,001-row column: past 1,024 workgroups the grid stops growing, so only
there does a workgroup take a second grid-stride step."""
import ctypes as C

import numpy as np
import pytest

from snappydata_amd import engine as se
from tests import devmem as dm
from tests import narrow_cases as nc

pytestmark = pytest.mark.gpu

BIG = 70_001
STRIDED = 1_100_001        # > 1,024 workgroups x 1,024 rows


@pytest.fixture(scope="module")
def launch():
    return dm.launcher("sn_launch_f64_narrow",
                       [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p])


def narrow_on_device(launch, v, misalign=0):
    """(codes, dict bits, ndict) from the kernels; checks every guard band.
    `misalign` shifts the code array off its 4-byte alignment."""
    n = v.size
    body = codes = d = nd = None
    try:
        body = dm.guarded(n * 8)
        body.write(np.ascontiguousarray(v))
        codes = dm.guarded(n + misalign)
        d = dm.guarded(256 * 8)
        nd = dm.guarded(4)
        rc = launch(body.ptr, n, codes.ptr + misalign, d.ptr, nd.ptr, None)
        dm.sync()
        assert rc == 0
        for g in (body, codes, d, nd):
            g.check_bands()
        assert body.read() == np.ascontiguousarray(v).tobytes()
        raw = np.frombuffer(codes.read(), dtype=np.uint8)
        assert (raw[:misalign] == dm.FILL).all()
        return (raw[misalign:].copy(),
                np.frombuffer(d.read(), dtype=np.uint64).copy(),
                int(np.frombuffer(nd.read(), dtype=np.int32)[0]))
    finally:
        for g in (body, codes, d, nd):
            if g is not None:
                g.free()


def check(launch, v, misalign=0):
    codes, d, nd = narrow_on_device(launch, v, misalign)
    hcodes, hd, hnd = se.f64_narrow_host(v, fill=dm.FILL)
    assert nd == hnd
    assert d.tobytes() == hd.tobytes()
    assert codes.tobytes() == hcodes.tobytes()
    if nd < 0:
        assert (codes == dm.FILL).all()
    else:
        assert d[codes].tobytes() == v.view(np.uint64).tobytes()
    return nd


@pytest.mark.parametrize("n,ndistinct", nc.cases() + [
    (BIG, 50), (BIG, 256), (BIG, 257), (STRIDED, 50), (STRIDED, 257)])
def test_matches_host_reference(launch, n, ndistinct):
    v = nc.column(n, ndistinct, seed=1000 * ndistinct + n)
    nd = check(launch, v)
    assert nd == (ndistinct if ndistinct <= 256 else -1)


def test_special_patterns(launch):
    v = np.resize(nc.SPECIAL_BITS, 1000).view(np.float64)
    assert check(launch, v) == len(nc.SPECIAL_BITS)


def test_257th_pattern_in_the_last_row(launch):
    v = np.concatenate([nc.column(BIG - 1, 256, seed=7),
                        np.array([123456.789])])
    assert check(launch, v) == -1


def test_unaligned_code_array(launch):
    v = nc.column(4097, 50, seed=11)
    assert check(launch, v, misalign=1) == 50
