"""sn_f64_narrow_host — the plain-C++ statement of the put-time narrowing
contract — against numpy: values are told apart by their 64-bit pattern, the
dictionary is sorted as unsigned integers and zero-padded, dict[codes] gives
back the input bits, and more than 256 patterns leave ndict == -1 with the
code buffer untouched.  The reference is np.unique on the uint64 view."""
import numpy as np
import pytest

from snappydata_amd import engine as se
from tests import narrow_cases as nc


def run(values):
    codes, d, nd = se.f64_narrow_host(values, fill=nc.FILL)
    return codes, d.view(np.uint64), nd


@pytest.mark.parametrize("n,ndistinct", nc.cases())
def test_matches_numpy_unique(n, ndistinct):
    v = nc.column(n, ndistinct, seed=1000 * ndistinct + n)
    assert len(np.unique(v.view(np.uint64))) == ndistinct
    codes, d, nd = run(v)
    wcodes, wd, wnd = nc.expect(v)
    assert nd == wnd
    assert nd == (ndistinct if ndistinct <= 256 else -1)
    assert d.tobytes() == wd.tobytes()
    assert codes.tobytes() == wcodes.tobytes()
    if nd > 0:
        assert (np.diff(d[:nd].astype(object)) > 0).all()   # unsigned order
        assert d[codes].tobytes() == v.view(np.uint64).tobytes()


def test_zero_signs_nan_payloads_inf_and_denormal_keep_their_bits():
    v = np.resize(nc.SPECIAL_BITS, 64).view(np.float64)
    codes, d, nd = run(v)
    assert nd == len(nc.SPECIAL_BITS)
    by_bits = {int(b): int(c) for b, c in zip(v.view(np.uint64), codes)}
    assert by_bits[0x8000000000000000] != by_bits[0x0000000000000000]
    assert by_bits[0x7FF8000000000001] != by_bits[0x7FF8000000000002]
    assert len(set(by_bits.values())) == len(nc.SPECIAL_BITS)
    # all ones is the largest pattern, +0.0 the smallest
    assert by_bits[0xFFFFFFFFFFFFFFFF] == nd - 1
    assert by_bits[0] == 0
    assert d[codes].tobytes() == v.tobytes()


def test_overflow_is_decided_by_the_whole_column():
    # 256 patterns in the first 4096 rows, the 257th in the last row
    v = np.concatenate([nc.column(4096, 256, seed=7),
                        np.array([123456.789])])
    assert 123456.789 not in v[:-1]
    codes, d, nd = run(v)
    assert nd == -1
    assert not d.any()
    assert (codes == nc.FILL).all()


def test_empty_column():
    codes, d, nd = run(np.zeros(0))
    assert nd == 0 and not d.any() and codes.size == 0
