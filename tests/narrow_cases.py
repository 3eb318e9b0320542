"""Inputs shared by the f64 narrowing tests (CPU reference and GPU kernels):
value pools whose first entries are the patterns a value-keyed dictionary
would get wrong, and the numpy statement of the contract."""
import numpy as np

SIZES = (1, 255, 256, 257, 4097)
DISTINCT = (1, 2, 255, 256, 257)      # 257 overflows
FILL = 0xA5                           # code buffers start as guard pattern

# -0.0 / +0.0, two NaN payloads, all ones (a NaN, and the largest pattern),
# +-inf, the smallest denormal
SPECIAL_BITS = np.array([
    0x8000000000000000, 0x0000000000000000,
    0x7FF8000000000001, 0x7FF8000000000002, 0xFFFFFFFFFFFFFFFF,
    0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001,
], dtype=np.uint64)


def pool(ndistinct, seed):
    """ndistinct distinct bit patterns: the special ones first (as many as
    fit), then random finite doubles."""
    rng = np.random.default_rng(seed)
    bits = list(SPECIAL_BITS[:ndistinct])
    seen = set(int(b) for b in bits)
    while len(bits) < ndistinct:
        b = int(np.float64(rng.normal() * 1e3).view(np.uint64))
        if b not in seen:
            seen.add(b)
            bits.append(np.uint64(b))
    return np.array(bits, dtype=np.uint64)


def column(n, ndistinct, seed):
    """n >= ndistinct doubles holding exactly ndistinct distinct patterns, in
    shuffled order."""
    k = ndistinct
    p = pool(k, seed)
    rng = np.random.default_rng(seed + 1)
    idx = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])
    rng.shuffle(idx)
    return p[idx].view(np.float64)


def cases():
    """every (n, distinct count) pair an n-row column can hold"""
    return [(n, d) for n in SIZES for d in DISTINCT if d <= n]


def expect(values, fill=FILL):
    """(codes, dict bits[256], ndict) by np.unique on the uint64 view."""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    uniq, inv = np.unique(bits, return_inverse=True)
    d = np.zeros(256, dtype=np.uint64)
    if uniq.size > 256:
        return np.full(bits.size, fill, dtype=np.uint8), d, -1
    d[:uniq.size] = uniq
    return inv.astype(np.uint8), d, int(uniq.size)
