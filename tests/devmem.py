"""Thin ctypes layer over libamdhip64.so for tests that launch the engine's
`sn_launch_*` kernels directly on small device buffers and compare the
output byte for byte with a CPU reference.

Every HIP return code is asserted to be 0.  `guarded()` buffers carry a
0xA5-filled band on both sides so an out-of-bounds write by the kernel under
test shows up in `Guarded.check_bands()`.

Usage rules: kernel launches go through `launcher(name, argtypes)` on the
null stream (`None`), are followed by `sync()` before any readback, and every
buffer is freed in a `finally` block.
"""
import ctypes as C

from snappydata_amd import engine as se

H2D, D2H = 1, 2
BAND = 65536
FILL = 0xA5

_hip = None


def hip():
    global _hip
    if _hip is None:
        h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipFree.argtypes = [C.c_void_p]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        for f in (h.hipMalloc, h.hipFree, h.hipMemcpy, h.hipMemset,
                  h.hipDeviceSynchronize):
            f.restype = C.c_int
        _hip = h
    return _hip


def malloc(nbytes):
    """Device pointer (int) of a fresh allocation of max(nbytes, 1) bytes."""
    p = C.c_void_p()
    rc = hip().hipMalloc(C.byref(p), max(int(nbytes), 1))
    assert rc == 0, f"hipMalloc({nbytes}) -> {rc}"
    assert p.value
    return p.value


def free(ptr):
    if ptr:
        rc = hip().hipFree(C.c_void_p(ptr))
        assert rc == 0, f"hipFree -> {rc}"


def memset(ptr, byte, nbytes):
    if nbytes:
        rc = hip().hipMemset(C.c_void_p(ptr), byte, nbytes)
        assert rc == 0, f"hipMemset -> {rc}"


def sync():
    rc = hip().hipDeviceSynchronize()
    assert rc == 0, f"hipDeviceSynchronize -> {rc}"


def to_device(ptr, data):
    """Copy a bytes-like object (bytes, bytearray, contiguous ndarray) to ptr."""
    mv = memoryview(data).cast("B")
    if mv.nbytes == 0:
        return
    if mv.readonly:
        src = (C.c_char * mv.nbytes).from_buffer_copy(mv)
    else:
        src = (C.c_char * mv.nbytes).from_buffer(mv)
    rc = hip().hipMemcpy(C.c_void_p(ptr), src, mv.nbytes, H2D)
    assert rc == 0, f"hipMemcpy H2D -> {rc}"


def from_device(ptr, nbytes):
    """nbytes of device memory at ptr, as bytes."""
    if nbytes == 0:
        return b""
    buf = C.create_string_buffer(nbytes)
    rc = hip().hipMemcpy(buf, C.c_void_p(ptr), nbytes, D2H)
    assert rc == 0, f"hipMemcpy D2H -> {rc}"
    return buf.raw


def upload(data):
    """malloc + to_device; the caller frees."""
    mv = memoryview(data).cast("B")
    p = malloc(mv.nbytes)
    try:
        to_device(p, mv)
    except BaseException:
        free(p)
        raise
    return p


class Guarded:
    """band + nbytes + band bytes, all 0xA5; `ptr` is the inner pointer."""

    def __init__(self, nbytes, band=BAND):
        self.nbytes, self.band = int(nbytes), int(band)
        self.base = malloc(self.nbytes + 2 * self.band)
        try:
            memset(self.base, FILL, self.nbytes + 2 * self.band)
        except BaseException:
            free(self.base)
            raise
        self.ptr = self.base + self.band

    def write(self, data):
        assert memoryview(data).cast("B").nbytes <= self.nbytes
        to_device(self.ptr, data)

    def read(self):
        return from_device(self.ptr, self.nbytes)

    def check_bands(self):
        whole = from_device(self.base, self.nbytes + 2 * self.band)
        clean = bytes([FILL]) * self.band
        assert whole[:self.band] == clean, "leading guard band overwritten"
        assert whole[self.band + self.nbytes:] == clean, \
            "trailing guard band overwritten"

    def free(self):
        free(self.base)
        self.base = 0


def guarded(nbytes, band=BAND):
    return Guarded(nbytes, band)


def launcher(name, argtypes):
    """The engine library's exported `name`, with its prototype declared."""
    fn = getattr(se.lib(), name)
    fn.argtypes = argtypes
    fn.restype = C.c_int
    return fn
