"""Query-compiled kernels over narrowed f64 columns, checked on the CPU.

tests/jit_shapes_narrow.cpp includes csrc/jit.cpp and generates the kernel
source for a keyless Q6 shape with kinds {F64C8, F64, F64C8, I32}, the same
with a delete mask, and Q1's register-accumulator shape with its two DICT16
keys.  Every shape compiles under hipRTC for gfx950 (no GPU needed), and the
value-dictionary lookup appears for exactly the narrowed columns: hoisted
once per tile, applied where the staged registers and the scalar tail form
the LDS image, and nowhere in the row phase."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "jit_shapes_narrow.cpp")

# shape -> (number of columns, narrowed column slots)
SHAPES = {
    "narrow_keyless_q6": (4, {0, 2}),
    "narrow_keyless_q6_del": (4, {0, 2}),
    "narrow_regs_q1": (7, {2, 4, 5}),
}


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("jit_shapes_narrow") / "jit_shapes_narrow")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-o", exe, SRC, "-lhiprtc"],
                   check=True)
    return exe


def _env():
    return {k: v for k, v in os.environ.items() if not k.startswith("SN_JIT_")}


def test_every_shape_compiles_for_gfx950(program):
    r = subprocess.run([program], capture_output=True, text=True, env=_env())
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [w for name in SHAPES for w in (name, "ok")]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_dictionary_lookup_for_exactly_the_narrowed_columns(program, shape):
    src = subprocess.run([program, "--dump", shape], check=True,
                         capture_output=True, text=True, env=_env()).stdout
    ncols, narrowed = SHAPES[shape]
    for c in range(ncols):
        hoists = len(re.findall(rf"const GAS double \*vd{c} = .*"
                                rf"b\.cols\[{c}\]\.rle_vals;", src))
        lookups = len(re.findall(rf"\bvd{c}\[", src))
        if c in narrowed:
            assert hoists == 1, (c, hoists)
            # four staged rows (two per register) and the scalar tail
            assert lookups == 5, (c, lookups)
            # 2 B per lane per staged load: rows 2*tid and 2*tid+1
            assert src.count(f"st{c}_0 = ((const GAS unsigned short *)"
                             f"(body{c} + (u64)(tile.row_start) * 1))[tid];") == 1
            assert f"unsigned short st{c}_0, st{c}_1;" in src
        else:
            assert hoists == 0 and lookups == 0, (c, hoists, lookups)
    # the image still holds the decoded double: the row phase is untouched
    row_phase = src[src.index("for (int k = 0; k < CHUNK / WG; k++)"):]
    assert "vd" not in row_phase.split("__syncthreads();")[0]
    assert ("del[(u64)gr >> 6]" in src) == shape.endswith("_del")
    # the extra descriptor member is pinned like the rest of the mirror
    assert "__builtin_offsetof(sn_dev_col, rle_vals) ==" in src
