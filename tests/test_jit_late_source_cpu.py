"""Query-compiled kernels with a late column, checked on the CPU.

tests/jit_shapes_late.cpp includes csrc/jit.cpp and generates the kernel
source for keyless Q6 with kinds {F64C8, F64_LATE, F64C8, I32}, the same with
a delete mask, the same over plain f64 predicate columns, SUM(a*b) over two
late columns, and a keyless MIN/MAX over a late column.  Every shape compiles
under hipRTC for gfx950 (no GPU needed).  A late column has no staged
register and no row of the LDS image; it is read nowhere but in the row
phase, under the row's `ok`; and the staged columns are loaded and converted
by the very lines of the corresponding shape without a late column."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# shape -> (columns, late column slots, rows per chunk)
SHAPES = {
    "late_keyless_q6": (4, {1}, 1024),
    "late_keyless_q6_del": (4, {1}, 1024),
    "late_keyless_q6_f64": (4, {1}, 1024),
    "late_keyless_two": (3, {1, 2}, 1024),
    "late_single_minmax": (3, {1}, 1024),
}
# the shape of jit_shapes_narrow.cpp with the same columns, all staged
NARROW_TWIN = {"late_keyless_q6": "narrow_keyless_q6",
               "late_keyless_q6_del": "narrow_keyless_q6_del"}


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def _build(tmp_path_factory, name):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run([hipcc, "-O1", "-std=c++17", "-o", exe,
                    os.path.join(REPO, "tests", name + ".cpp"), "-lhiprtc"],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "jit_shapes_late")


@pytest.fixture(scope="module")
def narrow_program(tmp_path_factory):
    return _build(tmp_path_factory, "jit_shapes_narrow")


def _env():
    return {k: v for k, v in os.environ.items() if not k.startswith("SN_JIT_")}


def _dump(exe, shape, **env):
    return subprocess.run([exe, "--dump", shape], check=True,
                          capture_output=True, text=True,
                          env=dict(_env(), **env)).stdout


def test_every_shape_compiles_for_gfx950(program):
    r = subprocess.run([program], capture_output=True, text=True, env=_env())
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [w for name in SHAPES for w in (name, "ok")]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_late_columns_are_read_in_the_row_phase_only(program, shape):
    src = _dump(program, shape)
    ncols, late, chunk = SHAPES[shape]
    assert f"#define CHUNK {chunk}\n" in src
    # the image has one row per staged column
    assert f"double sval[{ncols - len(late)}][CHUNK];" in src
    loop = src.index("for (int base = tile.row_start;")
    barrier = src.index("__syncthreads();", loop)
    row_phase = src.index("for (int k = 0; k < CHUNK / WG; k++)", barrier)
    for c in range(ncols):
        reads = [m.start() for m in re.finditer(rf"\(body{c}\b", src)]
        if c not in late:
            assert f" st{c}_0" in src
            assert reads and min(reads) < loop       # prologue stage_load
            continue
        assert not re.search(rf"\bst{c}_\d", src)
        # one read, in the row phase, the whole statement under `ok`, GAS
        assert len(reads) == 1 and reads[0] > row_phase, (c, reads)
        line = src[src.rindex("\n", 0, reads[0]) + 1:src.index("\n", reads[0])]
        assert line.strip() == (f"if (ok) e{c}[k] = ((const GAS double *)"
                                f"(body{c}))[base + r];"), line
        assert f"e{c}[k] = 0.0;" in src
        assert f"double e{c}[CHUNK / WG];" in src
    # the staged columns' image rows are dense: 0 .. nstaged-1
    rows = {int(m) for m in re.findall(r"sval\[(\d+)\](?!\[CHUNK\])", src)}
    assert rows == set(range(ncols - len(late)))
    # `ok` holds r < rows before any late read, and the select stays
    pass_a = src[row_phase:src.index("#pragma unroll", row_phase)]
    assert "int ok = r < rows;" in pass_a and "okv[k] = ok;" in pass_a
    assert ("del[(u64)gr >> 6]" in pass_a) == shape.endswith("_del")
    if shape.startswith("late_keyless"):
        assert "sums[0] += ok ? va0 : 0.0;" in src
    # the value-dictionary pin is still emitted for shapes with 1-byte codes
    assert ("__builtin_offsetof(sn_dev_col, rle_vals) ==" in src) == \
        (shape != "late_keyless_q6_f64" and shape != "late_keyless_two")


@pytest.mark.parametrize("lds_dict", [False, True])
@pytest.mark.parametrize("shape", sorted(NARROW_TWIN))
def test_staged_columns_keep_the_narrow_shape_lines(program, narrow_program,
                                                    shape, lds_dict):
    """with SN_JIT_LATE_LDSDICT=0 the lines are the twin's own; by default
    they differ in one thing, the dictionary they index: svd<c>, the LDS copy
    made once per tile, where the twin indexes vd<c> in global memory"""
    if lds_dict:
        text = _dump(program, shape)
        for c in (0, 2):
            assert f"double svd{c}[WG];" in text
            copy = text.index(f"    svd{c}[tid] = vd{c}[tid];\n")
            assert copy < text.index("__syncthreads();", copy) < \
                text.index("for (int base = tile.row_start;")
            # the only other use of the global dictionary is the scalar tail
            assert len(re.findall(rf"[^s]vd{c}\[", text)) == 2
        src = re.sub(r"\bsvd(\d)\[st", r"vd\1[st", text).splitlines()
    else:
        text = _dump(program, shape, SN_JIT_LATE_LDSDICT="0")
        assert "svd" not in text
        src = text.splitlines()
    twin = _dump(narrow_program, NARROW_TWIN[shape]).splitlines()
    _, late, _ = SHAPES[shape]
    # stage loads (prologue and next-chunk) and register -> double converts
    want = [ln for ln in twin
            if re.match(r"\s*st\d_\d = \(\(const GAS ", ln) or
            re.match(r"\s*(\{ )?double2_t y\d; y\d\.x = ", ln)]
    want = [ln for ln in want
            if not any(f"st{c}_" in ln or f"body{c} " in ln for c in late)]
    assert len(want) == 2 * 2 * 3 + 2 * 3
    got = [ln for ln in src
           if re.match(r"\s*st\d_\d = \(\(const GAS ", ln) or
           re.match(r"\s*(\{ )?double2_t y\d; y\d\.x = ", ln)]
    assert got == want
    # and the scalar tail's conversions, up to the image row they fill
    tail = [re.sub(r"sval\[\d\]", "sval[]", ln) for ln in twin
            if "for (int r = tid; r < rows; r += WG)" in ln and
            not any(f"(body{c})" in ln for c in late)]
    got = [re.sub(r"sval\[\d\]", "sval[]", ln) for ln in src
           if "for (int r = tid; r < rows; r += WG)" in ln]
    assert tail == got and len(got) == 3
