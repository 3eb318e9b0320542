"""The query-compiled scan kernel SOURCE is pinned, on the CPU.

tests/jit_shapes.cpp includes csrc/jit.cpp, generates the kernel source for a
fixed table of plan shapes (every accumulator mode, join probe, slot scheme
and column kind) and prints one hash of the kernel text per shape.  The
committed hashes come from the generator as it was before it was split into
emitters, so a restructuring of jit.cpp that changes any emitted kernel text
fails here, with no GPU and no timing involved."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "jit_shapes.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "jit_source_hashes.txt")
PRELUDE_MARK = "---- prelude ----"


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def _default_env():
    # every shape runs in the default environment; the program itself sets
    # the one variable a shape names, in a child process
    return {k: v for k, v in os.environ.items() if not k.startswith("SN_JIT_")}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("jit_shapes") / "jit_shapes")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-o", exe, SRC, "-lhiprtc"],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def output(program):
    return subprocess.run([program], check=True, capture_output=True,
                          text=True, env=_default_env()).stdout


def _golden():
    with open(GOLDEN) as f:
        return [ln.strip() for ln in f
                if ln.strip() and not ln.startswith("#")]


def test_kernel_text_matches_committed_hashes(output):
    lines = output.split(PRELUDE_MARK)[0].splitlines()
    golden = _golden()
    assert [ln.split()[0] for ln in lines] == [g.split()[0] for g in golden]
    changed = [(ln, g) for ln, g in zip(lines, golden) if ln != g]
    assert not changed, f"kernel text changed for: {changed}"


def test_shape_table_reaches_every_mode(output):
    """The table is only a pin if it covers the generator: each accumulator
    mode and probe leaves its own mark in the hashed kernel text."""
    names = [ln.split()[0] for ln in _golden()]
    for prefix in ("keyless_", "regs_", "wbin_", "lds_", "global_",
                   "join_hash_", "join_spay_", "join_slut_", "sparse_i",
                   "sparse_packed", "sparse_radix"):
        assert any(n.startswith(prefix) for n in names), prefix
    hashes = {}
    for ln in output.split(PRELUDE_MARK)[0].splitlines():
        name, h = ln.split()
        hashes.setdefault(h, []).append(name)
    # the only two shapes with the same kernel text: a span already too big
    # for the nibble LUT does not care that SN_JIT_SLUT=0 switches it off
    dup = sorted(v for v in hashes.values() if len(v) > 1)
    assert dup == [["join_spay_bigspan", "join_spay_bigspan_slut0"]]


def test_prelude_pins_the_layout_mirror(output):
    """The prelude ends with static_asserts built from the host's own
    sizeof/offsetof, one per mirrored struct and member the kernel reads."""
    prelude = output.split(PRELUDE_MARK)[1]
    pins = [ln for ln in prelude.splitlines() if ln.startswith("static_assert(")]
    for what in ("sizeof(sn_dev_col)", "sizeof(sn_dev_batch)",
                 "sizeof(sn_dev_tile)", "sizeof(sn_dev_agg)",
                 "sizeof(sn_dev_plan)",
                 "__builtin_offsetof(sn_dev_plan, aggs)",
                 "__builtin_offsetof(sn_dev_plan, preds_d)",
                 "__builtin_offsetof(sn_dev_plan, inp[1].bm)",
                 "__builtin_offsetof(sn_dev_plan, radix)",
                 "__builtin_offsetof(sn_dev_batch, cols)",
                 "__builtin_offsetof(sn_dev_col, dictmap)"):
        assert any(what + " ==" in p for p in pins), what
    # nothing but the asserts follows the last helper definition
    tail = prelude[prelude.rindex("#define TILE"):].splitlines()[1:]
    assert tail and all(ln.startswith("static_assert(") for ln in tail)


def test_asserts_hold_under_hiprtc(program):
    """One shape through hipRTC for gfx950 (no GPU needed): the layout
    asserts are true for the device ABI and the kernel compiles."""
    subprocess.run([program, "--one", "keyless_all_kinds", "--compile"],
                   check=True, capture_output=True, env=_default_env())
