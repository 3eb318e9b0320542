"""The image-free ("direct") keyless kernel's source, checked on the CPU.

tests/jit_shapes_direct.cpp includes csrc/jit.cpp and generates the kernel
source for plans whose late columns carry SN_K_F64_LATE_DIRECT: keyless Q6
with kinds {F64C8, LATE_DIRECT, F64C8, I32}, the same with a delete mask, an
int16 key, SUM(a*b) over two late columns, and a narrowed column that only an
aggregate factor reads.  Every shape compiles under hipRTC for gfx950 (no GPU
needed).  The kernel keeps no LDS image and no barrier in its row loop, reads
each late column once, under the row's `ok`, and accumulates with the lines
of every keyless kernel.

The same plans with SN_K_F64_LATE in place of the new tag must generate what
they generated before the tag existed: tests/fixtures/jit_late_twin_source.txt
holds those texts, made from the generator as it was then."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# shape -> (columns, late slots, narrowed predicate slots, narrowed factor slots)
SHAPES = {
    "direct_keyless_q6": (4, {1}, {0, 2}, {2}),
    "direct_keyless_q6_del": (4, {1}, {0, 2}, {2}),
    "direct_keyless_i16": (3, {1}, {2}, set()),
    "direct_keyless_two": (3, {1, 2}, set(), set()),
    "direct_keyless_factor": (3, {1}, set(), {2}),
}


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("jit_shapes_direct") / "jit_shapes_direct")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-o", exe,
                    os.path.join(REPO, "tests", "jit_shapes_direct.cpp"),
                    "-lhiprtc"], check=True)
    return exe


def _env():
    return {k: v for k, v in os.environ.items()
            if not k.startswith(("SN_JIT_", "SN_DIRECT"))}


def _dump(exe, shape, how="--dump"):
    return subprocess.run([exe, how, shape], check=True, capture_output=True,
                          text=True, env=_env()).stdout


def test_every_shape_compiles_for_gfx950(program):
    r = subprocess.run([program], capture_output=True, text=True, env=_env())
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [w for name in SHAPES for w in (name, "ok")]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_row_loop_has_no_image_and_no_barrier(program, shape):
    src = _dump(program, shape)
    ncols, late, pred8, fac8 = SHAPES[shape]
    assert "sval" not in src
    assert "#define DS 8\n" in src
    assert "__launch_bounds__(WG, 4)" in src
    head = src.index("for (int base = tile.row_start; base < tile_end;")
    end = src.index("    pb ^= 1;\n", head)
    assert "__syncthreads()" not in src[head:end]
    # one barrier per tile: between the tile loop's head and the row loop
    tile = src.index("for (int t = blockIdx.x; t < ntiles; t += gridDim.x)")
    assert src[tile:head].count("__syncthreads();") == 1
    for c in range(ncols):
        reads = [m.start() for m in re.finditer(rf"\(body{c}\b", src)]
        if c in late:
            # one read, inside the row loop, the whole statement under `ok`
            assert len(reads) == 1 and head < reads[0] < end, (c, reads)
            line = src[src.rindex("\n", 0, reads[0]) + 1:src.index("\n", reads[0])]
            assert line.strip() == (f"if (ok) e{c}[k] = ((const GAS double *)"
                                    f"(body{c} + (u64)base * 8))[r];"), line
            assert f"e{c}[k] = 0.0;" in src
        else:
            # the first step's loads and the next step's, clamped into the tile
            assert len(reads) == 2 and reads[0] < head < reads[1] < end
            for at in reads:
                line = src[src.rindex("\n", 0, at) + 1:src.index("\n", at)]
                assert re.fullmatch(
                    rf"\s*x{c}\[k\] = \(\(const GAS [a-z ]+ \*\)"
                    rf"\(body{c} \+ \(u64\)\((tile\.row_start|nbase)\) \* "
                    rf"[124]\)\)\[rr\];", line), line
        assert (f"u64 spass{c}[2][4];" in src) == (c in pred8)
        assert (f"double svd{c}[2][WG];" in src) == (c in fac8)
        if c in pred8:
            assert f"spass{c}[pb][tid >> 6] = m;" in src
            assert f"ok &= (int)((pw{c}[x{c}[k] >> 5] >> (x{c}[k] & 31u)) & 1u);" in src
        if c in fac8:
            assert f"svd{c}[pb][tid] = vd{c}[tid];" in src
            assert f"svd{c}[pb][f{c}[k]]" in src
    assert src.count("min((unsigned)(tid + k * WG),") == 2
    pass_a = src[head:src.index("const int nbase", head)]
    assert "int ok = base + r < tile_end;" in pass_a and "okv[k] = ok;" in pass_a
    assert ("del[(u64)gr >> 6]" in pass_a) == shape.endswith("_del")
    assert "sums[0] += ok ? va0 : 0.0;" in src[head:end]
    assert "rcnt += ok ? 1.0 : 0.0;" in src[head:end]


def test_two_range_predicates_on_an_int16_column(program):
    src = _dump(program, "direct_keyless_i16")
    assert "x0[k] = ((const GAS short *)" in src
    for i in (0, 1):
        assert (f"{{ const double x = (double)x0[k];\n"
                f"          ok &= (x >= pd{i}_lo) & (x <= pd{i}_hi); }}") in src
    assert "const double va1 = (double)f0[k] * e1[k];" in src


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_late_tag_keeps_its_text(program, shape):
    with open(os.path.join(REPO, "tests", "fixtures",
                           "jit_late_twin_source.txt")) as f:
        parts = re.split(r"/\* ==== (\w+) ==== \*/\n", f.read())
    was = dict(zip(parts[1::2], parts[2::2]))
    assert set(was) == set(SHAPES)
    now = _dump(program, shape, "--late-twin")
    assert now == was[shape]
    assert "sval" in now and "#define DS" not in now
