"""The join cases of tests/join_cases.py on the CPU: the oracle against the
numpy reference on every dimension set, key column and plan mode, so the
second opinion the GPU tests may ask is itself pinned on NULL keys and
extreme keys; and sn_lut_span under UBSan and AddressSanitizer.

tests/lut_span_host.cpp is a stand-alone host program (its own main, only
engine_internal.h included, no engine, no HIP)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import join_cases as jc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "lut_span_host.cpp")


def oracle_table(fx):
    t = po.OracleTable(jc.DTYPES, [1 if n else 0 for n in jc.NULLABLE])
    for s, e in fx.bounds():
        blobs = []
        for c, dt in enumerate(jc.DTYPES):
            ok = fx.valid[c][s:e]
            blobs.append(po.encode(dt, po.ENC_UNCOMPRESSED, fx.cols[c][s:e],
                                   None if ok.all() else ok.astype(np.uint8)))
        t.add_batch(e - s, blobs)
    return t


def oracle_rows(t, mode, key_col, aggs=jc.AGGS):
    plan = po.make_plan(**jc.plan_args(mode, key_col, 0, aggs))
    if mode == "semi":
        return {k: v for k, v in po.result_rows(t.query(plan))}
    return {k: v for k, v in t.query_groups(plan)}


@pytest.mark.parametrize("interpreted", [False, True], ids=["compiled", "interp"])
@pytest.mark.parametrize("name", sorted(jc.DIMSETS))
def test_oracle_equals_numpy(name, interpreted):
    dim = jc.DIMSETS[name]
    fx = jc.fact(dim, interpreted)
    t = oracle_table(fx)
    t.set_dim(np.array(dim.keys, dtype=np.int64), dim.attrs())
    for key_col in dim.key_cols():
        for mode in jc.MODES:
            exp = jc.reference(fx, key_col, dim.keys, dim.attrs(), mode)
            assert oracle_rows(t, mode, key_col) == exp, (key_col, mode)
    exp = jc.reference(fx, jc.C_K64, dim.keys, None, "semi_g3", jc.AGGS7)
    assert oracle_rows(t, "semi_g3", jc.C_K64, jc.AGGS7) == exp


def test_null_keys_are_dropped_not_joined_as_zero():
    """the figures of the defect: NULL slots hold a 0, the dimension holds
    the key 0, and the NULL rows still do not join"""
    dim = jc.LUT_EDGES[(204800, -100000)]
    fx = jc.fact(dim, True)
    keys, ok = fx.cols[jc.C_KN64], fx.valid[jc.C_KN64] & fx.valid[jc.C_F]
    as_zero = np.isin(keys, dim.keys) & fx.valid[jc.C_F]
    exp = jc.reference(fx, jc.C_KN64, dim.keys, None, "semi")[()]
    assert exp[1] == float((ok & np.isin(keys, dim.keys)).sum())
    assert exp[1] < float(as_zero.sum())       # the wrong answer differs


@pytest.mark.parametrize("name", sorted(jc.BUILDS))
def test_oracle_equals_numpy_on_build_tables(name):
    """the dimension a build table MEANS (NULL, deleted and patched rows
    applied) through the oracle"""
    b = jc.BUILDS[name]
    keys, attrs = b.effective()
    fx = jc.fact(jc.BUILD_FACT[name], False)
    t = oracle_table(fx)
    t.set_dim(np.array(keys, dtype=np.int64), attrs)
    for mode in ("semi", "attr"):
        exp = jc.reference(fx, jc.C_K64, keys, attrs, mode)
        assert oracle_rows(t, mode, jc.C_K64) == exp, mode


def test_oracle_refuses_int64_min_as_dimension_key():
    fx = jc.fact(jc.EXTREME, False)
    t = oracle_table(fx)
    with pytest.raises(AssertionError):
        t.set_dim(np.array([1, jc.I64_MIN, 3], dtype=np.int64))


def test_chain_sets_hold_their_precondition():
    """restated here so it is reported as a test, not an import error"""
    jc.check_chain(jc.HASH_CHAIN.keys, jc.HASH_CHAIN.near, jc.put_cap(12))
    jc.check_chain(jc.BUILD_CHAIN.keys, jc.BUILD_CHAIN.near, jc.build_cap(12))
    assert jc.put_cap(12) == 32 and jc.build_cap(12) == 1024
    # the splitmix64 finaliser's published first output for state 0
    assert jc.mix64(0) == 0xE220A8397B1DCDAF


# --------------------------------------------------------------- sn_lut_span


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("lut_span") / "lut_span_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
           "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
           "-o", exe, SRC]
    # a shared ASan runtime refuses to start behind another preloaded
    # library; linked in statically it needs nothing from the environment
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + static, capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_lut_span_clean_under_ubsan_and_asan(run):
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-1] == "OK"
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr
    # a loop that never ran cannot pass: all ten cases, of both outcomes
    m = re.search(r"cases (\d+) accepted (\d+) refused (\d+)", run.stdout)
    assert m and tuple(int(x) for x in m.groups()) == (10, 4, 6), run.stdout
