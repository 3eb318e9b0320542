"""csrc/partial_format.h under AddressSanitizer and UBSan, on the CPU.

tests/partial_format_host.cpp is a stand-alone host program (its own main,
only partial_format.h included, no engine, no HIP): partial blocks round-trip
through the writers and the bounds-checked reader, every block sits in a heap
buffer of exactly the bytes the reader is told about (a read past `stride` is
a heap overflow the sanitizer reports and aborts on), and the merge's fold,
group identity, shard hash, result-value rule and accumulator-row decoder are
checked against hand-written values."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "partial_format_host.cpp")
READER_FIELDS = ("stride", "count", "key", "keyless")
# (keys hashed, None = NULL): the tuples the program must print, in order
HASH_TUPLES = [(b"",), (b"a",), (b"ab", b"c"), (None, b"x"), (b"x", None),
               (b"z" * 47,)]
WORLDS = (1, 2, 3, 1024)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("partial_format") / "partial_format_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", exe, SRC]
    # static sanitizer runtimes where the compiler offers them: a shared ASan
    # runtime refuses to start behind any other preloaded library (see
    # test_blob_format_asan.py)
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + static, capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_sanitizers_silent_and_every_case_ok(run):
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK"
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr
    cases = [ln for ln in lines if ln.startswith("case ")]
    assert len(cases) >= 20 and all(ln.endswith(" ok") for ln in cases), cases


def test_reader_accepted_and_rejected_every_field(run):
    """a loop that never ran cannot pass: the block reader saw inputs of both
    outcomes for every field it checks"""
    seen = {}
    for ln in run.stdout.splitlines():
        m = re.match(r"reader (\w+) seen (\d+) accepted (\d+) rejected (\d+)", ln)
        if m:
            seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    assert sorted(seen) == sorted(READER_FIELDS), run.stdout[-2000:]
    for name, (n, ok, bad) in seen.items():
        assert ok >= 1 and bad >= 1 and ok + bad == n, (name, n, ok, bad)
    # every stride from 0 to one byte short of 8 + 2 * 304, and the exact one
    assert seen["stride"] == (8 + 2 * 304 + 1, 1, 8 + 2 * 304)


def fnv1a(keys):
    h = 1469598103934665603
    for k in keys:
        for b in (b"\x01" if k is None else k) + b"\xff":
            h = ((h ^ b) * 1099511628211) & (2 ** 64 - 1)
    return h


def test_shard_hash_is_fnv1a(run):
    """ranks running different builds must agree on the owner of a key"""
    got = []
    for ln in run.stdout.splitlines():
        m = re.match(r"hash ng (\d+) keys (.*) h ([0-9a-f]{16}) shards (.*)$", ln)
        if not m:
            continue
        keys = tuple(None if t == "NULL" else bytes.fromhex(t[1:])
                     for t in m.group(2).split())
        assert len(keys) == int(m.group(1))
        got.append(keys)
        h = fnv1a(keys)
        assert int(m.group(3), 16) == h, ln
        assert [int(x) for x in m.group(4).split()] == [h % w for w in WORLDS], ln
    assert got == HASH_TUPLES
