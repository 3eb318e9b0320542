"""csrc/blob_format.h under AddressSanitizer and UBSan, on the CPU.

tests/blob_format_asan.cpp is a stand-alone host program (its own main, only
blob_format.h included, no engine, no HIP): it builds a valid blob of every
kind, then decodes every proper prefix from an exact-size heap buffer and
every 4-byte header/positions/dictionary field overwritten with -1,
0x7fffffff and the blob length.  A read one byte past a truncated blob is a
heap overflow the sanitizer reports and aborts on."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "blob_format_asan.cpp")
DECODERS = ("column", "delete_mask", "delta", "snappy")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("blob_format") / "blob_format_asan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", exe, SRC]
    # gcc links the sanitizer runtimes as shared libraries unless told
    # otherwise, and a shared ASan runtime refuses to start behind any other
    # preloaded library; linked in statically it needs nothing from the
    # environment.  A compiler that does not know the flags links statically
    # already.
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + static, capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_sanitizers_silent_and_blobs_roundtrip(run):
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-1] == "OK"
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr


def test_every_decoder_accepted_and_rejected_inputs(run):
    """a loop that never ran cannot pass: each decoder saw inputs of both
    outcomes"""
    seen = {}
    for ln in run.stdout.splitlines():
        m = re.match(r"decoder (\w+) seen (\d+) accepted (\d+) rejected (\d+)", ln)
        if m:
            seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    assert sorted(seen) == sorted(DECODERS), run.stdout[-2000:]
    for name, (n, ok, bad) in seen.items():
        assert ok >= 1 and bad >= 1 and ok + bad == n, (name, n, ok, bad)
