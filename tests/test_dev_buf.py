"""ponyc_amd/csrc/dev_buf.h, the engine's owning buffer type, exercised by a
stand-alone program (tests/c_abi/dev_buf_check.cpp): alloc, re-alloc, move,
swap, reset, and the failure path — without a GPU every allocation fails, and
the program asserts an empty buffer and zero live counts after each."""
import os
import subprocess

from ponyc_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "dev_buf_check.cpp")


def test_dev_buf_check(tmp_path):
    exe = str(tmp_path / "dev_buf_check")
    cmd = [build.HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", "-O1", "-Wall", "-Werror",
           "-I", build.CSRC, SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dev_buf_check: ok" in r.stdout
