"""csrc/tail_window.h (the integer form of a window of k_tail_replay) against sequential double additions: tests/host/tail_window_harness.cpp built
with g++ and run on the CPU -- three million random windows (values hovering in [64, 128), around 64.0 and 128.0, mixed pushes and pops, one operation
in 16 an exact tie) and the crafted ones (ties from an even and an odd value, sums that reach 2^(e+1), sums within half an ulp of 2^e from either side,
an incoming 0.0, a push of 0.0, windows of 1 and of 64 operations, subnormals).  Once more as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "tail_window_harness.cpp")


def build_and_run(tmp_path, flags, windows):
    exe = str(tmp_path / "tail_window_harness")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", *flags, "-o", exe, SRC])
    r = subprocess.run([exe, str(windows)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout
    return r.stdout


def test_window_arithmetic_equals_sequential_adds(tmp_path):
    out = build_and_run(tmp_path, ["-O2"], 3000000)
    assert "3000000 random windows" in out


def test_window_arithmetic_under_sanitizers(tmp_path):
    build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], 300000)
