"""CPU check of the routed-search plan (ops/hip/ivf_plan.h).

The plan is a pure host header: row -> segment mapping, slice and slot
counts, segment-layout refusals. It is compiled into a stand-alone program
with the host C++ compiler under AddressSanitizer + UBSan and run here — no
GPU, no torch.
"""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "ivf_plan_test.cpp")
INC = os.path.join(REPO, "kakveda_amd", "ops", "hip")


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_ivf_plan_table(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ivf_plan_test")
    build = subprocess.run(
        [cxx, "-std=c++17", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "all checks passed" in run.stdout
