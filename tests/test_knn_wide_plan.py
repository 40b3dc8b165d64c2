"""CPU check of the host plan of the wide exact search (k up to 64).

Like tests/test_q8_stage_plan.py: the plan is a pure host header
(kakveda_amd/ops/hip/knn_wide_plan.h: the k clamp, whether a floor can exist,
the kernel choice, the record-segment capacity, the slices of the overflow
fallback and the groups of streamed batches), so it is compiled into a
stand-alone program (tests/host/knn_wide_plan_test.cpp) with the host C++
compiler under AddressSanitizer + UBSan and run here: no GPU, no torch.
"""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "knn_wide_plan_test.cpp")
INC = os.path.join(REPO, "kakveda_amd", "ops", "hip")


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_knn_wide_plan(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knn_wide_plan_test")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "cases passed" in run.stdout
