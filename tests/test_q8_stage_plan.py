"""CPU check of the stage plan of the batched int8 screen.

Like tests/test_knn_main_geom.py: the plan is a pure host header, so the rule
that cuts the screen's main launch into stages (knn_plan.h plan_q8_stages:
where the boundaries fall, how each stage is chunked, when the stage count is
reduced, the candidate-count model and the KAKVEDA_Q8_STAGES parsing) is
compiled into a stand-alone program (tests/host/q8_stage_plan_test.cpp) with
the host C++ compiler under AddressSanitizer + UBSan and run here: no GPU, no
torch.
"""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "q8_stage_plan_test.cpp")
INC = os.path.join(REPO, "kakveda_amd", "ops", "hip")


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_q8_stage_plan(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "q8_stage_plan_test")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "cases passed" in run.stdout
