"""CPU check of the prepass launch geometry in the dispatch plan.

Like tests/test_knn_main_geom.py: the plan is a pure host header, so the rule
that the compact prepass of the emission floors runs one round of long
blocks over an unchanged sample (KnnPlan::pre_grid / pre_tiles, which plans
keep one block per sampled chunk, the KAKVEDA_KNN_PRE_TILES parsing and which
forced sizes a request refuses) is compiled into a stand-alone program
(tests/host/knn_prepass_geom_test.cpp) with the host C++ compiler under
AddressSanitizer + UBSan and run here — no GPU, no torch.
"""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "knn_prepass_geom_test.cpp")
INC = os.path.join(REPO, "kakveda_amd", "ops", "hip")


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_knn_prepass_launch_geometry(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knn_prepass_geom_test")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "cases passed" in run.stdout
