"""CPU check of the list-major routed-scan plan (ops/hip/ivf_batch_plan.h).

The plan is a pure host header: the bound on the tile count that sizes the
launch without a device read, slice and slot counts, the candidate-byte cap
and the chunking that keeps to it. It is compiled into a stand-alone program
with the host C++ compiler under AddressSanitizer + UBSan and run here - no
GPU, no torch.
"""

import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "ivf_batch_plan_test.cpp")
INC = os.path.join(REPO, "kakveda_amd", "ops", "hip")


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_ivf_batch_plan_table(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ivf_batch_plan_test")
    build = subprocess.run(
        [cxx, "-std=c++17", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "all checks passed" in run.stdout


def test_python_mirrors_the_header():
    from kakveda_amd import ops

    text = open(os.path.join(INC, "ivf_batch_plan.h")).read()
    qtile = int(re.search(r"constexpr int IVF_BATCH_QTILE = (\d+);", text).group(1))
    assert ops.IVF_BATCH_QTILE == qtile and qtile >= 16
    for P, L in [(0, 5), (3, 3160), (15, 1), (200, 1), (67584, 3160), (100, 0)]:
        assert ops.ivf_batch_tile_bound(P, L) == min(P, P // qtile + L + 1)
    max_d = int(re.search(r"constexpr int IVF_BATCH_MAX_D = (\d+);", text).group(1))
    assert ops.IVF_BATCH_MAX_D == max_d
    # the constant the size dispatch uses is never below 64
    assert ops.IVF_BATCHED_MIN_B is None or ops.IVF_BATCHED_MIN_B >= 64


def test_size_dispatch(monkeypatch):
    from kakveda_amd import ops

    # an explicit choice always holds; None goes by batch size and row width
    assert ops._use_batched(True, 1, 768) and not ops._use_batched(False, 4096, 768)
    monkeypatch.setattr(ops, "IVF_BATCHED_MIN_B", 128)
    assert not ops._use_batched(None, 127, 768)
    assert ops._use_batched(None, 128, 768)
    assert ops._use_batched(None, 128, ops.IVF_BATCH_MAX_D)
    assert not ops._use_batched(None, 4096, ops.IVF_BATCH_MAX_D + 64)
    monkeypatch.setattr(ops, "IVF_BATCHED_MIN_B", None)
    assert not ops._use_batched(None, 1 << 20, 768)
