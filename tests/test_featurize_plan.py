"""CPU check of the device featurizer's contract (ops/hip/featurize_plan.h).

featurize_one, the serial C++ statement of what the kernel computes, is
compiled into a stand-alone program with the host C++ compiler under
AddressSanitizer + UBSan and run on a case file written here: the edge
texts at several hash_dims and seeds, with the rows Python's featurizer
gives. Indices must be equal; weights agree to 2^-18 (values of at most 1
through fewer than 64 fp32 roundings, against float64-then-float32). No
GPU, no torch in the program.
"""

import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featurize_cases as fc  # noqa: E402

from kakveda_amd import ops  # noqa: E402
from kakveda_amd.encoder.featurizer import featurize  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "featurize_plan_test.cpp")
INC = os.path.join(REPO, "kakveda_amd", "ops", "hip")

HASH_DIMS = (8, 64, 1000, 65536)
SEEDS = (0, 0x5EED1234ABCD)
MAX_FEATURES = 128


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def _case(text, hash_dim, seed, max_features):
    status = fc.expected_status(text, hash_dim, seed, max_features)
    idx, w = featurize(text, hash_dim=hash_dim, seed=seed) if status == 0 else ((), ())
    raw = text.encode("ascii")
    head = "%d %d %d %d %d %d" % (
        hash_dim, ops.featurize_start_state(seed), max_features, status, len(idx), len(raw)
    )
    return "\n".join(
        (
            head,
            " ".join(str(b) for b in raw),
            " ".join(str(int(i)) for i in idx),
            " ".join(repr(float(x)) for x in w),
        )
    )


def _cases():
    cases, statuses = [], set()
    for hash_dim in HASH_DIMS:
        for seed in SEEDS:
            for _name, text in fc.edge_texts():
                cases.append(_case(text, hash_dim, seed, MAX_FEATURES))
    # exactly max_features features, and one more
    for hash_dim, mf in ((64, 8), (1000, 64), (65536, 128)):
        for seed in SEEDS:
            cases.append(_case(fc.with_features(mf, hash_dim, seed), hash_dim, seed, mf))
            cases.append(_case(fc.with_features(mf + 1, hash_dim, seed), hash_dim, seed, mf))
    for c in cases:
        statuses.add(int(c.split()[3]))
    assert statuses == {0, 1, 2}  # the list reaches every status
    return cases


def test_featurize_one_matches_python(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "featurize_plan_test")
    build = subprocess.run(
        [cxx, "-std=c++17", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr[-3000:]
    cases = _cases()
    case_file = tmp_path / "cases.txt"
    case_file.write_text("%d\n" % len(cases) + "\n".join(cases) + "\n")
    run = subprocess.run([exe, str(case_file)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "all checks passed (%d cases)" % len(cases) in run.stdout
