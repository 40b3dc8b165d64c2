"""CPU check of the int8 mirror's contract (ops/hip/q8_plan.h).

The pieces the quantiser kernel is built from (q8_scale, q8_code, q8_err)
are compiled into a stand-alone program with the host C++ compiler under
AddressSanitizer + UBSan and run, as a serial quantiser, on a case file
written here: the rows of tests/q8_cases.py with the codes and scales of
``ops.quantize_rows_q8_ref``. Codes and scale bits must be equal, and the
stored error must bound the residual norm within 1%. No GPU, no torch in the
program.
"""

import os
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cases as qc  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "q8_plan_test.cpp")
INC = os.path.join(REPO, "kakveda_amd", "ops", "hip")


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_serial_quantiser_matches_reference(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "q8_plan_test")
    build = subprocess.run(
        [cxx, "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr[-3000:]
    d = 128
    rows = torch.cat([qc.quantiser_rows(d, 300, 31), qc.encoder_rows(40, d)])
    codes, meta = qc.quantise_ref(rows)
    bits = meta[:, 0].contiguous().view(torch.int32).tolist()
    lines = ["%d %d" % (rows.shape[0], d)]
    for r in range(rows.shape[0]):
        lines.append(" ".join(repr(v) for v in rows[r].float().tolist()))
        lines.append(" ".join(str(v) for v in codes[r].tolist()))
        lines.append(str(bits[r] & 0xFFFFFFFF))
    case_file = tmp_path / "rows.txt"
    case_file.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(case_file)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "all checks passed (%d rows)" % rows.shape[0] in run.stdout
