"""CPU checks of the batched int8 screen (ops/hip/q8_plan.h "Screening test").

tests/host/q8_screen_test.cpp is compiled into a stand-alone program with the
host C++ compiler under AddressSanitizer + UBSan and run: the serial screen
reference never rejects a pair whose exact score reaches the floor, and the
kernel's form of the test accepts whatever the reference accepts (random,
all-zero, one-hot and outlier rows; queries down to a tiny amax; D = 128 and
768).

The torch reference path: ``ops.cosine_topk_q8_ref`` at a batch of at least
``ops.Q8_BATCH_MIN_B`` queries equals ``ops.cosine_topk_ref``; the
``ShardedStore`` mirror defaults; the KAKVEDA_Q8_BATCH knob.
"""

import os
import shutil
import subprocess
import sys

import pytest
import torch

from kakveda_amd import ops
from kakveda_amd.parallel.sharded import ShardedStore

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "q8_screen_test.cpp")
INC = os.path.join(REPO, "kakveda_amd", "ops", "hip")

N = 70_001  # emission needs N >= 65,536; not a multiple of 256


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_serial_screen_is_a_superset(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "q8_screen_test")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "all checks passed" in run.stdout


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    return x / x.norm(dim=1, keepdim=True)


@pytest.fixture(scope="module")
def corpus128():
    c = _unit(N, 128, 11)
    codes, meta = ops.new_q8_mirror(N, 128, "cpu")
    cn = ops.new_q8_cnorm("cpu")
    ops.quantize_rows_q8(c, codes, meta, 0, cn)
    return c, codes, meta, cn


def test_cnorm_bounds_every_row_norm(corpus128):
    c, _codes, _meta, cn = corpus128
    top = float(c.double().norm(dim=1).max())
    assert top <= float(cn) <= top * (1 + 1e-4)


@pytest.mark.parametrize("k", [2, 5, 8])
def test_batched_ref_equals_plain_ref(corpus128, k):
    c, codes, meta, cn = corpus128
    B = max(ops.Q8_BATCH_MIN_B, 9) + 3
    q = _unit(B, 128, 12 + k)
    assert ops.q8_batch_in_plan(B, N, k, 128, False, min_rows=1)
    before = ops.q8_overflow_fallbacks + ops.q8_degenerate_fallbacks
    s, i = ops.cosine_topk_q8_ref(q, c, codes, meta, k, cnorm=cn, batch_min_rows=1)
    assert ops.q8_overflow_fallbacks + ops.q8_degenerate_fallbacks == before
    s0, i0 = ops.cosine_topk_ref(q, c, k)
    assert torch.equal(s, s0) and torch.equal(i, i0)
    # the public op takes the same path on the CPU
    s1, i1 = ops.cosine_topk_q8(q, c, codes, meta, k, cnorm=cn, batch_min_rows=1)
    assert torch.equal(s1, s0) and torch.equal(i1, i0)


def test_batched_ref_screens_rather_than_passes_everything(corpus128):
    """The reference's candidate mask keeps the true top-k and is a small part
    of the corpus: the equality above is not that of a mask of all ones."""
    c, codes, meta, cn = corpus128
    q = _unit(16, 128, 40)
    sims = q @ c.t()
    floors = torch.topk(sims, 8, dim=1).values[:, -1]
    qcodes, T, kappa, degenerate = ops.q8_screen_params_ref(q, floors, cn)
    assert degenerate == 0
    mask = ops.q8_screen_mask_ref(qcodes, codes, meta, T, kappa, N)
    assert bool(mask.gather(1, torch.topk(sims, 8, dim=1).indices).all())
    assert int(mask.sum(dim=1).max()) < N // 50


def test_degenerate_query_takes_the_plain_path(corpus128):
    c, codes, meta, cn = corpus128
    B = max(ops.Q8_BATCH_MIN_B, 9)
    q = _unit(B, 128, 50)
    q[3] = 0
    before = ops.q8_degenerate_fallbacks
    s, i = ops.cosine_topk_q8_ref(q, c, codes, meta, 5, cnorm=cn, batch_min_rows=1)
    assert ops.q8_degenerate_fallbacks == before + 1
    s0, i0 = ops.cosine_topk_ref(q, c, 5)
    assert torch.equal(s, s0) and torch.equal(i, i0)


def test_batch_knob(monkeypatch):
    B = max(ops.Q8_BATCH_MIN_B, 9)
    monkeypatch.delenv("KAKVEDA_Q8_BATCH", raising=False)
    monkeypatch.setattr(ops, "Q8_BATCH_MIN_ROWS", 1)
    assert ops.q8_batch_in_plan(B, N, 5, 768, False)
    assert not ops.q8_batch_in_plan(B, N, 5, 768, True)       # filtered
    assert not ops.q8_batch_in_plan(B, N, 1, 768, False)      # k = 1
    assert not ops.q8_batch_in_plan(B, 65_535, 5, 768, False)  # below emission
    assert not ops.q8_batch_in_plan(B, N, 5, 1152, False)     # D past the limit
    assert not ops.q8_batch_in_plan(B, N, 5, 192, False)      # D % 128
    assert not ops.q8_batch_in_plan(8, N, 5, 768, False, min_b=1)
    assert not ops.q8_batch_in_plan(B, N, 5, 768, False, min_rows=N + 1)
    assert not ops.q8_batch_in_plan(B - 1, N, 5, 768, False, min_b=B)
    monkeypatch.setenv("KAKVEDA_Q8_BATCH", "0")
    assert not ops.q8_batch_in_plan(B, N, 5, 768, False)
    monkeypatch.setenv("KAKVEDA_Q8_BATCH", "1")
    assert ops.q8_batch_in_plan(B, N, 5, 768, False)
    monkeypatch.setenv("KAKVEDA_Q8_BATCH", "yes")
    with pytest.raises(ValueError, match="KAKVEDA_Q8_BATCH"):
        ops.q8_batch_in_plan(B, N, 5, 768, False)


def test_sharded_store_mirror_defaults():
    assert ShardedStore(128, device="cpu").int8_mirror is False
    assert ShardedStore(128, device="cpu").local.int8_mirror is False
    on = ShardedStore(128, device="cpu", int8_mirror=True)
    assert on.int8_mirror is True and on.local.int8_mirror is True
    off = ShardedStore(128, device="cpu", int8_mirror=False)
    assert off.int8_mirror is False and off.local.int8_mirror is False


def test_sharded_store_search_is_the_same_with_the_mirror(corpus128, monkeypatch):
    # the store's searches take the batched path at this (small) corpus
    monkeypatch.setattr(ops, "Q8_BATCH_MIN_ROWS", 1)
    c, _codes, _meta, cn = corpus128
    B = max(ops.Q8_BATCH_MIN_B, 9) + 1
    q = _unit(B, 128, 60)
    on = ShardedStore(128, device="cpu", int8_mirror=True)
    on.load_shard(c, N)
    assert torch.equal(on.local._cnorm[0], cn)
    off = ShardedStore(128, device="cpu", int8_mirror=False)
    off.load_shard(c, N)
    seen = []
    real = ops.q8_batch_in_plan
    monkeypatch.setattr(ops, "q8_batch_in_plan", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    s1, i1 = on.search(q, 5)
    assert seen == [True]  # the mirror's batched path answered
    s0, i0 = off.search(q, 5)
    assert torch.equal(s1, s0) and torch.equal(i1, i0)
    # append keeps the mirror and its cnorm current
    extra = 2.0 * _unit(4, 128, 61)
    on.append(extra)
    off.append(extra)
    assert max(float(x) for x in on.local._cnorm) >= 2.0
    s1, i1 = on.search(q, 5)
    s0, i0 = off.search(q, 5)
    assert torch.equal(s1, s0) and torch.equal(i1, i0)
