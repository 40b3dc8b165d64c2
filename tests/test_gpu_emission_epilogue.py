"""GPU tests for the emission epilogue of the 256x256 8-phase top-k kernel:
floors read once per block, the wave-private LDS stash, the block-private
record segments with their binning kernel, and the floor depth k of the
emission probes.

Shapes are the smallest that reach the places it can break: two row tiles
with a partial second one, a partial last column tile, one K window per tile
(D = 64: the epilogue abuts the staging), every row group of a wave
qualifying at once (the stash must drain and refill), and a segment that
overflows while no row does."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_MAX = 65792
B_MAX = 300


def _unit_bf16(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, generator=g, device="cuda")
    return (x / x.norm(dim=-1, keepdim=True)).to(torch.bfloat16)


_DATA = {}


def _data(D):
    """(queries [300, D], corpus [65792, D], fp32 sims [300, 65792]); built
    once per D, shared by every case and never written to."""
    if D not in _DATA:
        q = _unit_bf16(B_MAX, D, seed=300 + D)
        c = _unit_bf16(N_MAX, D, seed=400 + D)
        _DATA[D] = (q, c, q.float() @ c.float().t())
    return _DATA[D]


def _assert_exact(s, i, sims, k):
    B, N = sims.shape
    rs, _ = torch.topk(sims, k, dim=1)
    assert s.shape == (B, k) and i.shape == (B, k)
    assert (i >= 0).all() and (i < N).all()
    assert torch.allclose(s, rs, atol=2e-2, rtol=1e-2), (s - rs).abs().max().item()
    gathered = sims.gather(1, i)
    assert torch.allclose(gathered, s, atol=1e-4), (gathered - s).abs().max().item()
    assert torch.allclose(gathered, rs, atol=1e-4), (gathered - rs).abs().max().item()


def _check_exact_repeat(D, B, N, k, calls=3):
    from kakveda_amd import ops

    q_all, c_all, sims_all = _data(D)
    q = q_all[:B].contiguous()
    c = c_all[:N]
    outs = []
    for _ in range(calls):
        s, i = ops.cosine_topk(q, c, k)
        outs.append((s.clone(), i.clone()))
    torch.cuda.synchronize()
    _assert_exact(outs[0][0], outs[0][1], sims_all[:B, :N], k)
    for s, i in outs[1:]:
        assert torch.equal(s, outs[0][0])
        assert torch.equal(i, outs[0][1])


@pytest.mark.parametrize("k", [2, 5, 8])
def test_emission_epilogue_exact_vs_torch(k):
    _check_exact_repeat(768, 300, 65700, k)


def test_emission_epilogue_exact_one_window():
    """D = 64: one K window per tile, the epilogue abuts the staging."""
    _check_exact_repeat(64, 300, 65700, 5)


def _dec_f32(u32):
    """The kernels' order-preserving u32 -> f32 decoding (dec_f32)."""
    u = np.asarray(u32).astype(np.uint32)
    b = np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u)
    return b.astype(np.uint32).view(np.float32)


def _check_counts_and_candidates(q, c, sims, k, preg):
    """Per-row emitted counts against the decoded floor, and every emitted
    candidate against the fp32 scores."""
    from kakveda_amd.ops import _require_ext

    ext = _require_ext()
    B, N = sims.shape
    cc, cand, rowthr = ext.emit_counts_probe(q, c, preg, k=k)
    torch.cuda.synchronize()
    cc = cc.long()
    floor = torch.from_numpy(_dec_f32(rowthr.cpu().numpy().view(np.uint32))).cuda()
    assert torch.isfinite(floor).all()
    lo = (sims >= (floor + 1e-4)[:, None]).sum(dim=1)
    hi = (sims >= (floor - 1e-4)[:, None]).sum(dim=1)
    print("counts min/max", cc.min().item(), cc.max().item(),
          "bounds", lo.min().item(), hi.max().item())
    assert (cc >= lo).all(), (cc - lo).min().item()
    assert (cc <= hi).all(), (cc - hi).max().item()
    assert (cc >= k).all()

    width = int(cc.max().item())
    assert width <= cand.shape[1]
    e = cand[:, :width]
    valid = torch.arange(width, device="cuda")[None, :] < cc[:, None]
    cols = 0x7FFFFFFF - (e & 0xFFFFFFFF)
    enc = ((e >> 32) & 0xFFFFFFFF).cpu().numpy().astype(np.uint32)
    score = torch.from_numpy(_dec_f32(enc)).cuda()
    vc = cols[valid]
    assert (vc >= 0).all() and (vc < N).all()
    rows = torch.arange(B, device="cuda")[:, None].expand(B, width)[valid]
    keys = rows * N + vc
    assert torch.unique(keys).numel() == keys.numel(), "duplicate candidate"
    true = sims[rows, vc]
    err = (score[valid] - true).abs().max().item()
    assert err <= 1e-4, err
    return cc, floor


def test_emission_burst_refills_stash():
    """256 identical queries whose 8 best columns sit in one wave's 64-column
    span of one tile: all 32 row groups of that wave qualify at once, more
    than the stash holds, so it must drain and refill. N = 65792 makes the
    prepass sample the whole corpus, so the floor is the exact 8th best and
    each row emits exactly its top 8."""
    from kakveda_amd import ops

    D, B, N, k = 768, 256, 65792, 8
    _, c_all, _ = _data(D)
    g = torch.Generator(device="cuda").manual_seed(77)
    q1 = torch.randn(D, generator=g, device="cuda")
    q1 = q1 / q1.norm()
    c = c_all[:N].clone()
    for j in range(8):  # distinct noisy copies: cosine ~0.99 down to ~0.8
        noise = torch.randn(D, generator=g, device="cuda")
        noise = noise / noise.norm()
        v = q1 + (0.15 + 0.08 * j) * noise
        c[1000 + j] = (v / v.norm()).to(torch.bfloat16)
    q = q1.to(torch.bfloat16)[None, :].repeat(B, 1).contiguous()
    sims = q.float() @ c.float().t()

    s, i = ops.cosine_topk(q, c, k)
    torch.cuda.synchronize()
    _assert_exact(s, i, sims, k)
    assert torch.equal(i.sort(dim=1).values,
                       torch.arange(1000, 1008, device="cuda")[None, :].expand(B, 8))
    # preg 72 = the plan's prepass grid at this shape: the whole corpus
    cc, _ = _check_counts_and_candidates(q, c, sims, k, 72)
    assert (cc == 8).all()


def test_emission_counts_follow_kth_floor():
    """Random data, whole corpus sampled, floor depth k = 5 given to the
    probe: the floor is the exact 5th best, so a row emits its top 5 and
    nothing below (an 8th-best floor would emit 8 and break the upper
    bound)."""
    D, B, N, k = 768, 130, 65536, 5
    q_all, c_all, sims_all = _data(D)
    q = q_all[:B].contiguous()
    c = c_all[:N]
    # preg 64 = the plan's prepass grid at this shape: the whole corpus
    _check_counts_and_candidates(q, c, sims_all[:B, :N], k, 64)


_OVERFLOW_CHILD = r"""
import sys, torch
from kakveda_amd import ops
def unit(n, d, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(n, d, generator=g, device='cuda')
    return (x / x.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
B, N, D, k = 130, 65600, 128, 5
q, c = unit(B, D, 21), unit(N, D, 22)
sims = q.float() @ c.float().t()
rs, _ = torch.topk(sims, k, dim=1)
for call in range(2):
    s, i = ops.cosine_topk(q, c, k)
    torch.cuda.synchronize()
    assert s.shape == (B, k) and i.shape == (B, k)
    assert (i >= 0).all() and (i < N).all()
    assert torch.allclose(s, rs, atol=2e-2, rtol=1e-2), (s - rs).abs().max().item()
    gathered = sims.gather(1, i)
    assert torch.allclose(gathered, s, atol=1e-4), (gathered - s).abs().max().item()
    assert torch.allclose(gathered, rs, atol=1e-4), (gathered - rs).abs().max().item()
print('child ok')
"""


def test_emission_segment_overflow_falls_back_exact():
    """One record per segment: at least 650 candidates (130 rows x k = 5)
    over at most 65 non-empty blocks overflow some segment while no row
    comes near its cap. Both calls must come back exact through the
    fallback, with one warning. The knobs are read once per process, so
    this is a subprocess."""
    env = dict(os.environ)
    for name in ("KAKVEDA_KNN_KERNEL", "KAKVEDA_KNN_EMIT_CAP"):
        env.pop(name, None)
    env["KAKVEDA_KNN_EMIT_SEG"] = "1"
    r = subprocess.run(
        [sys.executable, "-c", _OVERFLOW_CHILD], env=env, capture_output=True,
        text=True, timeout=300, cwd=REPO,
    )
    assert r.returncode == 0, r.stderr[-1500:]
    assert "child ok" in r.stdout
    assert r.stderr.count("emission candidate overflow") == 1, r.stderr[-1500:]
