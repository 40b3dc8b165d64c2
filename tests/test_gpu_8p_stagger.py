"""GPU tests for the staggered wave groups of the 256x256 8-phase top-k
kernel: group 1 (waves 4-7) runs one barrier behind group 0, and the
B(t+2) staging issues sit one phase later than on the lockstep schedule.

Shapes are the smallest that reach the places the schedule can break:
one / two / twelve K windows per tile (D = 64 / 128 / 768), a chunk whose
last tile is partial and alone (the drain-to-zero tail), a two-tile last
chunk, padded empty chunks, and a row tile where only group 0 holds real
rows."""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

N_MAX = 66000
B_MAX = 300


def _unit_bf16(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, generator=g, device="cuda")
    return (x / x.norm(dim=-1, keepdim=True)).to(torch.bfloat16)


_DATA = {}


def _data(D):
    """(queries [300, D], corpus [66000, D], fp32 sims [300, 66000]); built
    once per D, shared by every case and never written to."""
    if D not in _DATA:
        q = _unit_bf16(B_MAX, D, seed=100 + D)
        c = _unit_bf16(N_MAX, D, seed=200 + D)
        _DATA[D] = (q, c, q.float() @ c.float().t())
    return _DATA[D]


def _check_exact(D, B, N, k):
    from kakveda_amd import ops

    q_all, c_all, sims_all = _data(D)
    q = q_all[:B].contiguous()
    c = c_all[:N]
    sims = sims_all[:B, :N]
    s, i = ops.cosine_topk(q, c, k)
    torch.cuda.synchronize()
    rs, _ = torch.topk(sims, k, dim=1)
    assert s.shape == (B, k) and i.shape == (B, k)
    assert (i >= 0).all() and (i < N).all()
    assert torch.allclose(s, rs, atol=2e-2, rtol=1e-2), (s - rs).abs().max().item()
    gathered = sims.gather(1, i)
    # a stale or torn tile shows here: the claimed column's true score
    assert torch.allclose(gathered, s, atol=1e-4), (gathered - s).abs().max().item()
    assert torch.allclose(gathered, rs, atol=1e-4), (gathered - rs).abs().max().item()
    return s, i


@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize(
    "B,N",
    [
        (9, 65536),    # smallest MFMA-emission batch: only group 0 has rows
        (300, 65700),  # 2 row tiles (2nd: 44 rows); last chunk = 1 partial tile
        (256, 66000),  # last chunk has two tiles
    ],
)
def test_emission_stagger_exact_vs_torch(B, N, k):
    _check_exact(768, B, N, k)


@pytest.mark.parametrize("D", [64, 128])
def test_emission_stagger_short_k(D):
    """One and two windows per tile: the t+1 / t+2 staging crosses a tile
    boundary in every window and the shifted B issue abuts the epilogue."""
    _check_exact(D, 300, 65700, 5)


def test_emission_stagger_repeatable():
    """Five calls on the same buffers are bit-equal; a difference is an
    ordering bug in the staging ledger."""
    from kakveda_amd import ops

    q_all, c_all, _ = _data(768)
    q = q_all[:300].contiguous()
    c = c_all[:65700]
    outs = []
    for _ in range(5):
        s, i = ops.cosine_topk(q, c, 5)
        outs.append((s.clone(), i.clone()))
    torch.cuda.synchronize()
    for s, i in outs[1:]:
        assert torch.equal(s, outs[0][0])
        assert torch.equal(i, outs[0][1])


def test_emission_stagger_matches_list_kernel(tmp_path):
    """Default (staggered emission) and the forced 128x128 list kernel give
    bit-equal scores and equal ids. The kernel selection is read once per
    process, so the list run is a subprocess that regenerates the same
    seeded inputs."""
    from kakveda_amd import ops

    q = _unit_bf16(300, 768, seed=11)
    c = _unit_bf16(131072, 768, seed=12)
    s, i = ops.cosine_topk(q, c, 5)
    torch.cuda.synchronize()
    outp = str(tmp_path / "out.pt")
    code = (
        "import sys, torch\n"
        "from kakveda_amd import ops\n"
        "def unit(n, seed):\n"
        "    g = torch.Generator(device='cuda').manual_seed(seed)\n"
        "    x = torch.randn(n, 768, generator=g, device='cuda')\n"
        "    return (x / x.norm(dim=-1, keepdim=True)).to(torch.bfloat16)\n"
        "s, i = ops.cosine_topk(unit(300, 11), unit(131072, 12), 5)\n"
        "torch.cuda.synchronize()\n"
        "torch.save((s.cpu(), i.cpu()), sys.argv[1])\n"
    )
    env = dict(os.environ)
    env["KAKVEDA_KNN_KERNEL"] = "list"
    r = subprocess.run(
        [sys.executable, "-c", code, outp], env=env, capture_output=True,
        text=True, timeout=300,
    )
    assert r.returncode == 0, r.stderr[-1500:]
    ls, li = torch.load(outp)
    assert torch.equal(s.cpu(), ls), (s.cpu() - ls).abs().max().item()
    assert torch.equal(i.cpu(), li)


def test_probe8p_times_staggered_and_lockstep_core():
    """probe8p runs the GEMM-only core on both schedules (mode 1 staggered,
    mode 16 lockstep) on the same buffers; nothing is asserted about speed."""
    from kakveda_amd.ops import _require_ext

    ext = _require_ext()
    q_all, c_all, _ = _data(768)
    q = q_all[:256].contiguous()
    c = c_all[:65536]
    for mode in (1, 16):
        ms = ext.probe8p(q, c, mode, 2)
        assert ms > 0.0, (mode, ms)
