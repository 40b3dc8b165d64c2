"""GPU tests of the emission prepass launched as one round of long blocks.

The compact prepass behind the emission floors scores a fixed sample (the
first preg * 1024 corpus columns). How the sample is split into blocks
(pre_grid blocks of pre_tiles column tiles per row tile, knn_plan.h
prepass_geometry) must not change what comes out of it: a column's score
depends only on the K order inside its tile, so the sample's exact top-8,
the published floor and everything the main launch does with them stay what
the one-block-per-chunk launch (pre_tiles = 8) gives.

  floors        floor_probe at B = 300 (three row tiles, the last partial),
                N = 70,000, pregq = 64, pre_tiles 8 / 16 / 32 / 64 (grids
                64 / 32 / 16 / 8), and at B = 2048, N = 65,600, pre_tiles 16:
                32 x 16 = 512 blocks, the XCD-remapped branch of the kernel
  end to end    ops.cosine_topk at B = 2048 where the plan picks 32 x 16 (the
                smallest such N, where the sample is the corpus, and twice
                that, where the seeded main launch scans the rest), in child
                processes with the knob unset and with KAKVEDA_KNN_PRE_TILES=8
  filtered      a filtered B = 8 request keeps one block per chunk by the
                rule; forced to 16 tiles per block it returns the same
  bad values    refused with a RuntimeError, before anything is launched

D = 64 throughout (one K window per tile: the cheapest shape that runs the
whole path). The KAKVEDA_KNN_* settings are read once per process, hence the
children.
"""

import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_adversarial as ta  # noqa: E402

pytestmark = pytest.mark.gpu

D = 64
DEV = "cuda:0"


def gpu_unit(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, d, generator=g, device=DEV, dtype=torch.float32)
    x /= x.norm(dim=-1, keepdim=True)
    return x.to(torch.bfloat16)


# ---------------------------------------------------------------------------
# the plan's rule, mirrored (knn_plan.h plan_cosine_topk + prepass_geometry)
# ---------------------------------------------------------------------------

ROUND = 512  # PREPASS_ROUND: 2 resident blocks per CU, 256 CUs


def planned_prepass(B, N, pc):
    """(preg, pre_grid, pre_tiles) of the unfiltered 8-phase emission plan."""
    row_tiles8 = (B + pc["BM8"] - 1) // pc["BM8"]
    ntiles = (N + pc["BN8"] - 1) // pc["BN8"]
    want = (ntiles * row_tiles8 + pc["target8"] - 1) // pc["target8"]
    chunk_tiles = max(4, min(want, 128))
    nchunks = ((ntiles + chunk_tiles - 1) // chunk_tiles + 7) & ~7
    preg = min(pc["PREG_EMIT"], nchunks) & ~7
    total = preg * pc["PRE_TILES"]
    row_tiles = (B + pc["BM"] - 1) // pc["BM"]
    grid, tiles = preg, pc["PRE_TILES"]
    t = 2 * pc["PRE_TILES"]
    while total % t == 0:
        g = total // t
        if g % 8 or g * row_tiles < ROUND:
            break
        grid, tiles = g, t
        t *= 2
    return preg, grid, tiles


def smallest_long_block_n(B, pc):
    """Smallest N on the emission path whose plan runs pre_tiles > PRE_TILES
    (the plan changes with N only at multiples of BN8)."""
    n = pc["MIN_N_EMIT"]
    while planned_prepass(B, n, pc)[2] <= pc["PRE_TILES"]:
        n = (n // pc["BN8"] + 1) * pc["BN8"]
        assert n < 1 << 22
    return n


def test_plan_constants_match_the_mirror():
    pc = ta.plan_constants()
    text = open(os.path.join(ta.REPO, "kakveda_amd", "ops", "hip", "knn_plan.h")).read()
    assert re.search(r"constexpr int PREPASS_ROUND = 2 \* 256;", text)
    assert planned_prepass(2048, 10_000_000, pc) == (256, 32, 64)
    assert planned_prepass(2048, 1_250_000, pc) == (64, 32, 16)
    assert planned_prepass(256, 10_000_000, pc) == (256, 256, 8)


# ---------------------------------------------------------------------------
# floors across geometries
# ---------------------------------------------------------------------------

PREGQ = 64
SAMPLE = PREGQ * 8 * 128  # 65,536 columns


def _floors(B, N, seed):
    """(q, c, fp32 sims over the sample, the pre_tiles = 8 floors); built once
    per shape and never written to."""
    from kakveda_amd.ops import _require_ext

    q = gpu_unit(B, D, seed)
    c = gpu_unit(N, D, seed + 1)
    sims = q.float() @ c[:SAMPLE].float().t()
    s, i, thr = _require_ext().floor_probe(q, c, PREGQ, k=8, pre_tiles=8)
    torch.cuda.synchronize()
    return q, c, sims, (s.clone(), i.clone(), thr.clone())


@pytest.fixture(scope="module")
def floors_300():
    return _floors(300, 70_000, 7100)


@pytest.fixture(scope="module")
def floors_2048():
    return _floors(2048, 65_600, 7200)


def _check_floors(data, pre_tiles):
    from kakveda_amd.ops import _require_ext

    q, c, sims, (s8, i8, thr8) = data
    B = q.shape[0]
    s, i, thr = _require_ext().floor_probe(q, c, PREGQ, k=8, pre_tiles=pre_tiles)
    torch.cuda.synchronize()
    assert s.shape == (B, 8) and i.shape == (B, 8) and thr.shape == (B,)
    # the sample's top-8 scores and the published floor: bit for bit
    assert torch.equal(s.view(torch.int32), s8.view(torch.int32))
    assert torch.equal(thr, thr8)
    # ids: wherever the reference's nine best are pairwise distinct (equal
    # scores are all members of the result; which of them is unspecified)
    top9 = torch.topk(sims, 9, dim=1).values
    distinct = (top9[:, :-1] > top9[:, 1:]).all(dim=1)
    print("pre_tiles=%d rows with nine distinct best: %d of %d"
          % (pre_tiles, int(distinct.sum()), B))
    assert int(distinct.sum()) >= B - B // 16
    assert torch.equal(i[distinct], i8[distinct])
    # every returned id is a sampled column scoring what is claimed for it
    assert (i >= 0).all() and (i < SAMPLE).all()
    gathered = sims.gather(1, i)
    err = (gathered - s).abs().max().item()
    print("pre_tiles=%d max |fp32 score - returned score| = %.3g" % (pre_tiles, err))
    assert torch.allclose(gathered, s, atol=1e-4), err
    # and the floor is the 8th of them
    floor = torch.from_numpy(_dec_f32(thr.cpu().numpy().view(np.uint32))).to(s.device)
    assert torch.equal(floor.view(torch.int32), s[:, 7].contiguous().view(torch.int32))


def _dec_f32(u32):
    """The kernels' order-preserving u32 -> f32 decoding (dec_f32)."""
    u = np.asarray(u32).astype(np.uint32)
    b = np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u)
    return b.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("pre_tiles", [8, 16, 32, 64])
def test_floors_do_not_depend_on_the_geometry(floors_300, pre_tiles):
    """Grids 64 / 32 / 16 / 8 over three row tiles, the last one partial
    (pre_tiles = 8 repeats the reference launch: run to run determinism)."""
    _check_floors(floors_300, pre_tiles)


def test_default_argument_is_one_block_per_chunk(floors_300):
    from kakveda_amd.ops import _require_ext

    q, c, _, (s8, i8, thr8) = floors_300
    s, i, thr = _require_ext().floor_probe(q, c, PREGQ, k=8)
    torch.cuda.synchronize()
    assert torch.equal(s.view(torch.int32), s8.view(torch.int32))
    assert torch.equal(i, i8) and torch.equal(thr, thr8)


def test_floors_on_the_xcd_remapped_branch(floors_2048):
    """32 x 16 = 512 blocks: grid.x % 8 == 0 and a full round, so the kernel
    takes its XCD remap, as the plan's geometry does at B = 2048."""
    _check_floors(floors_2048, 16)


@pytest.mark.parametrize("pre_tiles", [-8, 4, 12, 24, 128, 1 << 40])
def test_probe_refuses_a_size_that_does_not_fit(floors_300, pre_tiles):
    """64 chunks x 8 tiles: 24 does not divide them, 128 leaves a grid of 4."""
    from kakveda_amd.ops import _require_ext

    q, c, _, _ = floors_300
    ext = _require_ext()
    for probe in (ext.floor_probe, ext.emit_counts_probe):
        with pytest.raises(RuntimeError, match="pre_tiles"):
            probe(q, c, PREGQ, k=8, pre_tiles=pre_tiles)


def test_emit_counts_probe_takes_the_geometry(floors_300):
    """The same floors reach the emission kernel: equal per-row counts."""
    from kakveda_amd.ops import _require_ext

    q, c, _, (_, _, thr8) = floors_300
    ext = _require_ext()
    cc8, _, t8 = ext.emit_counts_probe(q, c, PREGQ, k=8)
    cc32, _, t32 = ext.emit_counts_probe(q, c, PREGQ, k=8, pre_tiles=32)
    torch.cuda.synchronize()
    assert torch.equal(t8, thr8) and torch.equal(t32, thr8)
    assert torch.equal(cc8, cc32) and int(cc8.min()) >= 8


# ---------------------------------------------------------------------------
# child processes: the plan's geometry against the forced one-block-per-chunk
# ---------------------------------------------------------------------------

E2E_B = 2048
FILT_B, FILT_N = 8, 70_000


def child_main(argv):
    """``python tests/test_gpu_prepass_geometry.py MODE OUT`` under the
    caller's KAKVEDA_* environment. e2e: cosine_topk at B = 2048, k = 5 and 8,
    at the smallest N with long prepass blocks and at twice that, each result
    judged against the fp32 product; filtered: one filtered B = 8 call; both
    save their outputs to OUT. refused: the call must raise a RuntimeError
    that names the knob."""
    sys.path.insert(0, ta.REPO)
    from kakveda_amd import ops

    mode, out = argv[0], argv[1]
    pc = ta.plan_constants()
    saved = {}
    if mode == "refused":
        q, c = gpu_unit(16, D, 1), gpu_unit(pc["MIN_N_EMIT"], D, 2)
        try:
            ops.cosine_topk(q, c, 5)
        except RuntimeError as exc:
            assert "KAKVEDA_KNN_PRE_TILES" in str(exc), str(exc)
            print("CHILD refused", flush=True)
            return 0
        print("CHILD not refused", flush=True)
        return 1
    if mode == "e2e":
        n0 = smallest_long_block_n(E2E_B, pc)
        q = gpu_unit(E2E_B, D, 7300)
        c_all = gpu_unit(2 * n0, D, 7301)
        for n in (n0, 2 * n0):
            c = c_all[:n]
            for k in (5, 8):
                print("CASE n=%d k=%d" % (n, k), flush=True)
                s, i = ops.cosine_topk(q, c, k)
                torch.cuda.synchronize()
                for r0 in range(0, E2E_B, 256):
                    sims = (q[r0 : r0 + 256].float() @ c.float().t()).double()
                    ta.check_topk(s[r0 : r0 + 256], i[r0 : r0 + 256], sims, k, D,
                                  what="n=%d k=%d rows %d.." % (n, k, r0))
                saved["n=%d k=%d" % (n, k)] = (s.cpu(), i.cpu())
    else:
        assert mode == "filtered"
        q = gpu_unit(FILT_B, D, 7400)
        c = gpu_unit(FILT_N, D, 7401)
        g = torch.Generator(device=DEV).manual_seed(7402)
        labels = torch.randint(0, 4, (FILT_N,), generator=g, device=DEV, dtype=torch.int32)
        want = torch.tensor([0, 1, 2, 3, -1, 0, 1, -1], device=DEV, dtype=torch.int32)
        s, i = ops.cosine_topk_filtered(q, c, labels, want, 5)
        torch.cuda.synchronize()
        sims = (q.float() @ c.float().t()).double()
        elig = (want[:, None] < 0) | (labels[None, :] == want[:, None])
        ta.check_topk(s, i, sims, 5, D, eligible=elig, what="filtered")
        saved["filtered"] = (s.cpu(), i.cpu())
    torch.save(saved, out)
    print("CHILD ok", flush=True)
    return 0


def _child(env_set, mode, out):
    env = dict(os.environ)
    for name in list(env):
        if name.startswith("KAKVEDA_KNN_") or name == "KAKVEDA_SMALLB":
            env.pop(name)
    env.update(env_set)
    return subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(out)],
                          env=env, capture_output=True, text=True, timeout=300)


def _ok(r):
    assert r.returncode == 0 and "CHILD ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
    return r


def _same_outputs(a, b):
    assert sorted(a) == sorted(b) and a
    for name, (scores, idx) in a.items():
        assert torch.equal(scores.view(torch.int32), b[name][0].view(torch.int32)), name
        assert torch.equal(idx, b[name][1]), name


def test_end_to_end_equals_one_block_per_chunk(tmp_path):
    pc = ta.plan_constants()
    n0 = smallest_long_block_n(E2E_B, pc)
    preg, grid, tiles = planned_prepass(E2E_B, n0, pc)
    assert tiles > pc["PRE_TILES"] and grid * tiles == preg * pc["PRE_TILES"]
    # at n0 the sample is the corpus; at 2 * n0 the seeded main launch scans
    # the other half under the same prepass geometry
    assert preg * pc["PRE_TILES"] * pc["BN"] == n0
    assert planned_prepass(E2E_B, 2 * n0, pc) == (preg, grid, tiles)

    debug = {"KAKVEDA_KNN_EMIT_DEBUG": "1"}
    rule = _ok(_child(debug, "e2e", tmp_path / "rule.pt"))
    forced = _ok(_child(dict(debug, KAKVEDA_KNN_PRE_TILES="8"), "e2e", tmp_path / "forced.pt"))
    _same_outputs(torch.load(tmp_path / "rule.pt"), torch.load(tmp_path / "forced.pt"))

    def lines(r, prefix):
        return [l for l in r.stdout.splitlines() if l.startswith(prefix)]

    # the geometry each child ran ...
    assert set(lines(rule, "emit: prepass")) == {
        "emit: prepass pre_grid=%d pre_tiles=%d" % (grid, tiles)}
    assert set(lines(forced, "emit: prepass")) == {
        "emit: prepass pre_grid=%d pre_tiles=%d" % (preg, pc["PRE_TILES"])}
    # ... and the same emission counts under both, call for call
    counts = lines(rule, "emit: rows=")
    assert len(counts) == 4 and all(re.search(r"max=\d+ mean=[\d.]+", l) for l in counts)
    assert counts == lines(forced, "emit: rows=")


def test_filtered_small_batch_forced_to_long_blocks(tmp_path):
    """By the rule a filtered B = 8 request keeps preg x 8 (one row tile never
    fills a round); forced to 16 tiles per block (144 chunks -> 72 blocks)
    the Filter still reaches the prepass and the result is the same."""
    debug = {"KAKVEDA_KNN_EMIT_DEBUG": "1"}
    rule = _ok(_child(debug, "filtered", tmp_path / "rule.pt"))
    forced = _ok(_child(dict(debug, KAKVEDA_KNN_PRE_TILES="16"), "filtered", tmp_path / "forced.pt"))
    assert "emit: prepass pre_grid=144 pre_tiles=8" in rule.stdout
    assert "emit: prepass pre_grid=72 pre_tiles=16" in forced.stdout
    _same_outputs(torch.load(tmp_path / "rule.pt"), torch.load(tmp_path / "forced.pt"))


@pytest.mark.parametrize("value", ["12", "x", "24"])
def test_bad_knob_value_is_refused(tmp_path, value):
    """12 and x are no sizes at all; 24 is one, but the request's sample of
    64 x 8 tiles does not divide by it. Either way a RuntimeError naming the
    knob, raised by the plan, ahead of every allocation and launch."""
    r = _child({"KAKVEDA_KNN_PRE_TILES": value}, "refused", tmp_path / "none.pt")
    assert r.returncode == 0 and "CHILD refused" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1:]))
