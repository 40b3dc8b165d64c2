"""GPU tests of the staged int8 screen (``ops.cosine_topk_q8(..., stages=n)``:
the screen's main launch cut into n stages with the floors raised between
them, knn_plan.h plan_q8_stages and q8_plan.h "Staged floors").

The contract is unchanged: every check of the whole path is ``torch.equal`` on
scores and ids against ``ops.cosine_topk`` with ``batch_min_b=1,
batch_min_rows=1``. N = 70,001 is the smallest emission corpus with a partial
last tile: the sample covers it, nothing is skipped, the stages partition the
whole launch, and stages end in padded chunks. N = 300,001
(D = 128, B = 300) is the smallest shape whose main launch starts behind the
sample (960 of 1,172 tiles), so the lists are seeded and a floor really rises
between stages. Stage boundaries are read from ``ops.q8_stage_plan``.
"""

import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_stage_ref as sr  # noqa: E402
import topk_adversarial as ta  # noqa: E402

from kakveda_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 70_001
N_BIG = 300_001
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BASES = {}


def mirror_of(c, n=None):
    n = c.shape[0] if n is None else n
    codes, meta = ops.new_q8_mirror(c.shape[0], c.shape[1], c.device)
    cn = ops.new_q8_cnorm(c.device)
    ops.quantize_rows_q8(c[:n], codes, meta, 0, cn)
    return codes, meta, cn


def base_for(n, d):
    """Unit rows with their mirror per (N, D), shared and never modified."""
    if (n, d) not in _BASES:
        c = ta.rand_unit(n, d, seed=21 if n == N_BIG else 3).to(DEV)
        _BASES[(n, d)] = (c,) + mirror_of(c)
    return _BASES[(n, d)]


def fallbacks():
    return ops.q8_overflow_fallbacks, ops.q8_degenerate_fallbacks


def q8(q, c, codes, meta, cn, k, n=None, **kw):
    return ops.cosine_topk_q8(q, c, codes, meta, k, valid_n=n, cnorm=cn,
                              batch_min_b=1, batch_min_rows=1, **kw)


def assert_same(got, want, what):
    assert torch.equal(got[0], want[0]), (what, "scores")
    assert torch.equal(got[1], want[1]), (what, "ids")


# ---------------------------------------------------------------------------
# equality with the bf16 search
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [257, 300])
@pytest.mark.parametrize("d", [128, 768])
def test_stages_partition_the_whole_launch(d, B):
    c, codes, meta, cn = base_for(N, d)
    q = ta.rand_unit(B, d, seed=100 + B).to(DEV)
    for stages in (2, 3, 4):
        plan = ops.q8_stage_plan(B, N, 5, stages)
        assert plan["first"][0] == 0 and plan["first"][-1] == -(-N // 256)
        assert len(plan["first"]) == stages + 1
        # some stage's grid ends in padded chunks, which hold no tile
        real = [-(-(b - a) // ct) for a, b, ct in
                zip(plan["first"], plan["first"][1:], plan["chunk_tiles"])]
        assert any(r < nc for r, nc in zip(real, plan["nchunks"]))
    before = fallbacks()
    for k in (2, 5, 8):
        want = ops.cosine_topk(q, c, k)
        for stages in (2, 3, 4):
            got = q8(q, c, codes, meta, cn, k, stages=stages)
            assert_same(got, want, (d, B, k, stages))
    assert fallbacks() == before  # the int8 path answered, not the fallback


@pytest.fixture(scope="module")
def big():
    c, codes, meta, cn = base_for(N_BIG, 128)
    q = ta.rand_unit(300, 128, seed=22).to(DEV)
    return q, c, codes, meta, cn


def test_seeded_stages_equal_the_bf16_search(big):
    q, c, codes, meta, cn = big
    assert ops.q8_stage_plan(300, N_BIG, 5, 3)["first"][0] == 960  # seeds
    assert ops.q8_stage_plan(300, N_BIG, 5)["first"] == [960, 1172]  # the rule: one stage
    before = fallbacks()
    for k in (2, 5, 8):
        want = ops.cosine_topk(q, c, k)
        for stages in (1, 3):
            assert_same(q8(q, c, codes, meta, cn, k, stages=stages), want, (k, stages))
    assert fallbacks() == before


def test_counts_fall_with_stages(big):
    q, c, codes, meta, cn = big
    k = 5
    # the torch reference under the plan's own boundaries: strictly fewer
    first = ops.q8_stage_plan(300, N_BIG, k, 3)["first"]
    bounds = [t * 256 for t in first]
    one = sr.simulate(q, c, codes, meta, cn, k, [bounds[0], N_BIG], bounds[0])
    st = sr.simulate(q, c, codes, meta, cn, k, bounds, bounds[0])
    assert int(st["cand"].sum()) < int(one["cand"].sum())
    _s, _i, c1 = q8(q, c, codes, meta, cn, k, stages=1, return_counts=True)
    _s, _i, c3 = q8(q, c, codes, meta, cn, k, stages=3, return_counts=True)
    print("candidates: one launch %d (reference %d), three stages %d (reference %d)" % (
        int(c1.sum()) - 8 * 300, int(one["cand"].sum()),
        int(c3.sum()) - 8 * 300, int(st["cand"].sum())))
    assert bool((c3 <= c1).all())
    assert int(c3.sum()) < int(c1.sum())
    # every query keeps its 8 seeds and at least the k best
    assert int(c3.min()) >= 8
    # where nothing is skipped: per query no more than the single launch
    c70, codes70, meta70, cn70 = base_for(N, 768)
    q70 = ta.rand_unit(300, 768, seed=400).to(DEV)
    _s, _i, a1 = q8(q70, c70, codes70, meta70, cn70, k, stages=1, return_counts=True)
    _s, _i, a3 = q8(q70, c70, codes70, meta70, cn70, k, stages=3, return_counts=True)
    assert bool((a3 <= a1).all()) and int(a3.min()) >= k


# ---------------------------------------------------------------------------
# ties, duplicates, masked columns, copies across a stage boundary
# ---------------------------------------------------------------------------

def boundary_case(d, n, B, k, stages, seed):
    """Bit-identical copies of query row B-1 on both sides of the sample's end
    and of every stage boundary of the plan for (B, n, k, stages)."""
    first = ops.q8_stage_plan(B, n, k, stages)["first"]
    pos = []
    for t in first[:-1]:
        pos += [p for p in (t * 256 - 1, t * 256) if 0 <= p < n]
    q = ta.rand_unit(B, d, seed + 1)
    row = ta.rand_unit(1, d, seed + 2)
    q[B - 1] = row[0]
    case = ta.Case(
        name="boundary[|S|=%d,k=%d,B=%d,N=%d,stages=%d]" % (len(pos), k, B, n, stages),
        q=q, n=n, k=k, plant_pos=torch.tensor(pos, dtype=torch.int64),
        plant_rows=row.expand(len(pos), d).contiguous(),
    )
    if len(pos) >= k:
        case.within[B - 1] = pos
    else:
        case.contains[B - 1] = pos
    return case


def run_case(case, base, stages):
    c = ta.materialise(case, base)
    codes, meta, cn = mirror_of(c, case.n)
    q = case.q.to(DEV)
    got = q8(q, c, codes, meta, cn, case.k, n=case.n, stages=stages)
    want = ops.cosine_topk(q, c, case.k, valid_n=case.n)
    torch.cuda.synchronize()
    assert_same(got, want, case.name)
    sims64 = q.double() @ c[: case.n].double().t()
    ta.judge(case, got[0], got[1], sims64)


@pytest.mark.parametrize("d", [128, 768])
def test_ties_duplicates_and_masked_columns_under_stages(d):
    pc = ta.plan_constants()
    base = base_for(N, d)[0]
    before = fallbacks()
    cases = [
        (ta.dup_case(d, N, 300, 5, 8, "contig", pc, 500), 3),
        (ta.dup_case(d, N, 300, 5, 9, "scatter", pc, 510), 4),
        (ta.dup_case(d, N, 257, 8, 24, "scatter", pc, 520), 3),
        (ta.dup_case(d, N, 300, 2, 4, "contig", pc, 530), 2),
        (ta.neardup_case(d, N, 300, pc, 540), 3),
        (ta.poison_case(d, N - 300, 300, 5, 550), 3),  # masked columns past valid_n
        (boundary_case(d, N, 300, 5, 4, 560), 4),  # 7 copies >= k
        (boundary_case(d, N, 300, 8, 3, 570), 3),  # 5 copies < k
    ]
    for case, stages in cases:
        run_case(case, base, stages)
    assert fallbacks() == before


def test_copies_across_the_sample_and_the_stage_boundaries(big):
    base = big[1]
    before = fallbacks()
    for k in (5, 8):  # 6 copies: one seeded, five behind the sample
        run_case(boundary_case(128, N_BIG, 300, k, 3, 580 + k), base, 3)
    pc = ta.plan_constants()
    run_case(ta.dup_case(128, N_BIG, 300, 5, 9, "scatter", pc, 590), base, 3)
    run_case(ta.neardup_case(128, N_BIG, 300, pc, 600), base, 3)
    assert fallbacks() == before


# ---------------------------------------------------------------------------
# overflow, the knob
# ---------------------------------------------------------------------------

def test_overflow_under_stages_falls_back_to_the_bf16_answer():
    d = 768
    base = base_for(N, d)[0]
    q = ta.rand_unit(300, d, seed=800)
    g = torch.Generator().manual_seed(801)
    # 1,500 near-duplicates (cosine 0.9) of query row 7, scattered over every stage
    dups = ta.near_rows(q[7:8].expand(1500, d).contiguous(), g, cosines=[0.9])[:, 0]
    pos = torch.randperm(N, generator=g)[:1500]
    c = base.clone()
    c[pos.to(DEV)] = dups.to(DEV)
    codes, meta, cn = mirror_of(c)
    q = q.to(DEV)
    want = ops.cosine_topk(q, c, 5)
    over, degen = fallbacks()
    assert_same(q8(q, c, codes, meta, cn, 5, cap=1024, stages=3), want, "overflow")
    assert fallbacks() == (over + 1, degen)
    # a capacity the first stage alone overflows: the refresh raises nothing there
    assert_same(q8(q, c, codes, meta, cn, 5, cap=256, stages=3), want, "early overflow")
    assert fallbacks() == (over + 2, degen)
    assert_same(q8(q, c, codes, meta, cn, 5, stages=3), want, "no overflow")
    assert fallbacks() == (over + 2, degen)


def test_stages_argument_is_checked():
    c, codes, meta, cn = base_for(N, 128)
    q = ta.rand_unit(300, 128, seed=810).to(DEV)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError):
            q8(q, c, codes, meta, cn, 5, stages=bad)


_CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from kakveda_amd import ops
g = torch.Generator().manual_seed(5)
def unit(n):
    x = torch.randn(n, 128, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16).to("cuda:0")
c, q = unit(70001), unit(300)
codes, meta = ops.new_q8_mirror(70001, 128, c.device)
cn = ops.new_q8_cnorm(c.device)
ops.quantize_rows_q8(c, codes, meta, 0, cn)
s, i = ops.cosine_topk_q8(q, c, codes, meta, 5, cnorm=cn, batch_min_b=1, batch_min_rows=1)
s0, i0 = ops.cosine_topk(q, c, 5)
torch.cuda.synchronize()
assert torch.equal(s, s0) and torch.equal(i, i0)
print("stages", len(ops.q8_stage_plan(300, 70001, 5)["first"]) - 1)
"""


def test_env_knob_in_a_fresh_process():
    env = dict(os.environ, KAKVEDA_Q8_STAGES="3")
    out = subprocess.run([sys.executable, "-c", _CHILD % REPO], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "stages 3" in out.stdout
    env = dict(os.environ, KAKVEDA_Q8_STAGES="three")
    out = subprocess.run([sys.executable, "-c", _CHILD % REPO], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert "KAKVEDA_Q8_STAGES" in out.stdout + out.stderr
