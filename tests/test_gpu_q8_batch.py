"""GPU tests of the batched int8 screen (``ops.cosine_topk_q8`` at batch size:
cosine_topk_screen8p_i8 + emit_bin + q8_rescore_mfma + the unchanged merge).

The contract is bit equality with the bf16 search: every test of the whole
path is ``torch.equal`` on scores and ids against ``ops.cosine_topk`` on the
same inputs. N = 70,001 is the smallest emission corpus with a partial last
256-column tile; D = 128 / 256 / 768 are one, two and six K windows; B = 257
and 300 are two row tiles with a partial second, B = 512 two full ones.
``batch_min_b=1, batch_min_rows=1`` take the gates (``ops.Q8_BATCH_MIN_B`` and
``ops.Q8_BATCH_MIN_ROWS``, speed thresholds) out of the way; the gating itself
is tested at the end.
"""

import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_adversarial as ta  # noqa: E402

from kakveda_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 70_001
DIMS = (128, 256, 768)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BASES = {}


def mirror_of(c, n=None):
    """(codes, meta, cnorm) of the first n rows of c."""
    n = c.shape[0] if n is None else n
    codes, meta = ops.new_q8_mirror(c.shape[0], c.shape[1], c.device)
    cn = ops.new_q8_cnorm(c.device)
    ops.quantize_rows_q8(c[:n], codes, meta, 0, cn)
    return codes, meta, cn


def base_for(d):
    """70,001 unit rows per D with their mirror, shared and never modified."""
    if d not in _BASES:
        c = ta.rand_unit(N, d, seed=3).to(DEV)
        _BASES[d] = (c,) + mirror_of(c)
    return _BASES[d]


def fallbacks():
    return ops.q8_overflow_fallbacks, ops.q8_degenerate_fallbacks


def both(q, c, codes, meta, cn, k, n=None, **kw):
    got = ops.cosine_topk_q8(q, c, codes, meta, k, valid_n=n, cnorm=cn, batch_min_b=1, batch_min_rows=1, **kw)
    want = ops.cosine_topk(q, c, k, valid_n=n)
    torch.cuda.synchronize()
    return got, want


def assert_same(got, want, what):
    assert torch.equal(got[0], want[0]), (what, "scores")
    assert torch.equal(got[1], want[1]), (what, "ids")


# ---------------------------------------------------------------------------
# equality with the bf16 search
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [257, 300, 512])
@pytest.mark.parametrize("d", DIMS)
def test_equals_bf16_search_on_random_rows(d, B):
    c, codes, meta, cn = base_for(d)
    q = ta.rand_unit(B, d, seed=100 + B).to(DEV)
    before = fallbacks()
    for k in (2, 5, 8):
        got, want = both(q, c, codes, meta, cn, k)
        assert_same(got, want, (d, B, k))
    assert fallbacks() == before  # the int8 path answered, not the fallback


def adversarial_cases(d):
    pc = ta.plan_constants()
    return [
        ta.dup_case(d, N, 300, 5, 8, "contig", pc, 500),
        ta.dup_case(d, N, 300, 5, 9, "scatter", pc, 510),
        ta.dup_case(d, N, 257, 8, 24, "scatter", pc, 520),
        ta.dup_case(d, N, 300, 2, 4, "contig", pc, 530),
        ta.neardup_case(d, N, 300, pc, 540),
        ta.poison_case(d, N - 300, 300, 5, 550),  # masked columns past valid_n
    ]


@pytest.mark.parametrize("d", DIMS)
def test_equals_bf16_search_on_ties_duplicates_and_masked_columns(d):
    base = base_for(d)[0]
    before = fallbacks()
    for case in adversarial_cases(d):
        c = ta.materialise(case, base)
        codes, meta, cn = mirror_of(c, case.n)
        q = case.q.to(DEV)
        got, want = both(q, c, codes, meta, cn, case.k, n=case.n)
        assert_same(got, want, case.name)
        sims64 = q.double() @ c[: case.n].double().t()
        ta.judge(case, got[0], got[1], sims64)
    assert fallbacks() == before


def test_zero_query_sends_the_batch_to_the_bf16_search():
    d = 768
    c, codes, meta, cn = base_for(d)
    case = ta.zero_query_case(d, N, 300, 5, 560)
    q = case.q.to(DEV)
    over, degen = fallbacks()
    got = ops.cosine_topk_q8(q, c, codes, meta, 5, cnorm=cn, batch_min_b=1, batch_min_rows=1)
    torch.cuda.synchronize()
    assert fallbacks() == (over, degen + 1)
    sims64 = q.double() @ c.double().t()
    ta.judge(case, got[0], got[1], sims64)


# ---------------------------------------------------------------------------
# the screen's candidate lists (probe)
# ---------------------------------------------------------------------------

def pair_keys(entries, counts, first=None):
    """Sorted int64 keys row * N + column of the entries [first, counts) of
    every row of a candidate buffer, and the entries in that order."""
    B, cap = entries.shape
    pos = torch.arange(cap, device=entries.device)[None, :]
    live = pos < counts.long().clamp(max=cap)[:, None]
    if first is not None:
        live &= pos >= first.long()[:, None]
    rows = torch.arange(B, device=entries.device)[:, None].expand(B, cap)[live]
    ent = entries[live]
    _s, cols = ops.q8_unpack(ent)
    keys = rows * N + cols
    order = torch.argsort(keys)
    return keys[order], ent[order]


@pytest.fixture(scope="module")
def probe768():
    c, codes, meta, cn = base_for(768)
    q = ta.rand_unit(300, 768, seed=700).to(DEV)
    pr = ops.q8_screen_probe(q, c, codes, meta, cn, 5)
    torch.cuda.synchronize()
    return q, pr


def test_candidates_are_a_superset_of_the_bf16_kernels(probe768):
    q, pr = probe768
    c, codes, meta, cn = base_for(768)
    assert int(pr["counts"].max()) <= pr["before"].shape[1]
    keys, _ = pair_keys(pr["before"], pr["counts"])
    assert keys.numel() == int(pr["counts"].sum()) and keys.unique().numel() == keys.numel()

    # (a) the mode-9 bf16 kernel under the same floors: what it emits is what
    # reaches the floor in ops.cosine_topk's own arithmetic
    preg = 72  # the plan's sample at B = 300, N = 70,001: the whole corpus
    cnt16, cand16, thr16 = ops._require_ext().emit_counts_probe(q, c, preg, 8, 0)
    torch.cuda.synchronize()
    floors16 = ops._dec_f32(thr16.long() & 0xFFFFFFFF)
    assert torch.equal(floors16, pr["floors"])
    keys16, _ = pair_keys(cand16, cnt16)
    assert keys16.numel() >= 8 * 300
    assert bool(torch.isin(keys16, keys).all())

    # (b) fp32 torch: a score that clears the floor by the D * 2^-22 slack
    # reaches it under any fp32 summation order
    sims = q.float() @ c.float().t()
    need = (sims >= (pr["floors"] + 768 * 2.0 ** -22)[:, None]).nonzero()
    # not vacuous: the floor is the row's 8th best, and most of the seven
    # above it clear it by more than the slack (1.8e-4)
    assert need.shape[0] >= 4 * 300
    assert bool(torch.isin(need[:, 0] * N + need[:, 1], keys).all())


def test_candidates_equal_the_torch_screen_reference(probe768):
    q, pr = probe768
    c, codes, meta, cn = base_for(768)
    qcodes, T_ref, kappa_ref, degenerate = ops.q8_screen_params_ref(q, pr["floors"], cn)
    assert degenerate == 0
    # T and kappa: the same fp32 formulas, up to fused multiply-adds
    T, kappa = pr["T"].cpu(), pr["kappa"].cpu()
    assert bool(((T - T_ref).abs() <= T_ref.abs() * 2.0 ** -21).all())
    assert bool(((kappa - kappa_ref).abs() <= kappa_ref.abs() * 2.0 ** -22).all())
    mask, near = ops.q8_screen_mask_ref(qcodes, codes, meta, pr["T"], pr["kappa"], N, band=True)
    keys, _ = pair_keys(pr["before"], pr["counts"])
    dev_mask = torch.zeros_like(mask).view(-1)
    dev_mask[keys] = True
    dev_mask = dev_mask.view_as(mask)
    n_cand, n_near = int(mask.sum()), int(near.sum())
    print("candidates %d (%.1f per row), boundary pairs %d" % (n_cand, n_cand / 300, n_near))
    assert n_near < 1e-3 * n_cand
    assert int(((dev_mask != mask) & ~near).sum()) == 0


def test_rescored_scores_are_the_bf16_kernels_bits(probe768):
    q, pr = probe768
    c, codes, meta, cn = base_for(768)
    # a looser floor (an 8-chunk sample) makes the bf16 kernel emit more pairs
    cnt16, cand16, _thr = ops._require_ext().emit_counts_probe(q, c, 8, 8, 0)
    torch.cuda.synchronize()
    assert int(cnt16.max()) <= cand16.shape[1]
    keys16, ent16 = pair_keys(cand16, cnt16)
    keys, ent = pair_keys(pr["after"], pr["counts"], pr["first"])
    at = torch.searchsorted(keys16, keys).clamp(max=keys16.numel() - 1)
    hit = keys16[at] == keys
    assert int(hit.sum()) >= 2000
    # whole entries: the score word bit for bit, and the column
    assert torch.equal(ent[hit], ent16[at[hit]])
    # and the rescore changed every score word it was meant to
    _k, ent_b = pair_keys(pr["before"], pr["counts"], pr["first"])
    assert torch.equal(ent_b & 0xFFFFFFFF, ent & 0xFFFFFFFF)


# ---------------------------------------------------------------------------
# overflow, gating
# ---------------------------------------------------------------------------

def test_overflow_falls_back_to_the_bf16_answer():
    d = 768
    base = base_for(d)[0]
    q = ta.rand_unit(300, d, seed=800)
    g = torch.Generator().manual_seed(801)
    # 1,500 near-duplicates (cosine 0.9) of query row 7, scattered
    dups = ta.near_rows(q[7:8].expand(1500, d).contiguous(), g, cosines=[0.9])[:, 0]
    pos = torch.randperm(N, generator=g)[:1500]
    c = base.clone()
    c[pos.to(DEV)] = dups.to(DEV)
    codes, meta, cn = mirror_of(c)
    q = q.to(DEV)
    over, degen = fallbacks()
    got, want = both(q, c, codes, meta, cn, 5, cap=1024)
    assert fallbacks() == (over + 1, degen)
    assert_same(got, want, "overflow")
    # with the default capacity the same batch is answered by the int8 path
    got, want = both(q, c, codes, meta, cn, 5)
    assert fallbacks() == (over + 1, degen)
    assert_same(got, want, "no overflow")


def test_filtered_request_runs_the_bf16_path():
    d = 768
    c, codes, meta, cn = base_for(d)
    q = ta.rand_unit(300, d, seed=810).to(DEV)
    labels = (torch.arange(N, device=DEV) % 3).to(torch.int32)
    want = torch.full((300,), 1, dtype=torch.int32, device=DEV)
    ext = ops._require_ext()
    s, i, fb, counts = ext.cosine_topk_q8(q, c, codes, meta, 5, N, labels=labels,
                                          want=want, cnorm=cn, batch_min_b=1)
    s0, i0 = ext.cosine_topk_filtered(q, c, labels, want, 5, N)
    torch.cuda.synchronize()
    assert fb == 0 and counts.numel() == 0  # no int8 stage ran
    assert torch.equal(s, s0) and torch.equal(i, i0)
    # the unfiltered request does take it
    _s, _i, fb, counts = ext.cosine_topk_q8(q, c, codes, meta, 5, N, cnorm=cn, batch_min_b=1)
    assert fb == 0 and counts.numel() == 300
    # and a batch below the gate does not
    _s, _i, fb, counts = ext.cosine_topk_q8(q, c, codes, meta, 5, N, cnorm=cn, batch_min_b=301)
    assert fb == 0 and counts.numel() == 0


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
s, i, fb, counts = ops._require_ext().cosine_topk_q8(q, c, codes, meta, 5, 70001, cnorm=cn, batch_min_b=1)
s0, i0 = ops.cosine_topk(q, c, 5)
torch.cuda.synchronize()
assert torch.equal(s, s0) and torch.equal(i, i0)
print("counts", counts.numel(), "in_plan", ops.q8_batch_in_plan(300, 70001, 5, 128, False, 1, 1))
"""


@pytest.mark.parametrize("value,ran", [("0", False), ("1", True)])
def test_env_knob_in_a_fresh_process(value, ran):
    env = dict(os.environ, KAKVEDA_Q8_BATCH=value)
    out = subprocess.run([sys.executable, "-c", _CHILD % REPO], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert ("counts %d in_plan %s" % (300 if ran else 0, ran)) in out.stdout


def test_env_knob_rejects_other_values():
    env = dict(os.environ, KAKVEDA_Q8_BATCH="2")
    out = subprocess.run([sys.executable, "-c", _CHILD % REPO], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert "KAKVEDA_Q8_BATCH" in out.stdout + out.stderr
