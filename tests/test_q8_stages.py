"""CPU check that raising the int8 screen's floors between stages stays exact
(q8_plan.h "Staged floors"), simulated in torch (tests/q8_stage_ref.py) with
``ops.q8_screen_mask_ref`` and ``ops.quantize_rows_q8_ref`` on a few thousand
rows: for k = 1, 5 and 8 the seeds plus the staged candidates hold the exact
top-k, and per query the staged candidates are a subset of the single
launch's. The corpus carries copies of a query's best row on both sides of
every stage boundary, and the unseeded variant has queries that hold fewer
than k entries at a refresh.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_stage_ref as sr  # noqa: E402
import topk_adversarial as ta  # noqa: E402

from kakveda_amd import ops  # noqa: E402

D = 128
N = 4099
B = 24
SAMPLE = 1024
BOUNDS = [SAMPLE, 1600, 2560, N]  # ratio 1.6 a stage, as the plan's are


def _mirror(c):
    codes, meta = ops.new_q8_mirror(c.shape[0], D, "cpu")
    ops.quantize_rows_q8_ref(c, codes, meta)
    return codes, meta, ops.q8_cnorm_ref(c)


@pytest.fixture(scope="module")
def world():
    c = ta.rand_unit(N, D, seed=11)
    q = ta.rand_unit(B, D, seed=12)
    # query 3's best row, bit-identical, on both sides of each boundary, and
    # of the sample's end; query 5's near-duplicates likewise
    for b in BOUNDS[:-1]:
        c[b - 1] = q[3]
        c[b] = q[3]
    g = torch.Generator().manual_seed(13)
    near = ta.near_rows(q[5:6], g)[0]  # cosines 0.95 .. 0.60
    for j, pos in enumerate((1022, 1025, 1598, 1601, 2558, 2561, 4098, 0)):
        c[pos] = near[j]
    return (q, c) + _mirror(c)


def _holds_topk(sims, held, k):
    """Every column scoring above the row's k-th best is held, and at least k
    held columns score at least the k-th best (ties may stand in)."""
    kth = torch.topk(sims, k, dim=1).values[:, -1:]
    above = sims > kth
    assert bool((held | ~above).all())
    assert bool(((held & (sims >= kth)).sum(dim=1) >= k).all())


@pytest.mark.parametrize("k", [1, 5, 8])
def test_staged_candidates_hold_the_topk_and_shrink(world, k):
    q, c, codes, meta, cn = world
    one = sr.simulate(q, c, codes, meta, cn, k, [SAMPLE, N], SAMPLE)
    st = sr.simulate(q, c, codes, meta, cn, k, BOUNDS, SAMPLE)
    _holds_topk(one["sims"], one["cand"] | one["seeds"], k)
    _holds_topk(st["sims"], st["cand"] | st["seeds"], k)
    # per query a subset of the single launch's, and fewer in all
    assert bool((one["cand"] | ~st["cand"]).all())
    assert int(st["cand"].sum()) < int(one["cand"].sum())
    # the floors only rise, and the first stage screens against the prepass's
    assert torch.equal(st["floors"][0], one["floors"][0])
    for a, b in zip(st["floors"], st["floors"][1:]):
        assert bool((b >= a).all())
    assert bool((st["floors"][-1] > st["floors"][0]).any())
    # the planted copies behind the sample are all candidates: they tie with
    # (or are) the row's best, whatever the floor has risen to
    for b in BOUNDS[1:-1]:
        assert bool(st["cand"][3, b - 1]) and bool(st["cand"][3, b])


@pytest.mark.parametrize("k", [5, 8])
def test_unseeded_stages_with_rows_short_of_k_entries(world, k):
    """The sample covers the corpus: nothing is seeded, the stages partition
    every row, and the floor (the corpus's 8th best) leaves most queries with
    fewer than k entries after the first stage: those raise nothing."""
    q, c, codes, meta, cn = world
    bounds = [0, 1366, 2732, N]
    one = sr.simulate(q, c, codes, meta, cn, k, [0, N], N)
    st = sr.simulate(q, c, codes, meta, cn, k, bounds, N)
    assert bool(st["short"][0].any())
    keep = st["short"][0]
    assert torch.equal(st["floors"][1][keep], st["floors"][0][keep])
    _holds_topk(st["sims"], st["cand"], k)
    assert bool((one["cand"] | ~st["cand"]).all())


def test_reference_counts_fall_at_the_gpu_tests_shape():
    """The shape and seeds of tests/test_gpu_q8_stages.py's count check
    (N = 300,001, D = 128, B = 300, k = 5: 960 sampled tiles of 1,172): three
    geometric stages pass strictly fewer candidates than one launch."""
    n, b = 300_001, 300
    c = ta.rand_unit(n, D, seed=21)
    q = ta.rand_unit(b, D, seed=22)
    codes, meta = ops.new_q8_mirror(n, D, "cpu")
    ops.quantize_rows_q8_ref(c, codes, meta)
    cn = ops.q8_cnorm_ref(c)
    tiles = sr.geometric_bounds(960, 1172, 3)
    bounds = [t * 256 for t in tiles]
    one = sr.simulate(q, c, codes, meta, cn, 5, [bounds[0], n], bounds[0])
    st = sr.simulate(q, c, codes, meta, cn, 5, bounds, bounds[0])
    n1, n3 = int(one["cand"].sum()), int(st["cand"].sum())
    print("candidates: one launch %d, three stages %d" % (n1, n3))
    assert bool((one["cand"] | ~st["cand"]).all())
    assert n3 < n1
