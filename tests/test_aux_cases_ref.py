"""CPU half of the exact tests of kmeans_update, kmeans_assign(_scored),
embedding_bag and l2normalize_.

Every case of tests/aux_cases.py goes through the plain-torch CPU fallbacks
of kakveda_amd.ops under the same oracles the HIP kernels face in
tests/test_gpu_aux_exact.py: the cases meet their exactness preconditions,
the fallbacks satisfy the oracles bit for bit (the derived bound, for
l2normalize_), and the checkers reject hand-broken results. Also pins the
row width at which kmeans_assign_scored leaves the dedicated kernel.
"""

import os
import re

import pytest
import torch

import aux_cases as ac
from kakveda_amd import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ASSIGN_DIMS = (64, 128, 192, 256, 320, 768, 1152)
ASSIGN_CS = (1, 16, 17, 63)
ASSIGN_NS = (1, 31, 255, 256, 257)
GRID_STRIDE_N = 2048 * 256 + 300
ROUTE_CS = (65, 200, 513)
NORM_DIMS = (8, 64, 520, 768, 1536)


# -- kmeans_update -------------------------------------------------------------

@pytest.mark.parametrize("C,D,N,bad,empty", ac.UPDATE_CASES)
def test_update_cases(C, D, N, bad, empty):
    case = ac.update_case(C, D, N, bad, empty)
    assert (case.n_dropped > 0) == (bad > 0) and (case.empty is not None) == empty
    sums, counts = ops.kmeans_update(case.points, case.assign, C)
    ac.check_update(case, sums, counts)


def test_update_cases_reach_the_paths_they_name():
    ppc = ac.update_chunk_points
    assert ppc(768, 20003) == 118  # 64 < 118 < 128: one unrolled pass, then the tail
    assert ppc(64, 150001) == 74
    assert ppc(128, 40000) == 40  # < 61: no lane reaches the unrolled pass
    assert ppc(64, 3) == 1 and ppc(64, 1) == 1 and ppc(192, 67) == 1
    replicas = {C <= 128 for C, *_ in ac.UPDATE_CASES}
    assert replicas == {True, False}
    for want_bad, want_empty in ((True, False), (False, True)):
        paths = {C <= 128 for C, _, _, bad, empty in ac.UPDATE_CASES
                 if (bad > 0) == want_bad and empty == want_empty}
        assert paths == {True, False}


def test_update_checker_rejects_one_dropped_point():
    case = ac.update_case(64, 128, 20003, 0.05, False)
    keep = torch.ones(case.points.shape[0], dtype=torch.bool)
    victim = int(((case.assign >= 0) & (case.assign < case.C)).nonzero()[-1])  # the last live point
    keep[victim] = False
    sums, counts = ops.kmeans_update(case.points[keep], case.assign[keep], case.C)
    with pytest.raises(AssertionError, match="count of cluster"):
        ac.check_update(case, sums, counts)
    with pytest.raises(AssertionError, match=r"sum\["):
        ac.check_update(case, sums, case.counts)
    # counting the dropped (-1 / C) points into a neighbour is seen too
    clamped = case.assign.clamp(0, case.C - 1)
    sums, counts = ops.kmeans_update(case.points, clamped, case.C)
    with pytest.raises(AssertionError):
        ac.check_update(case, sums, counts)


# -- kmeans_assign -------------------------------------------------------------

def _cpu_assign(case):
    return ops.kmeans_assign_scored(case.points, case.centroids)


@pytest.mark.parametrize("D", ASSIGN_DIMS)
def test_assign_dims(D):
    case = ac.assign_case(777, D, 64)
    assert case.tied_rows > 0
    ac.check_assign(case, *_cpu_assign(case), lowest_index=True)


@pytest.mark.parametrize("C", ASSIGN_CS)
def test_assign_centroid_counts(C):
    case = ac.assign_case(777, 128, C)
    ac.check_assign(case, *_cpu_assign(case), lowest_index=True)


@pytest.mark.parametrize("N", ASSIGN_NS)
def test_assign_point_counts(N):
    case = ac.assign_case(N, 64, 33)
    ac.check_assign(case, *_cpu_assign(case), lowest_index=True)


def test_assign_grid_stride_size():
    case = ac.assign_case(GRID_STRIDE_N, 64, 64, keep_sims=False)
    assert case.tied_rows > 1000
    ac.check_assign(case, *_cpu_assign(case), lowest_index=True)


def test_assign_all_negative():
    case = ac.assign_case(300, 128, 17, negative=True)
    assert float(case.score.max()) < 0
    ac.check_assign(case, *_cpu_assign(case), lowest_index=True)


@pytest.mark.parametrize("C", ROUTE_CS)
def test_assign_general_route_cases(C):
    case = ac.assign_case(66000, 64, C)
    score, idx = _cpu_assign(case)
    ac.check_assign(case, score, idx, lowest_index=False)
    ac.check_assign(case, score, idx, lowest_index=True)  # the CPU path does keep the lowest


def test_assign_wide_rows_case():
    case = ac.assign_case(1000, 1536, 8)
    ac.check_assign(case, *_cpu_assign(case), lowest_index=False)


def test_assign_checker_rejects_wrong_tie_and_wrong_score():
    case = ac.assign_case(777, 64, 64)
    score, idx = _cpu_assign(case)
    tied = (case.sims == case.score[:, None])
    r = int((tied.sum(dim=1) > 1).nonzero()[0])
    other = int(tied[r].nonzero()[-1])  # the highest tied column
    bad = idx.clone()
    bad[r] = other
    with pytest.raises(AssertionError, match="row %d returns %d, lowest argmax" % (r, other)):
        ac.check_assign(case, score, bad, lowest_index=True)
    ac.check_assign(case, score, bad, lowest_index=False)  # a tie member: fine where order is free
    loser = int((~tied[r]).nonzero()[0])
    bad[r] = loser
    with pytest.raises(AssertionError, match="row %d returns %d whose dot" % (r, loser)):
        ac.check_assign(case, score, bad, lowest_index=False)
    off = score.clone()
    off[5] += 1.0
    with pytest.raises(AssertionError, match="row 5 scores"):
        ac.check_assign(case, off, idx, lowest_index=True)


def test_assign_kernel_row_width_limit():
    """1152 is the widest row the dedicated kernel holds in LDS, 1216 the
    first refused (64 * assign_pitch(D) against 160 KiB); wider rows and
    C > 64 take the general route."""
    assert ops.assign_pitch(1152) == 2368 and 64 * 2368 <= 160 * 1024
    assert ops.assign_pitch(1216) == 2624 and 64 * 2624 > 160 * 1024
    assert ops.assign_kernel_fits(64, 1152) and ops.assign_kernel_fits(1, 64)
    assert not ops.assign_kernel_fits(64, 1216) and not ops.assign_kernel_fits(8, 1536)
    assert not ops.assign_kernel_fits(65, 64)
    assert ops.KMEANS_ASSIGN_MAX_D == 1152
    assert all(ops.assign_kernel_fits(64, d) == (d <= 1152) for d in range(64, 4097, 64))
    # the header the kernel is built from states the same rule
    text = open(os.path.join(REPO, "kakveda_amd", "ops", "hip", "kernels_impl.h")).read()
    m = re.search(r"int assign_pitch\(int D\) \{\s*return ([^;]+);", text)
    assert m, "assign_pitch not found in kernels_impl.h"
    expr = m.group(1)
    assert re.fullmatch(r"[D0-9+\-*%() ]+", expr), expr
    for d in range(64, 4097, 64):
        assert eval(expr, {"__builtins__": {}}, {"D": d}) == ops.assign_pitch(d), d
    assert re.search(r"constexpr int ASSIGN_LDS_BYTES = 160 \* 1024;", text)
    assert ops._ASSIGN_LDS_BYTES == 160 * 1024


# -- embedding_bag -------------------------------------------------------------

@pytest.mark.parametrize("B,L,D,V", ac.BAG_CASES)
def test_bag_cases(B, L, D, V):
    case = ac.bag_case(B, L, D, V)
    if B * L >= 20:
        assert case.n_ignored >= 2 and case.n_zero_w >= 1
        assert bool((case.idx == -1).any()) and bool((case.idx == V).any())
        assert bool((case.w[(case.idx < 0) | (case.idx >= V)] != 0).all())
    ac.check_bag(case, ops.embedding_bag(case.table, case.idx, case.w))


def test_bag_int64_indices():
    case = ac.bag_case(64, 48, 1000, 5000, torch.int64)
    assert case.idx.dtype == torch.int64
    ac.check_bag(case, ops.embedding_bag(case.table, case.idx, case.w))


def test_bag_checker_rejects_a_counted_out_of_range_index():
    """The mutation of the index rule, on the CPU: the -1 / V indices are
    replaced by in-range rows, as a kernel without the range test would read
    some row for them."""
    case = ac.bag_case(300, 128, 768, 7)
    V = case.table.shape[0]
    wrapped = torch.where((case.idx < 0) | (case.idx >= V), torch.zeros_like(case.idx), case.idx)
    with pytest.raises(AssertionError, match=r"out\["):
        ac.check_bag(case, ops.embedding_bag(case.table, wrapped, case.w))


# -- l2normalize_ ---------------------------------------------------------------

def _cpu_norm(case):
    t = case.x.clone()
    ops.l2normalize_(t, case.start, case.end)
    return t


@pytest.mark.parametrize("D", NORM_DIMS)
def test_norm_dims(D):
    case = ac.norm_case(37, D)
    assert case.zero_rows == (4,)
    ac.check_norm(case, _cpu_norm(case))


def test_norm_grid_stride_rows():
    ac.check_norm(ac.norm_case(8192 + 5, 64), _cpu_norm(ac.norm_case(8192 + 5, 64)))


def test_norm_row_window():
    case = ac.norm_case(9000, 64, 3, 8193)
    ac.check_norm(case, _cpu_norm(case))
    t = case.x.clone()
    ops.l2normalize_(t, 8, 8)
    ops.l2normalize_(t, 9, 3)
    assert torch.equal(t.view(torch.int16), case.x.view(torch.int16))


def test_norm_checker_rejects_two_bf16_ulps_and_a_touched_row():
    case = ac.norm_case(9000, 64, 3, 8193)
    good = _cpu_norm(case)
    bad = good.clone()
    r = 100
    d = int(good[r].float().abs().argmax())
    # two bf16 ulps: >= 1.5 ulp from the reference, and an ulp is >= 2^-8 relative
    bad.view(torch.int16)[r, d] += 2
    with pytest.raises(AssertionError, match=r"out\[100, %d\]" % d):
        ac.check_norm(case, bad)
    bad = good.clone()
    bad[8193, 0] = 0.5
    with pytest.raises(AssertionError, match="row 8193 outside the window changed"):
        ac.check_norm(case, bad)
    bad = good.clone()
    bad[2] = good[2] * 0
    with pytest.raises(AssertionError, match="row 2 outside the window changed"):
        ac.check_norm(case, bad)
