"""Torch simulation of the staged int8 screen (knn_plan.h plan_q8_stages,
q8_plan.h "Staged floors"), shared by tests/test_q8_stages.py (CPU) and
tests/test_gpu_q8_stages.py.

The screen of one stage is ``ops.q8_screen_mask_ref`` over the stage's rows
with T from ``ops.q8_screen_params_ref`` of the floors in force; between two
stages each query's floor is raised to the k-th best exact (here: fp32 torch)
score among the entries it holds so far, seeds included; a query holding fewer
than k entries raises nothing.
"""

import torch

from kakveda_amd import ops


def geometric_bounds(prefix_tiles, ntiles, stages):
    """Tile bounds prefix * (ntiles / prefix)^(i / stages), unnudged."""
    return [round(prefix_tiles * (ntiles / prefix_tiles) ** (i / stages)) for i in range(stages + 1)]


def simulate(q, c, codes, meta, cnorm, k, bounds, sample_rows, n=None):
    """Run the stages ``[bounds[i], bounds[i + 1])`` (row numbers; bounds[-1]
    is clamped to n). The initial floors are the 8th best of the first
    ``sample_rows`` rows. With ``bounds[0] > 0`` the sample's top-8 are seeded
    and the stages start behind it (bounds[0] == sample_rows); with
    ``bounds[0] == 0`` nothing is seeded. Returns a dict: ``cand`` bool [B, n]
    (the screen's candidates, seeds not included), ``seeds`` bool [B, n],
    ``floors`` (list of fp32 [B]: the floors each stage screened against) and
    ``short`` (list of bool [B]: the queries that held fewer than k entries at
    each refresh)."""
    n = int(c.shape[0] if n is None else n)
    B = q.shape[0]
    dev = c.device
    sims = q.float() @ c[:n].float().t()
    top = torch.topk(sims[:, :sample_rows], 8, dim=1)
    floors = top.values[:, -1].clone()
    seeds = torch.zeros(B, n, dtype=torch.bool, device=dev)
    if bounds[0] > 0:
        assert bounds[0] == sample_rows
        seeds.scatter_(1, top.indices, True)
    cand = torch.zeros(B, n, dtype=torch.bool, device=dev)
    used, short = [], []
    for i in range(len(bounds) - 1):
        lo, hi = bounds[i], min(bounds[i + 1], n)
        used.append(floors.clone())
        qcodes, T, kappa, degenerate = ops.q8_screen_params_ref(q, floors, cnorm)
        assert degenerate == 0
        cand[:, lo:hi] = ops.q8_screen_mask_ref(qcodes, codes[lo:hi], meta[lo:hi], T, kappa, hi - lo)
        if i + 2 == len(bounds):
            break
        held = sims.masked_fill(~(seeds | cand), float("-inf"))
        kth = torch.topk(held, k, dim=1).values[:, -1]
        short.append(torch.isinf(kth))
        floors = torch.where(torch.isinf(kth), floors, torch.maximum(floors, kth))
    return dict(cand=cand, seeds=seeds, floors=used, short=short, sims=sims)
