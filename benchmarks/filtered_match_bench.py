"""Label-filtered search against unfiltered search on the same build.

For each (batch, selectivity) the two ops run in ONE process on the same
tensors, alternating: unfiltered window, filtered window, repeated
``--rounds`` times. Every shape is warmed up first; each window is timed
with device events around at least ``--window`` seconds of calls (the call
count is calibrated per arm). Reported per arm: the median window's ms per
call and the spread (max - min) / median over the rounds, and the ratio of
the medians. The ratio means something only beside the spreads.

Every query of a filtered batch is filtered (want = label 0), the worst
case; label 0 is drawn per row with the stated probability.

Which kernels run (ops/hip/knn_plan.h): B <= 8 streams the corpus once in
both arms (smallb_emit_kernel_v4, filtered or not); above that the
unfiltered arm is the 8-phase emission core and the filtered arm the
128x128 list kernel, which is expected to be slower.

Run: python benchmarks/filtered_match_bench.py [--rows 10000000]
         [--markdown table.md]   (results: profiles/filtered_search.md)
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _window_ms(fn, iters: int) -> float:
    """ms per call over one device-event window of ``iters`` calls."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _calibrate(fn, window_s: float) -> int:
    fn()  # warm-up: code objects, allocator
    fn()
    torch.cuda.synchronize()
    ms = _window_ms(fn, 3)
    return max(3, int(window_s * 1000.0 / ms) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--batches", default="1,8,256")
    ap.add_argument("--selectivities", default="0.5,0.01,0.0001")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--markdown", default=None, help="also write the table to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise RuntimeError("filtered_match_bench measures the GPU kernels; no GPU found")
    from kakveda_amd import ops

    if not ops.hip_available():
        raise RuntimeError("HIP extension missing on a GPU box")

    N, D, k = args.rows, args.dim, args.k
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    corpus = torch.empty(N, D, dtype=torch.bfloat16, device=dev)
    for s in range(0, N, 1 << 20):
        e = min(s + (1 << 20), N)
        corpus[s:e] = torch.randn(e - s, D, generator=gen, device=dev).to(torch.bfloat16)
    ops.l2normalize_(corpus)
    u = torch.rand(N, generator=gen, device=dev)

    results = []
    for B in [int(b) for b in args.batches.split(",")]:
        q = torch.randn(B, D, generator=gen, device=dev).to(torch.bfloat16)
        ops.l2normalize_(q)
        want = torch.zeros(B, dtype=torch.int32, device=dev)
        for sel in [float(s) for s in args.selectivities.split(",")]:
            labels = torch.where(u < sel, 0, 1).to(torch.int32)
            eligible = int((labels == 0).sum())
            arms = {
                "unfiltered": lambda: ops.cosine_topk(q, corpus, k),
                "filtered": lambda: ops.cosine_topk_filtered(q, corpus, labels, want, k),
            }
            # sanity before timing: every filtered hit carries the wanted label
            # (exactness is the tests' job, tests/test_gpu_filtered_topk.py)
            _, fi = arms["filtered"]()
            assert bool(((fi < 0) | (labels[fi.clamp_min(0)] == 0)).all())
            iters = {name: _calibrate(fn, args.window) for name, fn in arms.items()}
            ms = {name: [] for name in arms}
            for _ in range(args.rounds):
                for name, fn in arms.items():  # alternate the arms
                    ms[name].append(_window_ms(fn, iters[name]))
            row = {"B": B, "rows": N, "dim": D, "k": k, "selectivity": sel,
                   "eligible_rows": eligible, "rounds": args.rounds}
            for name in arms:
                med = statistics.median(ms[name])
                row[name + "_ms"] = med
                row[name + "_spread"] = (max(ms[name]) - min(ms[name])) / med
                row[name + "_calls_per_window"] = iters[name]
            row["filtered_over_unfiltered"] = row["filtered_ms"] / row["unfiltered_ms"]
            results.append(row)
            print(json.dumps(row), flush=True)

    lines = [
        "| B | selectivity | eligible rows | unfiltered ms | spread | filtered ms | spread | filtered / unfiltered |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for r in results:
        lines.append(
            "| %d | %g%% | %d | %.3f | %.1f%% | %.3f | %.1f%% | %.3f |"
            % (r["B"], r["selectivity"] * 100, r["eligible_rows"], r["unfiltered_ms"],
               r["unfiltered_spread"] * 100, r["filtered_ms"], r["filtered_spread"] * 100,
               r["filtered_over_unfiltered"])
        )
    table = "\n".join(lines)
    print(table)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
