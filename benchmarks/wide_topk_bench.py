"""The wide exact search (k = 16, 32, 64) beside the k = 8 search, same build.

For each (rows, B) the arms run in ONE process on the same tensors,
alternating: ``ops.cosine_topk`` at k = 8, then ``ops.cosine_topk_wide`` at
each wide k, repeated ``--rounds`` times. Every arm is warmed up first; each
window is timed with device events around at least ``--window`` seconds of
calls (the call count is calibrated per arm). Reported per cell: the median
window's ms per call and the spread (max - min) / median over the rounds,
the ratio to the k = 8 arm, the mean and max candidates per query of the wide
arm's emission pass, the count its plan expects (k * N / sampled rows, the
sample being the first 262,144 rows or the corpus), and overflow fallbacks.
A ratio means something only beside the spreads.

Corpus and queries: the isotropic ones of routed_search_bench.py. Before
timing, the first 8 score columns of every wide arm must agree with the
k = 8 arm within D * 2^-23.

Run: python benchmarks/wide_topk_bench.py [--rows 1000000,10000000]
         [--batches 1,64,2048] [--markdown table.md]
     (results: profiles/wide_topk.md)
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filtered_match_bench import _calibrate, _window_ms  # noqa: E402
from routed_search_bench import isotropic_corpus  # noqa: E402

SAMPLE_ROWS = 256 * 8 * 128  # knn_wide_plan.h: WIDE_PRE_BLOCKS * PRE_TILES * BN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--ks", default="16,32,64")
    ap.add_argument("--batches", default="1,64,2048")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--markdown", default=None, help="also write the table to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise RuntimeError("wide_topk_bench measures the GPU kernels; no GPU found")
    from kakveda_amd import ops

    if not ops.hip_available():
        raise RuntimeError("HIP extension missing on a GPU box")
    ext = ops._require_ext()

    D = args.dim
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    ks = [int(k) for k in args.ks.split(",")]
    results = []
    for N in [int(n) for n in args.rows.split(",")]:
        corpus, queries, _ = isotropic_corpus(N, max(batches), D, dev)
        for B in batches:
            q = queries[:B].contiguous()
            arms = {"k8": lambda: ops.cosine_topk(q, corpus, 8)}
            for k in ks:
                arms["k%d" % k] = lambda k=k: ops.cosine_topk_wide(q, corpus, k)
            s8 = arms["k8"]()[0]
            counts, fallbacks = {}, {}
            for k in ks:
                before = ops.wide_overflow_fallbacks
                sw = arms["k%d" % k]()[0]
                fallbacks[k] = ops.wide_overflow_fallbacks - before
                err = float((sw[:, :8].double() - s8.double()).abs().max())
                assert err <= D * 2.0 ** -23, (N, B, k, err)
                counts[k] = ext.wide_counts_probe(q, corpus, k, N)[3]
            iters = {a: _calibrate(fn, args.window) for a, fn in arms.items()}
            ms = {a: [] for a in arms}
            for _ in range(args.rounds):
                for a, fn in arms.items():  # alternate the arms
                    ms[a].append(_window_ms(fn, iters[a]))
            med8 = statistics.median(ms["k8"])
            for a in arms:
                med = statistics.median(ms[a])
                row = {"rows": N, "dim": D, "B": B, "arm": a, "ms": med,
                       "spread": (max(ms[a]) - min(ms[a])) / med, "over_k8": med / med8,
                       "rounds": args.rounds}
                if a != "k8":
                    k = int(a[1:])
                    c = counts[k]
                    row.update(cand_mean=float(c.float().mean()), cand_max=int(c.max()),
                               cand_expected=k * N / min(N, SAMPLE_ROWS), fallbacks=fallbacks[k])
                results.append(row)
                print(json.dumps(row), flush=True)
        del corpus, queries
        torch.cuda.empty_cache()

    lines = [
        "| rows | B | arm | ms | spread | / k8 | cand/query mean (max) | expected | fallbacks |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    for r in results:
        wide = "cand_mean" in r
        lines.append("| %d | %d | %s | %.3f | %.1f%% | %.2f | %s | %s | %s |" % (
            r["rows"], r["B"], r["arm"], r["ms"], r["spread"] * 100, r["over_k8"],
            "%.0f (%d)" % (r["cand_mean"], r["cand_max"]) if wide else "-",
            "%.0f" % r["cand_expected"] if wide else "-",
            "%d" % r["fallbacks"] if wide else "-"))
    table = "\n".join(lines)
    print(table)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
