"""Int8-mirror exact search against the bf16 exact search on the same build.

For each (corpus, rows, B, filter) the two ops run in ONE process on the
same tensors, alternating: bf16 window (``ops.cosine_topk`` /
``ops.cosine_topk_filtered``: the streaming kernel smallb_emit_kernel_v4 over
the bf16 rows), q8 window (``ops.cosine_topk_q8``: q8_emit_kernel over the
int8 mirror, q8_rescore over the candidates), repeated ``--rounds`` times.
Every shape is warmed up first; each window is timed with device events
around at least ``--window`` seconds of calls (the call count is calibrated
per arm). Reported per cell: the median window's ms per call and the spread
(max - min) / median over the rounds for both arms, bf16 / q8, the mean and
max stage-1 candidates per query of both arms (one set of floors), overflow
fallbacks of the q8 arm, and the mirror's bytes. A ratio means something only
beside the spreads: the q8 arm "wins" a cell when it is faster by more than
both.

Corpora: the mixture and the isotropic corpus of routed_search_bench.py.
The filtered cells want label 0, drawn per row with probability 0.1, for
every query. Before timing, both arms must return the same indices wherever
the bf16 arm's k-th and (k+1)-th scores differ.

Also reported per corpus size: rows/s of ``EmbeddingStore.adopt`` with the
mirror on (the quantiser over all rows, in chunks of 1M).

Run: python benchmarks/q8_scan_bench.py [--rows 1000000,10000000]
         [--markdown table.md]   (results: profiles/q8_mirror.md)
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filtered_match_bench import _calibrate, _window_ms  # noqa: E402
from routed_search_bench import isotropic_corpus, mixture_corpus  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--corpora", default="mixture,isotropic")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--selectivity", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--markdown", default=None, help="also write the tables to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise RuntimeError("q8_scan_bench measures the GPU kernels; no GPU found")
    from kakveda_amd import ops
    from kakveda_amd.gfkb.engine import EmbeddingStore

    if not ops.hip_available():
        raise RuntimeError("HIP extension missing on a GPU box")
    ext = ops._require_ext()

    D, k = args.dim, args.k
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    results, adopts = [], []
    for N in [int(n) for n in args.rows.split(",")]:
        for name in args.corpora.split(","):
            if name == "mixture":
                corpus, queries, _ = mixture_corpus(
                    N, max(batches), D, dev, topics=4096, families=min(500_000, N // 2),
                    topic_spread=1.0, row_spread=1.22, query_spread=0.48)
            else:
                corpus, queries, _ = isotropic_corpus(N, max(batches), D, dev)
            store = EmbeddingStore(D, device="cuda", int8_mirror=True)
            ops.quantize_rows_q8(corpus[:64], *ops.new_q8_mirror(64, D, dev), 0)  # load the kernel
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store.adopt(corpus)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            codes, meta = store._codes[0], store._meta[0]
            mirror_bytes = codes.numel() + meta.numel() * 4
            adopt = {"corpus": name, "rows": N, "adopt_seconds": dt, "adopt_rows_per_s": N / dt,
                     "mirror_bytes": mirror_bytes, "row_bytes": corpus.numel() * 2}
            adopts.append(adopt)
            print(json.dumps(adopt), flush=True)
            gen = torch.Generator(device=dev).manual_seed(11)
            labels = torch.where(torch.rand(N, generator=gen, device=dev) < args.selectivity, 0, 1).to(torch.int32)
            for B in batches:
                q = queries[:B].contiguous()
                want = torch.zeros(B, dtype=torch.int32, device=dev)
                for filtered in (False, True):
                    filt = dict(labels=labels, want=want) if filtered else {}
                    arms = {
                        "bf16": (lambda: ops.cosine_topk_filtered(q, corpus, labels, want, k))
                        if filtered else (lambda: ops.cosine_topk(q, corpus, k)),
                        "q8": lambda: ops.cosine_topk_q8(q, corpus, codes, meta, k, **filt),
                    }
                    # sanity before timing (exactness is tests/test_gpu_q8.py's job)
                    s16, i16 = arms["bf16"]()
                    before = ops.q8_overflow_fallbacks
                    s8, i8 = arms["q8"]()
                    kk = min(k + 1, 8)
                    probe = (ops.cosine_topk_filtered(q, corpus, labels, want, kk)
                             if filtered else ops.cosine_topk(q, corpus, kk))[0]
                    clear = (probe[:, k - 1] - probe[:, k]) > D * 2.0 ** -22 if kk > k else None
                    same = (i8.sort(dim=1).values == i16.sort(dim=1).values).all(dim=1)
                    assert clear is None or bool(same[clear].all()), (name, N, B, filtered)
                    c8, c16 = ext.q8_counts_probe(q, corpus, codes, meta, k, N, **filt)
                    iters = {a: _calibrate(fn, args.window) for a, fn in arms.items()}
                    ms = {a: [] for a in arms}
                    for _ in range(args.rounds):
                        for a, fn in arms.items():  # alternate the arms
                            ms[a].append(_window_ms(fn, iters[a]))
                    row = {"corpus": name, "rows": N, "dim": D, "k": k, "B": B,
                           "filtered": filtered, "rounds": args.rounds,
                           "scores_bit_equal": bool(torch.equal(s8, s16)),
                           "q8_cand_mean": float(c8.float().mean()), "q8_cand_max": int(c8.max()),
                           "bf16_cand_mean": float(c16.float().mean()), "bf16_cand_max": int(c16.max()),
                           "q8_overflow_fallbacks": ops.q8_overflow_fallbacks - before,
                           "mirror_bytes": mirror_bytes}
                    for a in arms:
                        med = statistics.median(ms[a])
                        row[a + "_ms"] = med
                        row[a + "_spread"] = (max(ms[a]) - min(ms[a])) / med
                    row["bf16_over_q8"] = row["bf16_ms"] / row["q8_ms"]
                    results.append(row)
                    print(json.dumps(row), flush=True)
            del store, codes, meta, corpus, labels
            torch.cuda.empty_cache()

    lines = [
        "| corpus | rows | B | filter | bf16 ms | spread | q8 ms | spread | bf16 / q8 | cand/query bf16 mean (max) | cand/query q8 mean (max) | fallbacks |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for r in results:
        lines.append(
            "| %s | %d | %d | %s | %.3f | %.1f%% | %.3f | %.1f%% | %.2f | %.0f (%d) | %.0f (%d) | %d |"
            % (r["corpus"], r["rows"], r["B"], "10%" if r["filtered"] else "-", r["bf16_ms"],
               r["bf16_spread"] * 100, r["q8_ms"], r["q8_spread"] * 100, r["bf16_over_q8"],
               r["bf16_cand_mean"], r["bf16_cand_max"], r["q8_cand_mean"], r["q8_cand_max"],
               r["q8_overflow_fallbacks"])
        )
    lines += ["", "| corpus | rows | adopt s | rows/s | mirror bytes | bf16 row bytes |", "|---|---|---|---|---|---|"]
    for a in adopts:
        lines.append("| %s | %d | %.3f | %.3g | %d | %d |" % (
            a["corpus"], a["rows"], a["adopt_seconds"], a["adopt_rows_per_s"], a["mirror_bytes"], a["row_bytes"]))
    table = "\n".join(lines)
    print(table)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
