"""Label-filtered routed search against the exact filtered search, same build.

On the mixture corpus of ``routed_search_bench.py`` (10M x 768 by default)
every row gets label 1 with probability ``selectivity`` and label 0
otherwise, and the queries ask for label 1: "the top-k of this type" at a
type that ``selectivity`` of the rows have. Per selectivity and batch size,
in ONE process on the same tensors, alternating (a round is one timed window
of every arm, ``--rounds`` rounds, device events around at least ``--window``
seconds of calls, the call count calibrated per arm):

  exact           store.search(q, k, want=w): ops.cosine_topk_filtered
  routed n        store.search(q, k, want=w, nprobe=n, route_filtered=True),
                  exact fill on (the default), batched=None
  per-query / list-major
                  the same at the first nprobe with batched=False / True:
                  where the two scans cross for filtered batches
  mixed exact     10% of the queries filtered, the rest want=-1, answered as
                  today: the whole batch through the exact filtered search
  mixed routed    the same batch through the routed filtered search

Reported per arm: the median window's ms per call and the spread
(max - min) / median. Beside the times: recall@k and recall@1 of the routed
answer against the exact filtered answer with the fill on and off, and the
share of the batch's queries the fill re-ran.

Run: python benchmarks/routed_filtered_bench.py [--rows 10000000]
         [--json out.json] [--markdown table.md]
     (results: profiles/routed_filtered.md)
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

from routed_search_bench import _calibrate, _recalls, _window_ms, mixture_corpus  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64,256,2048")
    ap.add_argument("--nprobes", default="32,64")
    ap.add_argument("--selectivities", default="0.5,0.1,0.01,0.001")
    ap.add_argument("--mixed-share", type=float, default=0.10)
    ap.add_argument("--n-lists", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--mix-topics", type=int, default=4096)
    ap.add_argument("--mix-families", type=int, default=500_000)
    ap.add_argument("--mix-topic-spread", type=float, default=1.0)
    ap.add_argument("--mix-row-spread", type=float, default=1.22)
    ap.add_argument("--query-spread", type=float, default=0.48)
    ap.add_argument("--json", default=None, help="also write every result row here")
    ap.add_argument("--markdown", default=None, help="also write the table to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise RuntimeError("routed_filtered_bench measures the GPU kernels; no GPU found")
    from kakveda_amd import ops
    from kakveda_amd.gfkb.engine import EmbeddingStore

    if not ops.hip_available():
        raise RuntimeError("HIP extension missing on a GPU box")

    N, D, k = args.rows, args.dim, args.k
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    nq = max(batches)
    rows, queries, info = mixture_corpus(
        N, nq, D, dev, args.mix_topics, args.mix_families, args.mix_topic_spread,
        args.mix_row_spread, args.query_spread,
    )
    store = EmbeddingStore(D, device="cuda")
    store.adopt(rows)
    index = store.build_index(n_lists=args.n_lists)
    nprobes = sorted({min(int(p), index.n_lists) for p in args.nprobes.split(",")})
    head = {"corpus": "mixture", "rows": N, "dim": D, "k": k, "queries": nq,
            "index": dict(index.stats), "IVF_BATCHED_MIN_B": ops.IVF_BATCHED_MIN_B, **info}
    print(json.dumps(head), flush=True)

    gen = torch.Generator(device=dev).manual_seed(23)
    draw = torch.rand(N, generator=gen, device=dev)
    mixed_pick = torch.rand(nq, generator=gen, device=dev) < args.mixed_share
    results = []
    for sel in [float(s) for s in args.selectivities.split(",")]:
        labels = (draw < sel).to(torch.int32)
        store.adopt(rows, labels)  # the same rows under new labels
        store.index = index
        for B in batches:
            q = queries[:B].contiguous()
            w = torch.ones(B, dtype=torch.int32, device=dev)
            wm = torch.where(mixed_pick[:B], 1, -1).to(torch.int32)
            if B == 1:
                wm[0] = 1  # one query: the filtered one

            def routed(p, want=w, **kw):
                return store.search(q, k, want=want, nprobe=p, route_filtered=True, **kw)

            p0 = nprobes[0]
            arms = {"exact": lambda: store.search(q, k, want=w)}
            for p in nprobes:
                arms["routed %d" % p] = lambda p=p: routed(p)
            arms["per-query"] = lambda: routed(p0, batched=False)
            arms["list-major"] = lambda: routed(p0, batched=True)
            arms["mixed exact"] = lambda: store.search(q, k, want=wm)
            arms["mixed routed"] = lambda: routed(p0, want=wm)
            iters = {name: _calibrate(fn, args.window) for name, fn in arms.items()}
            ms = {name: [] for name in arms}
            for _ in range(args.rounds):
                for name, fn in arms.items():  # alternate the arms
                    ms[name].append(_window_ms(fn, iters[name]))
            med = {name: statistics.median(v) for name, v in ms.items()}
            spread = {name: (max(v) - min(v)) / med[name] for name, v in ms.items()}
            es, ei = arms["exact"]()
            row = {"selectivity": sel, "B": B, "label_rows": store.label_rows(1),
                   "rounds": args.rounds, "ms": med, "spread": spread}
            for p in nprobes:
                before = store.exact_fills
                _, ri = routed(p)
                filled = store.exact_fills - before
                _, ni = routed(p, fill_exact=False)
                r5, r1, _, _ = _recalls(ri, es, ei)
                n5, n1, _, _ = _recalls(ni, es, ei)
                row["nprobe %d" % p] = {
                    "routed_over_exact": med["routed %d" % p] / med["exact"],
                    "recall_at_k_fill": r5, "recall_at_1_fill": r1,
                    "recall_at_k_nofill": n5, "recall_at_1_nofill": n1,
                    "short_rows_nofill": int(((ni >= 0).sum(dim=1) < (ei >= 0).sum(dim=1)).sum()),
                    "fill_share": filled / B,
                }
            row["mixed_routed_over_exact"] = med["mixed routed"] / med["mixed exact"]
            row["mixed_filtered_queries"] = int((wm >= 0).sum())
            results.append(row)
            print(json.dumps(row), flush=True)

    cols = ["exact"] + ["routed %d" % p for p in nprobes] + [
        "per-query", "list-major", "mixed exact", "mixed routed"]
    lines = [
        "| selectivity | B | " + " | ".join("%s ms (spread)" % c for c in cols) + " | "
        + " | ".join("routed %d / exact | recall@%d fill / no fill | recall@1 fill / no fill "
                     "| fill share" % (p, k) for p in nprobes)
        + " | mixed routed / exact |",
        "|" + "---|" * (2 + len(cols) + 4 * len(nprobes) + 1),
    ]
    for r in results:
        cells = ["%g%%" % (100 * r["selectivity"]), "%d" % r["B"]]
        cells += ["%.3f (%.1f%%)" % (r["ms"][c], 100 * r["spread"][c]) for c in cols]
        for p in nprobes:
            a = r["nprobe %d" % p]
            cells += ["%.3f" % a["routed_over_exact"],
                      "%.3f / %.3f" % (a["recall_at_k_fill"], a["recall_at_k_nofill"]),
                      "%.3f / %.3f" % (a["recall_at_1_fill"], a["recall_at_1_nofill"]),
                      "%.1f%%" % (100 * a["fill_share"])]
        cells.append("%.3f" % r["mixed_routed_over_exact"])
        lines.append("| " + " | ".join(cells) + " |")
    table = "\n".join(lines)
    print(table)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump({"head": head, "results": results}, fh, indent=1)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write(json.dumps(head) + "\n\n" + table + "\n")


if __name__ == "__main__":
    main()
