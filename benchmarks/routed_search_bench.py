"""Routed (IVF) search against exact search on the same build.

For each corpus and batch size the exact arm (``EmbeddingStore.search``)
and two routed arms per ``nprobe`` - the per-query scan (``batched=False``)
and the list-major scan (``batched=True``) - run in ONE process on the same
tensors, alternating: a round is one timed window of every arm, repeated
``--rounds`` times. Every shape is warmed up first; each window is timed
with device events around at least ``--window`` seconds of calls (the call
count is calibrated per arm). Reported per arm: the median window's ms per
call and the spread (max - min) / median over the rounds.

Beside the times, per (B, nprobe): recall@5 and recall@1 of the routed
result against the exact arm's output on the same queries, recall
restricted to exact matches scoring >= 0.8 (the warning threshold), the
rows scanned per query (probed list lengths + tail), and the scan's
achieved bytes/s = rows x D x 2 / time of the scan op on its own (scan
kernel + its merge, precomputed probes), to set beside the ~5.5 TB/s the
hardware reaches on gathered whole rows of this size. The route (centroid
scoring), select (torch.topk on [B, L]) and group (sorting the (query,
probe) pairs by list, batched arm only) steps are timed on their own as
well, so their share of a routed call can be read off. ``--tail-fraction``
appends that share of the rows after the index is built: every routed
search scans them, and the list-major scan re-reads them once per tile of
queries, its worst case. The run ends with the crossover per ``nprobe``: the
smallest measured B from which on the batched arm's median stays below the
per-query arm's by more than the larger of the two arms' spreads (max - min
over the rounds, in ms).

Corpora (all seeded):
  encoder    templated signature texts through the real TraceEncoder; the
             queries are corpus texts with one token replaced
  mixture    two-level Gaussian mixture (topics -> families -> rows) sized
             by --mix-*; queries are perturbed rows. Its exact top-5 cosine
             profile is printed next to the encoder corpus's
  isotropic  unit Gaussian rows and queries: no structure, the worst case

Run: python benchmarks/routed_search_bench.py --corpus mixture --rows 10000000
         [--json out.json] [--markdown table.md]
     (results: profiles/routed_search.md)
"""

from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

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


def _unit(x: torch.Tensor) -> torch.Tensor:
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


# -- corpora ------------------------------------------------------------------

VERBS = ["summarize", "translate", "explain", "list", "compare", "write", "debug",
         "refactor", "classify", "extract"]
TOOLS = ["search", "calc", "sql", "browser", "python", "email", "calendar", "files"]


def encoder_corpus(n: int, n_queries: int, dim: int, dev, seed: int = 5):
    """Templated signature texts (a verb, 4-14 words of a 3000-word
    vocabulary, an optional citation clause, 0-3 tools, an env key) through
    the TraceEncoder; queries are corpus texts with one token replaced."""
    from kakveda_amd.core.signature import signature_text
    from kakveda_amd.encoder.model import TraceEncoder

    rnd = random.Random(seed)
    words = [f"w{i}" for i in range(3000)]

    def prompt():
        p = rnd.choice(VERBS) + " " + " ".join(
            rnd.choice(words) for _ in range(rnd.randint(4, 14))
        )
        return p + " and include references" if rnd.random() < 0.3 else p

    t0 = time.perf_counter()
    texts = [
        signature_text(prompt(), rnd.sample(TOOLS, rnd.randint(0, 3)),
                       {"env": rnd.choice(["prod", "dev", "e2e"])})
        for _ in range(n)
    ]
    enc = TraceEncoder(dim=dim, hash_dim=16384, seed=1234, device=str(dev))
    rows = torch.empty(n, dim, dtype=torch.bfloat16, device=dev)
    for s in range(0, n, 8192):
        rows[s : s + 8192] = _unit(enc.encode_texts(texts[s : s + 8192]).float()).to(
            torch.bfloat16
        )
    qt = []
    for i in rnd.sample(range(n), n_queries):
        toks = texts[i].split(" ")
        toks[rnd.randrange(len(toks))] = rnd.choice(words)
        qt.append(" ".join(toks))
    q = _unit(enc.encode_texts(qt).float()).to(torch.bfloat16)
    return rows, q, {"generate_seconds": time.perf_counter() - t0}


def mixture_corpus(n, n_queries, dim, dev, topics, families, topic_spread,
                   row_spread, query_spread, seed=7):
    """topics unit centres; each family = unit(topic + topic_spread * noise);
    each row = unit(family + row_spread * noise) (noise of norm ~1)."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    sd = 1.0 / dim ** 0.5
    t0 = time.perf_counter()
    top = _unit(torch.randn(topics, dim, generator=gen, device=dev))
    fam_topic = torch.randint(0, topics, (families,), generator=gen, device=dev)
    fam = torch.empty(families, dim, device=dev)
    for s in range(0, families, 1 << 18):
        e = min(s + (1 << 18), families)
        noise = torch.randn(e - s, dim, generator=gen, device=dev) * sd
        fam[s:e] = _unit(top[fam_topic[s:e]] + topic_spread * noise)
    rows = torch.empty(n, dim, dtype=torch.bfloat16, device=dev)
    for s in range(0, n, 1 << 20):
        e = min(s + (1 << 20), n)
        f = torch.randint(0, families, (e - s,), generator=gen, device=dev)
        noise = torch.randn(e - s, dim, generator=gen, device=dev) * sd
        rows[s:e] = _unit(fam[f] + row_spread * noise).to(torch.bfloat16)
    pick = torch.randint(0, n, (n_queries,), generator=gen, device=dev)
    noise = torch.randn(n_queries, dim, generator=gen, device=dev) * sd
    q = _unit(rows[pick].float() + query_spread * noise).to(torch.bfloat16)
    return rows, q, {"generate_seconds": time.perf_counter() - t0}


def isotropic_corpus(n, n_queries, dim, dev, seed=7):
    gen = torch.Generator(device=dev).manual_seed(seed)
    t0 = time.perf_counter()
    rows = torch.empty(n, dim, dtype=torch.bfloat16, device=dev)
    for s in range(0, n, 1 << 20):
        e = min(s + (1 << 20), n)
        rows[s:e] = _unit(torch.randn(e - s, dim, generator=gen, device=dev)).to(
            torch.bfloat16
        )
    q = _unit(torch.randn(n_queries, dim, generator=gen, device=dev)).to(torch.bfloat16)
    return rows, q, {"generate_seconds": time.perf_counter() - t0}


# -- measurement --------------------------------------------------------------

def _recalls(ri, es, ei):
    """(recall@5, recall@1, hits and total over exact matches >= 0.8)."""
    B, k = ei.shape
    found = (ei.unsqueeze(2) == ri.unsqueeze(1)).any(dim=2) & (ei >= 0)
    r5 = found.float().sum().item() / max(int((ei >= 0).sum()), 1)
    r1 = found[:, 0].float().mean().item()
    warn = (es >= 0.8) & (ei >= 0)
    return r5, r1, int((found & warn).sum()), int(warn.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=["encoder", "mixture", "isotropic"], required=True)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64,256,2048")
    ap.add_argument("--nprobes", default="1,4,8,16,32,64,128")
    ap.add_argument("--n-lists", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--mix-topics", type=int, default=4096)
    ap.add_argument("--mix-families", type=int, default=500_000)
    ap.add_argument("--mix-topic-spread", type=float, default=1.0)
    ap.add_argument("--mix-row-spread", type=float, default=1.22)
    ap.add_argument("--query-spread", type=float, default=0.48)
    ap.add_argument("--tail-fraction", type=float, default=0.0,
                    help="rows appended after the index build, as a share of --rows")
    ap.add_argument("--json", default=None, help="also write every result row here")
    ap.add_argument("--markdown", default=None, help="also write the tables to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise RuntimeError("routed_search_bench measures the GPU kernels; no GPU found")
    from kakveda_amd import ops
    from kakveda_amd.gfkb.engine import EmbeddingStore

    if not ops.hip_available():
        raise RuntimeError("HIP extension missing on a GPU box")

    N, D, k = args.rows, args.dim, args.k
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    nq = max(batches)
    n_tail = int(round(N * args.tail_fraction))
    n_all = N + n_tail  # the tail rows come from the same generator
    if args.corpus == "encoder":
        rows, queries, info = encoder_corpus(n_all, nq, D, dev)
    elif args.corpus == "mixture":
        rows, queries, info = mixture_corpus(
            n_all, nq, D, dev, args.mix_topics, args.mix_families, args.mix_topic_spread,
            args.mix_row_spread, args.query_spread,
        )
    else:
        rows, queries, info = isotropic_corpus(n_all, nq, D, dev)
    torch.cuda.synchronize()

    store = EmbeddingStore(D, device="cuda")
    store.adopt(rows[:N] if n_tail else rows)
    index = store.build_index(n_lists=args.n_lists)
    if n_tail:
        store.append(rows[N:])
        del rows
    torch.cuda.synchronize()
    segments = [seg for seg, _v, _b in store._live_segments()]
    n_live, n_indexed = store.count, index.n_indexed
    es, ei = store.search(queries, k)
    profile = es.float().mean(dim=0).tolist()
    head = {
        "corpus": args.corpus, "rows": N, "tail_rows": n_tail, "dim": D, "k": k,
        "queries": nq,
        "exact_top%d_mean_cosine" % k: profile,
        "exact_matches_ge_0.8": int((es >= 0.8).sum()),
        "index": {key: val for key, val in index.stats.items()},
        **info,
    }
    print(json.dumps(head), flush=True)

    ext = ops._require_ext()
    lens = (index.offsets[1:] - index.offsets[:-1])
    nprobes = sorted({min(int(p), index.n_lists) for p in args.nprobes.split(",")})
    results = []
    for B in batches:
        q = queries[:B].contiguous()
        exs, exi = store.search(q, k)
        arms = {"exact": lambda: store.search(q, k)}
        for p in nprobes:
            arms["nprobe=%d" % p] = (
                lambda p=p: store.search(q, k, nprobe=p, batched=False))
            arms["nprobe=%d batched" % p] = (
                lambda p=p: store.search(q, k, nprobe=p, batched=True))
        iters = {name: _calibrate(fn, args.window) for name, fn in arms.items()}
        ms = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():  # alternate the arms
                ms[name].append(_window_ms(fn, iters[name]))
        exact_ms = statistics.median(ms["exact"])
        for p in nprobes:
            name, bname = "nprobe=%d" % p, "nprobe=%d batched" % p
            rs, ri = arms[name]()
            bs, bi = arms[bname]()
            r5, r1, wh, wt = _recalls(ri, exs, exi)
            b5, b1, bwh, bwt = _recalls(bi, exs, exi)
            route = ops.ivf_route_scores(q, index.centroids)
            probes = torch.topk(route, p, dim=1).indices.to(torch.int32)
            scanned = float(lens[probes.long()].sum(dim=1).float().mean()) + n_tail
            # the steps on their own (shorter windows: they only apportion
            # the routed call, the arms above are the result). scan_batched
            # includes its grouping, which is also timed alone.
            scan_args = (q, segments, index.offsets, index.ids, probes, k, n_live,
                         n_indexed, n_live, index.max_list_len)
            parts = {
                "route": lambda: ops.ivf_route_scores(q, index.centroids),
                "select": lambda: torch.topk(route, p, dim=1).indices.to(torch.int32),
                "group": lambda: ext.ivf_group_probes(probes, index.n_lists),
                "scan": lambda: ops.ivf_scan_topk(*scan_args, batched=False),
                "scan_batched": lambda: ops.ivf_scan_topk(*scan_args, batched=True),
            }
            part_ms = {}
            for pname, fn in parts.items():
                part_ms[pname] = _window_ms(fn, _calibrate(fn, min(args.window, 0.25)))
            med = statistics.median(ms[name])
            bmed = statistics.median(ms[bname])
            row = {
                "corpus": args.corpus, "B": B, "rows": N, "tail_rows": n_tail,
                "nprobe": p, "n_lists": index.n_lists,
                "exact_ms": exact_ms,
                "exact_spread": (max(ms["exact"]) - min(ms["exact"])) / exact_ms,
                "routed_ms": med,
                "routed_spread": (max(ms[name]) - min(ms[name])) / med,
                "routed_over_exact": med / exact_ms,
                "batched_ms": bmed,
                "batched_spread": (max(ms[bname]) - min(ms[bname])) / bmed,
                "batched_over_exact": bmed / exact_ms,
                "batched_over_routed": bmed / med,
                "recall_at_5": r5, "recall_at_1": r1,
                "recall_ge_0.8": [wh, wt],
                "batched_recall_at_5": b5, "batched_recall_at_1": b1,
                "batched_recall_ge_0.8": [bwh, bwt],
                "batched_ids_equal": (bi == ri).float().mean().item(),
                "batched_max_score_diff": (bs - rs)[(bi >= 0) & (ri >= 0)].abs().max().item(),
                "rows_scanned_per_query": scanned,
                "scanned_fraction": scanned / n_live,
                "route_ms": part_ms["route"], "select_ms": part_ms["select"],
                "group_ms": part_ms["group"],
                "scan_ms": part_ms["scan"],
                "scan_batched_ms": part_ms["scan_batched"],
                "scan_TBps": B * scanned * D * 2 / (part_ms["scan"] * 1e-3) / 1e12,
                "rounds": args.rounds,
            }
            results.append(row)
            print(json.dumps(row), flush=True)

    # crossover per nprobe: the smallest measured B from which on the batched
    # median is below the per-query median by more than the larger spread (ms)
    crossover = {}
    for p in nprobes:
        first = None
        for r in sorted((r for r in results if r["nprobe"] == p), key=lambda r: r["B"]):
            margin = max(r["routed_spread"] * r["routed_ms"],
                         r["batched_spread"] * r["batched_ms"])
            if r["routed_ms"] - r["batched_ms"] > margin:
                first = r["B"] if first is None else first
            else:
                first = None
        crossover[str(p)] = first
    print(json.dumps({"corpus": args.corpus, "rows": N, "tail_rows": n_tail,
                      "batched_crossover_B": crossover}), flush=True)

    lines = [
        "| B | nprobe | rows scanned / query | exact ms | spread | per-query ms | spread | "
        "batched ms | spread | per-query / exact | batched / exact | batched / per-query | "
        "recall@5 per-query | batched | recall@1 per-query | batched | "
        "recall (score >= 0.8) per-query | batched | route ms | select ms | group ms | "
        "scan ms | batched scan ms | scan TB/s |",
        "|" + "---|" * 24,
    ]
    for r in results:
        lines.append(
            "| %d | %d | %.0f (%.2f%%) | %.3f | %.1f%% | %.3f | %.1f%% | %.3f | %.1f%% | "
            "%.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %d/%d | %d/%d | %.3f | %.3f "
            "| %.3f | %.3f | %.3f | %.2f |"
            % (r["B"], r["nprobe"], r["rows_scanned_per_query"],
               r["scanned_fraction"] * 100, r["exact_ms"], r["exact_spread"] * 100,
               r["routed_ms"], r["routed_spread"] * 100, r["batched_ms"],
               r["batched_spread"] * 100, r["routed_over_exact"],
               r["batched_over_exact"], r["batched_over_routed"],
               r["recall_at_5"], r["batched_recall_at_5"], r["recall_at_1"],
               r["batched_recall_at_1"], r["recall_ge_0.8"][0], r["recall_ge_0.8"][1],
               r["batched_recall_ge_0.8"][0], r["batched_recall_ge_0.8"][1],
               r["route_ms"], r["select_ms"], r["group_ms"], r["scan_ms"],
               r["scan_batched_ms"], r["scan_TBps"])
        )
    table = "\n".join(lines)
    print(table)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump({"head": head, "results": results,
                       "batched_crossover_B": crossover}, fh, indent=1)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write(json.dumps(head) + "\n\n" + table + "\n")


if __name__ == "__main__":
    main()
