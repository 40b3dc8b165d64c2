"""Flagship benchmark: pre-flight warning lookups/sec against a 10M-entry
GFKB (BASELINE.json north-star metric), on 1..8 MI355X GPUs.

Per step (the full warning_policy hot path of SURVEY.md section 3.2, on
synthetic traces / random-init fingerprint embeddings):
  1. encode a batch of pre-hashed signature features on GPU
     (embedding_bag HIP kernel + projection GEMM + L2 normalise),
  2. fused MFMA cosine-topk against this rank's HBM-resident GFKB shard,
  3. RCCL all-gather of per-shard (score, global-id) candidates over xGMI,
  4. top-k merge + threshold policy decision.

Corpus: `--entries` total random unit bf16 fingerprints, sharded evenly
across ranks (strong scaling: fixed total corpus). Every rank evaluates the
same `--batch` queries per step; one "lookup" = one query fully resolved
against the whole corpus.

Launch (driver contract):
  python bench.py --gpus 1 --steps 20 --warmup 5 [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
      --master-addr 127.0.0.1 bench.py --gpus 8 --steps 20 --warmup 5

A plain run does only what the headline figure needs: set up, warm up, time
`--steps` steps, print one JSON line. `--dump-outputs DIR` additionally
writes what the last timed step returned to its caller (rank 0 only) as
DIR/scores.npy (f32 [batch, topk]), DIR/ids.npy (global ids as f64, exact
below 2^53) and DIR/warn_count.npy (f64 [1]); inputs are seeded, so two
builds run with the same arguments can be compared output for output.
`--full` is where any measurement beyond the headline figure belongs (CPU
baselines, other sizes or precisions, per-kernel figures); the benchmark has
none today, so the flag currently adds nothing to a plain run.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--entries", type=int, default=10_000_000)
    p.add_argument("--batch", type=int, default=2048)
    p.add_argument("--topk", type=int, default=5)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--threshold", type=float, default=0.8)
    p.add_argument(
        "--dump-outputs",
        metavar="DIR",
        default=None,
        help="write the last timed step's outputs to DIR/<name>.npy",
    )
    p.add_argument(
        "--full",
        action="store_true",
        help="also run measurements beyond the headline figure (none today)",
    )
    return p.parse_args()


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    on_gpu = torch.cuda.is_available()
    dist = world > 1
    if dist:
        import torch.distributed as td

        td.init_process_group(backend="nccl" if on_gpu else "gloo")
    if on_gpu:
        device = torch.device(f"cuda:{local_rank}")
        torch.cuda.set_device(device)
    else:
        # CPU dry-run mode: same code path (sharding, all-gather merge)
        # over gloo with the torch fallback ops — used to validate the
        # exact torchrun launch contract without a GPU.
        device = torch.device("cpu")

    from kakveda_amd import ops
    from kakveda_amd.parallel.sharded import ShardedStore

    if on_gpu and not ops.hip_available():
        raise RuntimeError("HIP extension not built; run __graft_entry__.build() first")

    D, B, k = args.dim, args.batch, args.topk
    per_rank = args.entries // world

    # ---- build the sharded GFKB (synthetic fingerprints, bf16 in HBM) ----
    gen = torch.Generator(device=device).manual_seed(1000 + rank)
    cdtype = torch.bfloat16 if on_gpu else torch.float32
    corpus = torch.empty(per_rank, D, dtype=cdtype, device=device)
    fill = 1 << 20
    for s in range(0, per_rank, fill):
        e = min(s + fill, per_rank)
        corpus[s:e] = torch.randn(e - s, D, generator=gen, device=device, dtype=torch.float32).to(
            cdtype
        )
    ops.l2normalize_(corpus)
    store = ShardedStore(D, device=str(device), capacity=1024)
    store.load_shard(corpus, per_rank * world)  # zero-copy adopt

    # ---- query pool: pre-hashed synthetic signature features --------------
    # (feature hashing is CPU-side and untimed, as in production where the
    # signature arrives with the request; the encode GEMMs run in-step.)
    from kakveda_amd.encoder.featurizer import featurize_batch
    from kakveda_amd.encoder.model import TraceEncoder

    enc = TraceEncoder(dim=D, hash_dim=1 << 16, seed=1234, device=str(device))
    texts = [
        f"intent_tags:intent:citations_required | prompt_hint:synthetic probe "
        f"{i} explain with sources | tools:t{i % 7} | env_keys:e2e,k{i % 5}"
        for i in range(min(B, 1024))
    ]
    idx_np, w_np = featurize_batch(texts, hash_dim=enc.hash_dim, max_features=64)
    reps = (B + len(texts) - 1) // len(texts)
    feat_idx = torch.from_numpy(idx_np).to(device).repeat(reps, 1)[:B].contiguous()
    feat_w = torch.from_numpy(w_np).to(device).repeat(reps, 1)[:B].contiguous()

    last = {}

    def step() -> int:
        # 1. encode on GPU (embedding_bag kernel + projection GEMM + norm)
        q = enc.encode_features(feat_idx, feat_w).to(cdtype)
        # 2-4. fused cosine top-k per shard, RCCL all-gather over xGMI,
        #      exact (score, global-id) merge — kakveda_amd.parallel
        fs, fid = store.search(q, k)
        # 5. threshold policy decision
        warn = (fs[:, 0] >= args.threshold).sum()
        last["scores"], last["ids"], last["warn_count"] = fs, fid, warn
        return int(warn.item() >= 0)

    # ---- warmup ----------------------------------------------------------
    for _ in range(args.warmup):
        step()
    if dist:
        import torch.distributed as td

        td.barrier()
    if on_gpu:
        torch.cuda.synchronize()

    # ---- timed region ----------------------------------------------------
    times = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ts = time.perf_counter()
        step()
        if on_gpu:
            torch.cuda.synchronize()
        times.append(time.perf_counter() - ts)
    if dist:
        import torch.distributed as td

        td.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    if dist:
        import torch.distributed as td

        t = torch.tensor([elapsed], device=device)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        elapsed = float(t.item())

    lookups_per_sec = B * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0
    p50_ms = statistics.median(times) * 1000.0

    if rank == 0 and args.dump_outputs and last:
        import numpy as np

        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, t, dt in (
            ("scores", last["scores"], torch.float32),
            ("ids", last["ids"], torch.float64),
            ("warn_count", last["warn_count"].reshape(1), torch.float64),
        ):
            np.save(
                os.path.join(args.dump_outputs, name + ".npy"),
                t.detach().to("cpu", dt).numpy(),
            )

    if rank == 0:
        out = {
            "metric": "preflight_warning_lookups_per_sec",
            "value": lookups_per_sec,
            "unit": "lookups/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "fp32-cpu-dryrun",
            "data": "synthetic",
            "config": {
                "model": "gfkb-cosine-knn-768d",
                "global_batch": B,
                "seq_len": D,
                "parallelism": f"shard{world}",
                "entries": args.entries,
                "top_k": k,
                "p50_ms": p50_ms,
            },
        }
        print(json.dumps(out))

    if dist:
        import torch.distributed as td

        td.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())
