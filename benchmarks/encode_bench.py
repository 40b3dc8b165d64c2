"""Host featurizer against device featurizer on the same build.

Two encoders over the same weights run in ONE process, alternating: the
host arm (``device_featurize=False``: ``featurize_batch`` in Python, the
path every build before the device featurizer took) and the device arm
(``device_featurize=True``: pack, upload, ``ops.featurize_bytes``). What the
device featurizer saves is host time, so a call is timed with the wall
clock around ``encode_texts`` plus a device synchronise. A round is one
timed window of each arm at each batch size, repeated ``--rounds`` times;
reported per arm: the median round's ms per call and the spread
(max - min) / median over the rounds. ``DEVICE_FEATURIZE_MIN_B`` is forced
to 1 for the run, so the device arm is the kernel at every batch size.

The texts are realistic signatures (``core.signature.signature_text``:
prompts of 5 to 30 words from a fixed 30-word list, 0 to 3 tools, two env
keys). After the encode table, ``match_batch`` at ``--match-batch`` texts
against a store of ``--rows`` random unit rows, both arms (the rows have no
identity, so the search runs and no matches are built). The run ends with
the crossover: the smallest measured B from which on the device arm's
median stays below the host arm's by more than the larger of the two arms'
spreads (max - min over the rounds, in ms).

Run: python benchmarks/encode_bench.py [--rows 1000000] [--json out.json]
     (results: profiles/device_featurize.md)
"""

from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORDS = (
    "summarize explain describe the report include references citations sources "
    "please provide a short summary of this document with bibliography even if "
    "none translate code review quarterly results customer email draft policy"
).split()[:30]
TOOLS = ("search", "calculator", "browser", "code_interpreter", "retriever")


def signatures(n: int, seed: int = 7):
    from kakveda_amd.core.signature import signature_text

    rng = random.Random(seed)
    out = []
    for _ in range(n):
        prompt = " ".join(rng.choice(WORDS) for _ in range(rng.randint(5, 30)))
        tools = rng.sample(TOOLS, rng.randint(0, 3))
        env = {"region_%d" % rng.randint(0, 9): 1, "tier_%d" % rng.randint(0, 3): 1}
        out.append(signature_text(prompt, tools, env))
    return out


def _wall_ms(fn, iters: int) -> float:
    """Wall-clock ms per call over ``iters`` calls, the device drained."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0 / iters


def _calibrate(fn, window_s: float) -> int:
    fn()  # warm-up: code objects, allocator
    fn()
    ms = _wall_ms(fn, 2)
    return max(2, min(2000, int(window_s * 1000.0 / ms) + 1))


def _summary(samples):
    med = statistics.median(samples)
    return {
        "median_ms": med,
        "min_ms": min(samples),
        "max_ms": max(samples),
        "spread": (max(samples) - min(samples)) / med,
        "rounds_ms": samples,
    }


def run_arms(arms, rounds: int, window_s: float):
    """``arms``: {name: fn}. Alternates the arms round by round."""
    iters = {name: _calibrate(fn, window_s) for name, fn in arms.items()}
    samples = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            samples[name].append(_wall_ms(fn, iters[name]))
    return {name: dict(_summary(s), iters=iters[name]) for name, s in samples.items()}


def device_wins(row) -> bool:
    host, dev = row["host"], row["device"]
    band = max(host["max_ms"] - host["min_ms"], dev["max_ms"] - dev["min_ms"])
    return host["median_ms"] - dev["median_ms"] > band


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", default="1,8,64,256,2048")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--hash-dim", type=int, default=1 << 16)
    ap.add_argument("--rows", type=int, default=1_000_000, help="store rows for match_batch (0: skip)")
    ap.add_argument("--match-batch", type=int, default=2048)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three rounds"
    assert torch.cuda.is_available(), "encode_bench needs a GPU"

    from kakveda_amd.encoder import model as encoder_model
    from kakveda_amd.encoder.featurizer import featurize_batch
    from kakveda_amd.encoder.model import TraceEncoder
    from kakveda_amd.gfkb.engine import GfkbEngine

    encoder_model.DEVICE_FEATURIZE_MIN_B = 1
    batches = [int(b) for b in args.batches.split(",")]
    texts = signatures(max(batches + [args.match_batch]))
    nbytes = [len(t) for t in texts]
    result = {
        "device": torch.cuda.get_device_name(0),
        "rounds": args.rounds,
        "window_s": args.window,
        "text_bytes": {"min": min(nbytes), "mean": sum(nbytes) / len(nbytes), "max": max(nbytes)},
        "encode_texts": [],
    }

    enc = {
        "host": TraceEncoder(dim=args.dim, hash_dim=args.hash_dim, device="cuda"),
        "device": TraceEncoder(dim=args.dim, hash_dim=args.hash_dim, device="cuda",
                               device_featurize=True),
    }
    print("%6s %12s %8s %12s %8s %8s  %s" % (
        "B", "host ms", "spread", "device ms", "spread", "speedup", "device wins"))
    for B in batches:
        batch = texts[:B]
        row = run_arms(
            {name: (lambda e=e: e.encode_texts(batch)) for name, e in enc.items()},
            args.rounds, args.window,
        )
        # the featurizer alone, for the share of the host arm it accounts for
        row["featurize_batch_only"] = run_arms(
            {"host": lambda: featurize_batch(batch, hash_dim=args.hash_dim, seed=0,
                                             max_features=64)},
            args.rounds, args.window,
        )["host"]
        row["B"] = B
        row["device_wins"] = device_wins(row)
        result["encode_texts"].append(row)
        print("%6d %12.4f %7.1f%% %12.4f %7.1f%% %7.2fx  %s" % (
            B, row["host"]["median_ms"], 100 * row["host"]["spread"],
            row["device"]["median_ms"], 100 * row["device"]["spread"],
            row["host"]["median_ms"] / row["device"]["median_ms"], row["device_wins"]))
    result["host_fallbacks"] = enc["device"].host_fallbacks
    print("device arm host_fallbacks:", enc["device"].host_fallbacks)

    # the smallest measured B from which on the device arm wins
    min_b = None
    for row in reversed(result["encode_texts"]):
        if not row["device_wins"]:
            break
        min_b = row["B"]
    result["crossover_min_b"] = min_b
    print("crossover: device arm wins from B =", min_b)

    if args.rows > 0:
        with tempfile.TemporaryDirectory() as td:
            engines = {
                name: GfkbEngine(data_dir=os.path.join(td, name), device="cuda", dim=args.dim,
                                 hash_dim=args.hash_dim, device_featurize=(name == "device"))
                for name in ("host", "device")
            }
            gen = torch.Generator(device="cuda").manual_seed(3)
            for eng in engines.values():
                for s in range(0, args.rows, 1 << 18):
                    n = min(1 << 18, args.rows - s)
                    rows = torch.randn(n, args.dim, device="cuda", generator=gen)
                    rows = rows / rows.norm(dim=1, keepdim=True)
                    eng.store.append(rows.to(eng.store.dtype))
                gen.manual_seed(3)
            batch = texts[: args.match_batch]
            row = run_arms(
                {name: (lambda e=e: e.match_batch(batch)) for name, e in engines.items()},
                args.rounds, max(args.window, 1.0),
            )
            row["B"] = args.match_batch
            row["rows"] = args.rows
            row["device_wins"] = device_wins(row)
            result["match_batch"] = row
            print("match_batch B=%d rows=%d: host %.3f ms (%.1f%%), device %.3f ms (%.1f%%), %.2fx" % (
                args.match_batch, args.rows, row["host"]["median_ms"],
                100 * row["host"]["spread"], row["device"]["median_ms"],
                100 * row["device"]["spread"],
                row["host"]["median_ms"] / row["device"]["median_ms"]))

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "encode_texts"}, default=str))


if __name__ == "__main__":
    main()
