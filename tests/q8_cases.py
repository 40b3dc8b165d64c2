"""Shared inputs and checks of the int8-mirror tests (tests/test_q8_mirror.py
on the CPU, tests/test_gpu_q8.py on the GPU). Not a test module.

The planted input is the one that tells a correct two-stage search from a
broken one: its 16 rows per query lie 1e-4 apart in cosine, closer than the
int8 scores resolve, so a search without the per-row error margin loses true
top-8 rows and one that skips the bf16 rescore returns them in the wrong
order.
"""

import torch

import topk_adversarial as ta

from kakveda_amd import ops

D = 128
PLANT_N, PLANT_B, PLANT_K, PLANT_RUN = 65_573, 8, 8, 16


def planted_q8_case(d=D, n=PLANT_N, seed=900) -> ta.Case:
    """N = 65,573, B = 8, k = 8: query b owns rows [16b, 16b + 16), row j of
    its run at cosine 0.90 - 1e-4 * j to it; everything else random unit
    rows (cosines as planted in float64; the bf16 rows' own are what the
    float64 sims of the judge say)."""
    g = torch.Generator().manual_seed(seed)
    q = ta.rand_unit(PLANT_B, d, seed + 1)
    cosines = [0.90 - 1e-4 * j for j in range(PLANT_RUN)]
    rows = ta.near_rows(q, g, cosines).reshape(PLANT_B * PLANT_RUN, d)
    pos = torch.arange(PLANT_B * PLANT_RUN, dtype=torch.int64)
    return ta.Case(name="q8planted[N=%d,D=%d]" % (n, d), q=q, n=n, k=PLANT_K,
                   plant_pos=pos, plant_rows=rows)


def quantiser_rows(d: int, n: int, seed: int) -> torch.Tensor:
    """n >= 1 bf16 rows for the quantiser: Gaussian unit rows, with (as far
    as n allows) an all-zero row, a row of rounding ties, a row with one huge
    element, a tiny row and a row of +-amax written over the first ones."""
    x = ta.rand_unit(n, d, seed).float()
    special = []
    special.append(torch.zeros(d))
    # amax = 127 makes inv = 1 exactly: k + 0.5 are ties, round half to even
    tie = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 63.5, -126.5])
    special.append(torch.cat([tie.repeat(d // 8 - 1), torch.tensor([127.0, -3.5, 4.5, 0, 0, 0, 0, 0])]))
    huge = x[0].clone() if n else torch.zeros(d)
    huge[3] = 100.0
    special.append(huge)
    special.append(torch.full((d,), 2.0 ** -110))
    pm = torch.ones(d)
    pm[::3] = -1.0
    special.append(pm * 0.25)
    for i, row in enumerate(special[:n]):
        x[i] = row
    return x.to(torch.bfloat16)


def encoder_rows(n: int, d: int) -> torch.Tensor:
    from kakveda_amd.encoder.model import TraceEncoder

    enc = TraceEncoder(dim=d, hash_dim=4096, seed=7, device="cpu")
    texts = [
        "intent_tags:intent:%d | prompt_hint:summarize item %d with refs | tools:t%d | env_keys:e" % (i % 7, i, i % 3)
        for i in range(n)
    ]
    return enc.encode_texts(texts).to(torch.bfloat16)


def check_quantised(rows, codes, meta):
    """The quantiser's contract on (rows, codes, meta), all on the CPU."""
    x = rows.double()
    assert codes.dtype == torch.int8 and meta.dtype == torch.float32
    assert int(codes.min()) >= -127 and int(codes.max()) <= 127
    assert bool(torch.isfinite(meta).all())
    true = (x - meta[:, 0].double()[:, None] * codes.double()).norm(dim=1)
    err = meta[:, 1].double()
    assert bool((err >= true).all()), float((true - err).max())
    assert bool((err <= 1.01 * true + 1e-7).all()), float((err - 1.01 * true).max())
    zero = x.abs().amax(dim=1) == 0
    assert bool((meta[zero] == 0).all()) and bool((codes[zero] == 0).all())


def quantise_ref(rows):
    codes, meta = ops.new_q8_mirror(rows.shape[0], rows.shape[1], "cpu")
    ops.quantize_rows_q8_ref(rows, codes, meta, 0)
    return codes, meta
