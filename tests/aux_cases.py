"""Case builders with exact oracles for the kernels around the search:
kmeans_update, kmeans_assign(_scored), embedding_bag and l2normalize_.

Imported by tests/test_aux_cases_ref.py (CPU: the plain-torch fallbacks of
kakveda_amd.ops under the oracles) and tests/test_gpu_aux_exact.py (the HIP
kernels under the same oracles). Not a test module and not a conftest.

Where arithmetic can be made exact no tolerance is used: the inputs are
small integers (or multiples of 1/8), exact in bf16, chosen so that every
product and every partial sum, in any order, is an integer (or a multiple of
1/8) below 2^24 in magnitude and therefore exact in fp32. A correct kernel is
then bit-equal to the int64 / float64 oracle whatever its summation order,
its MFMA shape or its atomics, and anything dropped, doubled or mis-indexed
changes an integer. Every builder asserts its own exactness precondition, so
a bad case fails here, on the CPU, not on the GPU. Everything is generated
with seeded CPU generators; builders are cached and their tensors are shared
between the tests, which copy them to their device and never modify them.
"""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import torch

F32_EXACT = 2 ** 24  # every integer of magnitude <= 2^24 is an fp32 value


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _ints(lo: int, hi: int, shape, g: torch.Generator) -> torch.Tensor:
    """Seeded integers in [lo, hi] as int64."""
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


def _as_bf16_exact(x: torch.Tensor) -> torch.Tensor:
    b = x.to(torch.bfloat16)
    assert torch.equal(b.to(torch.float64), x.to(torch.float64)), "values are not exact in bf16"
    return b


# ---------------------------------------------------------------------------
# kmeans_update
# ---------------------------------------------------------------------------

@dataclass
class UpdateCase:
    name: str
    points: torch.Tensor  # bf16 [N, D], integers in [-4, 4]
    assign: torch.Tensor  # int32 [N]
    C: int
    sums: torch.Tensor  # f32 [C, D], exact
    counts: torch.Tensor  # f32 [C], exact
    n_dropped: int  # points whose assignment is outside [0, C)
    empty: Optional[int]  # a cluster no point is assigned to


#: (C, D, N, fraction of out-of-range assignments, leave a cluster empty).
#: The binding cuts N into chunks of ppc = ceil(N / (2048 / (D / 64))) points;
#: a block's four point lanes walk 64 points per unrolled pass, then a
#: stride-4 tail. C <= 128 keeps four LDS replicas, C > 128 one with atomics.
UPDATE_CASES = (
    (64, 768, 20003, 0.0, False),   # 4 replicas; ppc = 118: one unrolled pass + tail
    (128, 64, 150001, 0.0, False),  # 4 replicas at the LDS limit; ppc = 74
    (129, 64, 150001, 0.0, False),  # first single-replica size
    (512, 128, 40000, 0.0, False),  # the maximum C; ppc = 40: tail loop only
    (1, 64, 3, 0.0, False),         # N below the chunk count
    (5, 64, 1, 0.0, False),
    (7, 192, 67, 0.0, False),
    (64, 128, 20003, 0.05, False),  # ~5 % assigned -1 or C: dropped, 4 replicas
    (200, 64, 9001, 0.05, False),   # the same on the single-replica path
    (9, 64, 5000, 0.0, True),       # an empty cluster: sum and count exactly 0
    (130, 64, 5000, 0.0, True),
)


def update_chunk_points(D: int, N: int) -> int:
    """points_per_chunk as the binding computes it (kakveda_kernels.hip)."""
    chunks = max(1, 2048 // (D // 64))
    return (N + chunks - 1) // chunks


@lru_cache(maxsize=None)
def update_case(C: int, D: int, N: int, bad_frac: float = 0.0, empty: bool = False,
                seed: int = 11) -> UpdateCase:
    g = _gen(seed + 7 * C + D + N)
    pts = _ints(-4, 4, (N, D), g)
    # exactness: any partial sum of any subset, in any order, is an integer
    # of magnitude <= 4 N < 2^24
    assert int(pts.abs().max()) <= 4 and 4 * N < F32_EXACT
    hole = C // 2 if empty else None
    if empty:
        assert C >= 2
        a = _ints(0, C - 2, (N,), g)
        a = a + (a >= hole).long()  # skip the hole
    else:
        a = _ints(0, C - 1, (N,), g)
    n_bad = int(round(bad_frac * N))
    if n_bad:
        where = torch.randperm(N, generator=g)[:n_bad]
        a[where[0::2]] = -1
        a[where[1::2]] = C
    live = (a >= 0) & (a < C)
    sums = torch.zeros(C, D, dtype=torch.int64).index_add_(0, a[live], pts[live])
    counts = torch.zeros(C, dtype=torch.int64).index_add_(0, a[live], torch.ones_like(a[live]))
    assert int(counts.sum()) == N - n_bad and int(counts.max()) < F32_EXACT
    if empty:
        assert int(counts[hole]) == 0
    elif N >= 20 * C:
        assert int(counts.min()) > 0
    return UpdateCase(
        name="update[C=%d,D=%d,N=%d,bad=%d%s]" % (C, D, N, n_bad, ",empty" if empty else ""),
        points=_as_bf16_exact(pts), assign=a.to(torch.int32), C=C,
        sums=sums.to(torch.float32), counts=counts.to(torch.float32),
        n_dropped=n_bad, empty=hole,
    )


def check_update(case: UpdateCase, sums: torch.Tensor, counts: torch.Tensor) -> None:
    sums, counts = sums.cpu(), counts.cpu()
    assert sums.dtype == torch.float32 and counts.dtype == torch.float32, case.name
    assert sums.shape == case.sums.shape and counts.shape == case.counts.shape, case.name
    if not torch.equal(counts, case.counts):
        c = int((counts != case.counts).nonzero()[0])
        raise AssertionError("%s: count of cluster %d is %r, exact %r (%d clusters differ)" % (
            case.name, c, float(counts[c]), float(case.counts[c]), int((counts != case.counts).sum())))
    if not torch.equal(sums, case.sums):
        bad = (sums != case.sums).nonzero()
        c, d = (int(v) for v in bad[0])
        raise AssertionError("%s: sum[%d, %d] is %r, exact %r (%d of %d entries differ)" % (
            case.name, c, d, float(sums[c, d]), float(case.sums[c, d]), bad.shape[0], sums.numel()))
    if case.empty is not None:
        assert float(counts[case.empty]) == 0.0 and not bool(sums[case.empty].any()), case.name


# ---------------------------------------------------------------------------
# kmeans_assign / kmeans_assign_scored
# ---------------------------------------------------------------------------

@dataclass
class AssignCase:
    name: str
    points: torch.Tensor  # bf16 [N, D], integers in [-2, 2]
    centroids: torch.Tensor  # bf16 [C, D], integers in [-2, 2]
    score: torch.Tensor  # f32 [N]: the exact best dot
    lowest: torch.Tensor  # int64 [N]: the lowest index achieving it
    sims: Optional[torch.Tensor]  # f32 [N, C] exact dots (None for the largest case)
    tied_rows: int  # rows whose best dot is achieved more than once


@lru_cache(maxsize=None)
def assign_case(N: int, D: int, C: int, negative: bool = False, keep_sims: bool = True,
                seed: int = 23) -> AssignCase:
    g = _gen(seed + 3 * N + 5 * D + 7 * C)
    if negative:
        # every dot is negative: a masked or padded column scoring 0 would win
        pts = _ints(1, 2, (N, D), g)
        cents = -_ints(1, 2, (C, D), g)
    else:
        pts = _ints(-2, 2, (N, D), g)
        cents = _ints(-2, 2, (C, D), g)
    # a quarter of the centroids repeat another one, so exact ties sit at
    # arbitrary pairs of columns besides the ones small integers give anyway
    for _ in range(C // 4):
        src, dst = (int(v) for v in torch.randperm(C, generator=g)[:2])
        cents[dst] = cents[src]
    # exactness: every product is an integer of magnitude <= 4, every partial
    # sum of a dot an integer of magnitude <= 4 D < 2^24
    assert int(pts.abs().max()) <= 2 and int(cents.abs().max()) <= 2 and 4 * D < F32_EXACT
    sims = pts.double() @ cents.double().t()  # exact: integers far below 2^53
    assert float(sims.abs().max()) <= 4 * D
    best = sims.max(dim=1).values
    hit = sims == best[:, None]
    cols = torch.arange(C, dtype=torch.int64)[None, :].expand(N, C)
    lowest = torch.where(hit, cols, torch.full_like(cols, C)).min(dim=1).values
    if negative:
        assert float(best.max()) < 0
    return AssignCase(
        name="assign[N=%d,D=%d,C=%d%s]" % (N, D, C, ",negative" if negative else ""),
        points=_as_bf16_exact(pts), centroids=_as_bf16_exact(cents),
        score=best.to(torch.float32), lowest=lowest,
        sims=sims.to(torch.float32) if keep_sims else None,
        tied_rows=int((hit.sum(dim=1) > 1).sum()),
    )


def check_assign(case: AssignCase, score: torch.Tensor, idx: torch.Tensor, lowest_index: bool) -> None:
    """Exact best score; the lowest index achieving it (the dedicated kernel
    and the CPU path) or any index achieving it (the general route)."""
    score, idx = score.cpu(), idx.cpu()
    N = case.points.shape[0]
    C = case.centroids.shape[0]
    assert score.shape == (N,) and idx.shape == (N,), (case.name, score.shape, idx.shape)
    assert score.dtype == torch.float32 and idx.dtype == torch.int64, (case.name, score.dtype, idx.dtype)
    if not torch.equal(score, case.score):
        bad = (score != case.score).nonzero()[:, 0]
        r = int(bad[0])
        raise AssertionError("%s: row %d scores %r, exact max %r (%d of %d rows differ)" % (
            case.name, r, float(score[r]), float(case.score[r]), bad.numel(), N))
    assert bool(((idx >= 0) & (idx < C)).all()), "%s: index outside [0, %d)" % (case.name, C)
    if lowest_index:
        if not torch.equal(idx, case.lowest):
            bad = (idx != case.lowest).nonzero()[:, 0]
            r = int(bad[0])
            raise AssertionError("%s: row %d returns %d, lowest argmax is %d (%d of %d rows differ)" % (
                case.name, r, int(idx[r]), int(case.lowest[r]), bad.numel(), N))
    else:
        got = case.sims.gather(1, idx[:, None])[:, 0]
        if not torch.equal(got, case.score):
            bad = (got != case.score).nonzero()[:, 0]
            r = int(bad[0])
            raise AssertionError("%s: row %d returns %d whose dot is %r, the max is %r (%d of %d rows differ)" % (
                case.name, r, int(idx[r]), float(got[r]), float(case.score[r]), bad.numel(), N))


# ---------------------------------------------------------------------------
# embedding_bag
# ---------------------------------------------------------------------------

@dataclass
class BagCase:
    name: str
    table: torch.Tensor  # bf16 [V, D], integers in [-8, 8]
    idx: torch.Tensor  # int32 or int64 [B, L]; some -1 or V
    w: torch.Tensor  # f32 [B, L], multiples of 1/8 in [-4, 4]; some 0
    out: torch.Tensor  # f32 [B, D], exact
    n_ignored: int  # out-of-range indices (all with non-zero weight)
    n_zero_w: int


#: (B, L, D, V)
BAG_CASES = (
    (300, 128, 768, 7),   # L at the staging limit, D = 3 passes of the block
    (1, 1, 64, 7),        # one bag of one index
    (64, 48, 1000, 5000), # D no multiple of the 256 threads
    (5, 128, 8, 3),       # D below a wave
)


@lru_cache(maxsize=None)
def bag_case(B: int, L: int, D: int, V: int, idx_dtype: torch.dtype = torch.int32,
             seed: int = 37) -> BagCase:
    g = _gen(seed + B + 3 * L + 5 * D + V)
    table = _ints(-8, 8, (V, D), g)
    w8 = _ints(-32, 32, (B, L), g)  # weights in eighths
    idx = _ints(0, V - 1, (B, L), g)
    n = B * L
    flat_i, flat_w = idx.view(-1), w8.view(-1)
    order = torch.randperm(n, generator=g)
    n_bad = n // 10
    n_zero = n // 10
    bad, zero = order[:n_bad], order[n_bad:n_bad + n_zero]
    flat_i[bad[0::2]] = -1
    flat_i[bad[1::2]] = V
    # an ignored index must have weight: it has to be the index rule that drops it
    flat_w[bad] = torch.where(flat_w[bad] == 0, torch.ones_like(flat_w[bad]), flat_w[bad])
    flat_w[zero] = 0
    # exactness: every term is a multiple of 1/8 of magnitude <= 32, so every
    # partial sum of a bag is a multiple of 1/8 of magnitude <= 32 L <= 4096,
    # i.e. an integer count of eighths below 2^15
    assert int(table.abs().max()) <= 8 and int(w8.abs().max()) <= 32 and L <= 128
    assert 8 * 32 * L < F32_EXACT
    live = (idx >= 0) & (idx < V)
    rows = table[idx.clamp(0, V - 1)].double()  # [B, L, D]
    out = (rows * ((w8.double() / 8.0) * live)[:, :, None]).sum(dim=1)
    assert torch.equal(out.float().double(), out)
    w = (w8.double() / 8.0).to(torch.float32)
    assert torch.equal(w.double() * 8.0, w8.double())
    return BagCase(
        name="bag[B=%d,L=%d,D=%d,V=%d,%s]" % (B, L, D, V, str(idx_dtype).split(".")[-1]),
        table=_as_bf16_exact(table), idx=idx.to(idx_dtype), w=w, out=out.to(torch.float32),
        n_ignored=int((~live).sum()), n_zero_w=int((w8 == 0).sum()),
    )


def check_bag(case: BagCase, out: torch.Tensor) -> None:
    out = out.cpu()
    assert out.dtype == torch.float32 and out.shape == case.out.shape, (case.name, out.dtype, out.shape)
    if not torch.equal(out, case.out):
        bad = (out != case.out).nonzero()
        b, d = (int(v) for v in bad[0])
        raise AssertionError("%s: out[%d, %d] is %r, exact %r (%d of %d entries differ)" % (
            case.name, b, d, float(out[b, d]), float(case.out[b, d]), bad.shape[0], out.numel()))


# ---------------------------------------------------------------------------
# l2normalize_
# ---------------------------------------------------------------------------

@dataclass
class NormCase:
    name: str
    x: torch.Tensor  # bf16 [R, D]: the tensor before the call (never modified)
    start: int
    end: int
    ref: torch.Tensor  # f64 [end - start, D]: normalised rows of the window
    zero_rows: tuple  # rows (absolute) that are all zero


def norm_bound(D: int) -> float:
    """Relative bound on an element of a normalised bf16 row against the
    float64 normalisation of the same bf16 input: 2^-8 is half a bf16 ulp
    relative to the element (8 significand bits, round to nearest), D * 2^-23
    covers the fp32 sum of D squares (relative error <= D * 2^-24, halved by
    the square root), the reciprocal square root and the product."""
    return 2.0 ** -8 + D * 2.0 ** -23


@lru_cache(maxsize=None)
def norm_case(R: int, D: int, start: int = 0, end: Optional[int] = None, seed: int = 41) -> NormCase:
    g = _gen(seed + R + 3 * D)
    end = R if end is None else end
    x = torch.randn(R, D, generator=g, dtype=torch.float32)
    zero_rows = ()
    if R >= 8:
        x[start + 1] *= 2.0 ** 30
        x[start + 2] *= 2.0 ** -30
        x[start + 4] = 0
        x[end - 1] *= 2.0 ** 30
        zero_rows = (start + 4,)
    x = x.to(torch.bfloat16)
    seg = x[start:end].double()
    norm = seg.norm(dim=-1, keepdim=True)
    ref = torch.where(norm > 0, seg / norm.clamp_min(1e-300), torch.zeros_like(seg))
    assert bool(torch.isfinite(ref).all())
    # the derived bound presumes normal bf16 results and an fp32 sum of
    # squares that neither overflows nor vanishes
    nz = ref[ref != 0].abs()
    assert nz.numel() == 0 or float(nz.min()) > 2.0 ** -100
    ss = seg.pow(2).sum(dim=-1)
    assert float(ss.max()) < 2.0 ** 100 and float(ss[ss > 0].min()) > 2.0 ** -70
    return NormCase(name="norm[R=%d,D=%d,rows %d..%d]" % (R, D, start, end), x=x, start=start,
                    end=end, ref=ref, zero_rows=zero_rows)


def check_norm(case: NormCase, out: torch.Tensor) -> None:
    """``out`` is the whole tensor after the call."""
    out = out.cpu()
    assert out.dtype == torch.bfloat16 and out.shape == case.x.shape, (case.name, out.dtype, out.shape)
    D = case.x.shape[1]
    s, e = case.start, case.end
    # rows outside the window are untouched, bit for bit
    for lo, hi in ((0, s), (e, case.x.shape[0])):
        if hi > lo and not torch.equal(out[lo:hi].view(torch.int16), case.x[lo:hi].view(torch.int16)):
            r = lo + int((out[lo:hi].view(torch.int16) != case.x[lo:hi].view(torch.int16)).any(dim=1).nonzero()[0])
            raise AssertionError("%s: row %d outside the window changed" % (case.name, r))
    got = out[s:e].double()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % case.name
    err = (got - case.ref).abs()
    lim = norm_bound(D) * case.ref.abs()
    if not bool((err <= lim).all()):
        bad = (err > lim).nonzero()
        r, d = (int(v) for v in bad[0])
        worst = float((err / case.ref.abs().clamp_min(1e-300))[err > lim].max())
        raise AssertionError(
            "%s: out[%d, %d] = %r, float64 reference %r: relative error %.3g > bound %.3g "
            "(%d entries over the bound, worst %.3g)" % (
                case.name, s + r, d, float(got[r, d]), float(case.ref[r, d]),
                float(err[r, d] / case.ref[r, d].abs()), norm_bound(D), bad.shape[0], worst))
    for r in case.zero_rows:
        if s <= r < e:
            assert not bool(out[r].float().any()), "%s: zero row %d is no longer zero" % (case.name, r)
