"""GPU ops: hand-written CDNA4 (gfx950) HIP kernels + CPU references.

Kernels (kakveda_amd/ops/hip/):
- cosine_topk  — fused MFMA-tiled score GEMM (queries x corpus^T) with an
  LDS-resident per-row top-k epilogue per corpus chunk + a merge kernel.
  Replaces the reference's per-request TF-IDF refit + full-corpus cosine
  (/root/reference/services/shared/similarity.py:14-20,
  /root/reference/services/gfkb/app.py:79-102).
- cosine_topk_filtered — the same search with a per-query label predicate
  pushed into the scan (filtered instantiations of the 128x128 list kernel
  and of the streaming small-batch kernel; exact at any selectivity).
- cosine_topk_wide — the exact search for 8 < k <= 64: a k-deep floor from
  the prepass partials, the emission kernels of the k <= 8 search, and a
  block-wide bitonic selection in registers, shuffles and LDS
  (ops/hip/knn_wide_plan.h, knn_wide_impl.h).
- quantize_rows_q8 / cosine_topk_q8 — the optional int8 row mirror: per-row
  symmetric int8 codes with the row's scale and an upper bound of its
  quantisation error, and the exact small-batch search that scans the codes
  (half the bytes), adds the error as a margin and rescores the survivors
  from the bf16 rows (ops/hip/q8_plan.h, q8_impl.h).
- l2normalize_ — in-place row L2-normalisation (bf16, vectorised loads).
- embedding_bag — weighted gather-sum over the hashed-feature table
  (the trace-encoder front end).
- kmeans_assign / kmeans_update — streaming k-means for the pattern
  detector (assignment reuses the score GEMM; update is a segmented
  reduction).
- ivf_route_scores / ivf_scan_topk / ivf_search — the optional cluster-routed
  (IVF) search: centroid scoring, then a gather scan of the probed inverted
  lists plus the rows appended since the index was built (approximate; the
  exact search stays the default). Two scans share one contract: the
  per-query kernel (one block per query, list and slice) and, with
  ``batched=True`` or from IVF_BATCHED_MIN_B queries on, the list-major one
  (ivf_group_probes sorts the (query, probe) pairs by list;
  ivf_scan_grouped_kernel gathers each probed list once per tile of 16
  queries and scores the tile with MFMA).
- ivf_scan_topk_filtered / ivf_search_filtered — the routed search with the
  label predicate of cosine_topk_filtered inside either scan (the
  ``FILTER`` instantiation of the same kernel template), so a filter-first
  request can stay routed.
- featurize_bytes — the optional device featurizer: signature-text bytes to
  the padded index/weight rows of encoder.featurizer.featurize_batch, one
  wave per text (tokenise by ballot, FNV-1a per token, two LDS bitonic
  sorts); rows it cannot take are flagged for the host.

Policy: on a CUDA(ROCm) device the HIP extension is REQUIRED — ops raise
if it is missing rather than silently falling back to eager PyTorch. The
torch fallbacks exist for CPU (tests, BASELINE config 1) only.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

_EXT = None
_EXT_ERR: Optional[str] = None


def _load_extension():
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        import importlib

        _EXT = importlib.import_module("kakveda_amd.ops._kakveda_hip")
    except ImportError as exc:  # pragma: no cover - exercised on GPU boxes
        _EXT_ERR = str(exc)
        _EXT = None
    return _EXT


def hip_available() -> bool:
    return _load_extension() is not None


def _require_ext():
    ext = _load_extension()
    if ext is None:
        raise RuntimeError(
            "kakveda_amd HIP extension (_kakveda_hip) is not built but a GPU "
            "op was requested on a CUDA device. Build it in-tree with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). "
            f"Import error: {_EXT_ERR}"
        )
    return ext


# ---------------------------------------------------------------------------
# cosine top-k
# ---------------------------------------------------------------------------

#: per-row candidate capacity of the fused HIP kernel (kakveda_kernels.hip)
KMAX = 8

def cosine_topk(
    queries: torch.Tensor, corpus: torch.Tensor, k: int, valid_n: Optional[int] = None
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k inner products of each query row against every corpus row.

    queries: [B, D], corpus: [N, D]; rows are expected pre-normalised so the
    inner product is the cosine. Returns (scores f32 [B, k], idx i64 [B, k])
    sorted descending per row. ``valid_n`` limits the search to the first
    valid_n corpus rows (the live prefix of a preallocated store).

    The HIP kernel keeps at most KMAX=8 candidates per row; a request with
    k > 8 on GPU returns the true top-8 padded with (-inf, -1) so CPU and
    GPU agree on the leading 8 columns instead of the GPU path raising.

    Precondition of exactness on GPU: unit rows (|q| = |c| = 1 up to bf16
    rounding). The streaming kernels (B <= 8, N >= 64k) admit a row when its
    score clears the emission floor lowered by D * 2^-22, the bound on how
    far two fp32 summation orders of one unit-row inner product can differ;
    rows of larger norm can exceed it and lose a match that sits on the
    floor. Equal scores are all eligible members of the result (k distinct
    indices); which of them are returned, and in what order, is unspecified.
    """
    n = int(valid_n) if valid_n is not None else corpus.shape[0]
    B = queries.shape[0]
    if n <= 0:
        return (
            torch.full((B, k), float("-inf"), dtype=torch.float32, device=queries.device),
            torch.full((B, k), -1, dtype=torch.int64, device=queries.device),
        )
    if queries.device.type == "cuda":
        ext = _require_ext()
        kk = min(int(k), KMAX)
        scores, idx = ext.cosine_topk(queries, corpus, kk, n)
        if kk < k:
            pad_s = torch.full((B, k - kk), float("-inf"), dtype=scores.dtype, device=scores.device)
            pad_i = torch.full((B, k - kk), -1, dtype=idx.dtype, device=idx.device)
            scores = torch.cat([scores, pad_s], dim=1)
            idx = torch.cat([idx, pad_i], dim=1)
        return scores, idx
    return cosine_topk_ref(queries, corpus, k, n)


def cosine_topk_ref(
    queries: torch.Tensor, corpus: torch.Tensor, k: int, valid_n: Optional[int] = None
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain-PyTorch reference (fp32 accumulate), used on CPU and in tests."""
    n = int(valid_n) if valid_n is not None else corpus.shape[0]
    kk = min(k, n)
    sims = queries.float() @ corpus[:n].float().t()
    scores, idx = torch.topk(sims, kk, dim=1)
    if kk < k:
        pad_s = torch.full((queries.shape[0], k - kk), float("-inf"), device=queries.device)
        pad_i = torch.full((queries.shape[0], k - kk), -1, dtype=idx.dtype, device=queries.device)
        scores = torch.cat([scores, pad_s], dim=1)
        idx = torch.cat([idx, pad_i], dim=1)
    return scores.float(), idx.long()


def cosine_topk_filtered(
    queries: torch.Tensor,
    corpus: torch.Tensor,
    labels: torch.Tensor,
    want: torch.Tensor,
    k: int,
    valid_n: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``cosine_topk`` with a per-query label predicate pushed into the scan.

    labels: int32 [N], one per corpus row (-1 = unlabelled); want: int32 [B],
    one per query. Corpus row j is eligible for query b iff
    ``want[b] < 0 or labels[j] == want[b]``, so a batch may mix filtered and
    unfiltered queries. Returns (scores f32 [B, k], idx i64 [B, k]) sorted
    descending; a query with fewer than k eligible rows is padded with
    (-inf, -1), as is everything past KMAX columns on GPU.

    The search is exact whatever the selectivity: the kernels mask
    ineligible rows before any pruning threshold is formed (see
    ops/hip/kernels_impl.h), they do not over-fetch and post-filter.
    """
    n = int(valid_n) if valid_n is not None else corpus.shape[0]
    B = queries.shape[0]
    if n <= 0:
        return (
            torch.full((B, k), float("-inf"), dtype=torch.float32, device=queries.device),
            torch.full((B, k), -1, dtype=torch.int64, device=queries.device),
        )
    if queries.device.type != "cuda":
        return cosine_topk_filtered_ref(queries, corpus, labels, want, k, n)
    ext = _require_ext()
    kk = min(int(k), KMAX)
    scores, idx = ext.cosine_topk_filtered(
        queries,
        corpus,
        labels.to(device=corpus.device, dtype=torch.int32).contiguous(),
        want.to(device=queries.device, dtype=torch.int32).contiguous(),
        kk,
        n,
    )
    # empty slots leave the kernels as (-1e30 or -inf, -1): one sentinel out
    scores = torch.where(idx < 0, torch.full_like(scores, float("-inf")), scores)
    if kk < k:
        pad_s = torch.full((B, k - kk), float("-inf"), dtype=scores.dtype, device=scores.device)
        pad_i = torch.full((B, k - kk), -1, dtype=idx.dtype, device=idx.device)
        scores = torch.cat([scores, pad_s], dim=1)
        idx = torch.cat([idx, pad_i], dim=1)
    return scores, idx


def cosine_topk_filtered_ref(
    queries: torch.Tensor,
    corpus: torch.Tensor,
    labels: torch.Tensor,
    want: torch.Tensor,
    k: int,
    valid_n: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain-PyTorch reference of ``cosine_topk_filtered`` (fp32 accumulate):
    ineligible columns are scored -inf, and whatever of them reaches the
    top-k of a sparsely populated label is reported as a pad, never as an
    index of a masked row."""
    n = int(valid_n) if valid_n is not None else corpus.shape[0]
    B = queries.shape[0]
    kk = min(k, n)
    sims = queries.float() @ corpus[:n].float().t()
    lab = labels[:n].to(sims.device).long()
    w = want.to(sims.device).long()
    eligible = (w[:, None] < 0) | (lab[None, :] == w[:, None])
    sims = sims.masked_fill(~eligible, float("-inf"))
    scores, idx = torch.topk(sims, kk, dim=1)
    idx = torch.where(torch.isinf(scores) & (scores < 0), torch.full_like(idx, -1), idx)
    if kk < k:
        pad_s = torch.full((B, k - kk), float("-inf"), device=queries.device)
        pad_i = torch.full((B, k - kk), -1, dtype=idx.dtype, device=queries.device)
        scores = torch.cat([scores, pad_s], dim=1)
        idx = torch.cat([idx, pad_i], dim=1)
    return scores.float(), idx.long()


# ---------------------------------------------------------------------------
# wide exact top-k: KMAX < k <= KWIDE_MAX
# ---------------------------------------------------------------------------

#: most results per query of ``cosine_topk_wide`` (knn_wide_plan.h KWIDE_MAX)
KWIDE_MAX = 64

#: batches of ``cosine_topk_wide`` whose candidates overflowed their buffer and
#: were answered slice by slice instead (a process-wide counter)
wide_overflow_fallbacks = 0


def _wide_ext():
    ext = _require_ext()
    if int(ext.KWIDE_MAX) != KWIDE_MAX:
        raise RuntimeError(
            f"ops.KWIDE_MAX = {KWIDE_MAX} but the built extension has "
            f"KWIDE_MAX = {int(ext.KWIDE_MAX)}: rebuild it"
        )
    return ext


def cosine_topk_wide(
    queries: torch.Tensor,
    corpus: torch.Tensor,
    k: int,
    valid_n: Optional[int] = None,
    labels: Optional[torch.Tensor] = None,
    want: Optional[torch.Tensor] = None,
    cap: Optional[int] = None,
    seg: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k for k up to ``KWIDE_MAX`` = 64: ``cosine_topk`` (or, with
    ``labels``/``want``, ``cosine_topk_filtered``) without the KMAX clamp.

    Returns (scores f32 [B, k], idx i64 [B, k]), score descending (on a GPU,
    among equal scores, index ascending); ranks past the eligible rows are
    (-inf, -1). On a GPU ``k <= KMAX`` is answered by ``cosine_topk`` /
    ``cosine_topk_filtered`` as they are, and ``k > KWIDE_MAX`` returns the top
    ``KWIDE_MAX`` padded, the convention of ``cosine_topk``. On a CPU it is the
    plain-torch reference at any k.

    The GPU path (ops/hip/knn_wide_plan.h) takes per query the k-th largest
    partial of an 8-deep prepass over a prefix of the corpus as a floor, emits
    every row at or above it with the kernels of the k <= 8 search, and selects
    the top k of those in LDS. It scans the whole corpus once for B <= 8
    (streaming kernel) and for unfiltered batches (8-phase MFMA kernel); a
    filtered batch of more than 8 queries, and any batch over fewer than 4,096
    rows, is served in groups of 8 queries, each group reading the corpus
    again. Unit rows are the precondition, as for ``cosine_topk``.

    ``cap`` (candidates per query; default KAKVEDA_KNN_EMIT_CAP, 32,768) and
    ``seg`` (records per block segment of the 8-phase launch) are for tests and
    measurements. A batch that overflows either is answered exactly over
    consecutive corpus slices of ``cap`` rows and counted in
    ``wide_overflow_fallbacks``.
    """
    global wide_overflow_fallbacks
    if (labels is None) != (want is None):
        raise ValueError("labels and want go together")
    n = int(valid_n) if valid_n is not None else corpus.shape[0]
    B = queries.shape[0]
    k = int(k)
    if n <= 0 or B == 0:
        return (
            torch.full((B, k), float("-inf"), dtype=torch.float32, device=queries.device),
            torch.full((B, k), -1, dtype=torch.int64, device=queries.device),
        )
    if queries.device.type != "cuda":
        if labels is None:
            return cosine_topk_ref(queries, corpus, k, n)
        return cosine_topk_filtered_ref(queries, corpus, labels, want, k, n)
    if k <= KMAX:
        if labels is None:
            return cosine_topk(queries, corpus, k, n)
        return cosine_topk_filtered(queries, corpus, labels, want, k, n)
    ext = _wide_ext()
    kk = min(k, KWIDE_MAX)
    scores, idx, fallback = ext.cosine_topk_wide(
        queries,
        corpus,
        kk,
        n,
        None if labels is None else labels.to(device=corpus.device, dtype=torch.int32).contiguous(),
        None if want is None else want.to(device=queries.device, dtype=torch.int32).contiguous(),
        int(cap or 0),
        int(seg or 0),
    )
    wide_overflow_fallbacks += int(fallback == 1)
    # one sentinel out, as cosine_topk_filtered
    scores = torch.where(idx < 0, torch.full_like(scores, float("-inf")), scores)
    if kk < k:
        pad_s = torch.full((B, k - kk), float("-inf"), dtype=scores.dtype, device=scores.device)
        pad_i = torch.full((B, k - kk), -1, dtype=idx.dtype, device=idx.device)
        scores = torch.cat([scores, pad_s], dim=1)
        idx = torch.cat([idx, pad_i], dim=1)
    return scores, idx


# ---------------------------------------------------------------------------
# int8 row mirror: quantiser and the two-stage exact small-batch search
# ---------------------------------------------------------------------------

#: codes per 128-byte segment of a mirror row; D must be a multiple of it
#: (mirror of q8_plan.h Q8_SEG)
Q8_SEG = 128
#: rows with a smaller amax are stored as zeros (q8_plan.h Q8_MIN_AMAX)
_Q8_MIN_AMAX = 2.0 ** -100
#: additive part of the stored error and of qn (q8_plan.h Q8_ERR_ABS)
_Q8_ERR_ABS = 2.0 ** -50
#: candidates per query of the emission path (knn_plan.h KnnEnv.cap)
_Q8_CAP = 32768

#: Largest batch at which ``EmbeddingStore.search`` takes the int8 mirror: the
#: largest B at which the q8 arm of benchmarks/q8_scan_bench.py beat the bf16
#: arm by more than both arms' spread in every cell (profiles/q8_mirror.md:
#: D=768, k=5, mixture and isotropic corpus, unfiltered and a 10% label). At
#: 10M rows it wins at every B (1.43-1.48x at B=1, 1.27-1.33x at 2,
#: 1.11-1.12x at 4, 1.06-1.09x at 8); at 1M rows 1.09-1.10x, 1.06-1.07x and
#: 1.02-1.03x (spread <= 0.7%) at B=1, 2, 4, and 0.99-1.00x at B=8: a loss.
Q8_MAX_B = 4

#: largest D of the batched int8 screen (q8_plan.h Q8_SCREEN_MAX_D: the int32
#: dot of the codes must convert to fp32 exactly)
Q8_SCREEN_MAX_D = 1024

#: Smallest batch at which ``EmbeddingStore.search`` and ``cosine_topk_q8``
#: screen the 8-phase emission scan with int8 (``q8_batch_in_plan``): the
#: smallest B of the sweep (profiles/q8_batch_screen.md: D=768, k=5, isotropic
#: rows and queries, both arms alternating in one process, 8 timings each). At
#: 10M rows the int8 arm wins at every B measured: 1.41x at B=16 and 32, 1.33x
#: at 64, 1.30x at 128, 1.24x at 256, 1.26x at 512, 1.30x at 1024, 1.32x at
#: 2048, with both arms' spread under 3.5% (one 11% outlier at B=16). Batches
#: of 9..15 queries were not measured; they pay the same single 256-row tile.
Q8_BATCH_MIN_B = 16

#: Fewest rows (of one store segment) at which they do so. With the screen's
#: floors raised between stages (profiles/q8_staged_floors.md) bench.py
#: (correlated queries, B=2048, three alternating runs per arm) runs 7.03-7.12
#: ms/step with the int8 arm against 9.36-9.58 on bf16 at 2.5M rows, and
#: 4.60-4.63 against 5.02-5.14 at 1.25M: 1.32x and 1.10x, beyond both arms'
#: spread. Before the stages the int8 arm lost 6% and 11% there and the gate
#: stood at 8M rows. The earlier sweep at 1.25M rows (one stage, isotropic
#: queries) had the int8 arm at 1.03-1.07x up to B=1024, inside the bf16 arm's
#: spread: not a loss. Smaller shards were not measured; the value sits just
#: below the smallest size measured to win.
Q8_BATCH_MIN_ROWS = 1_200_000

#: batches of the batched screen that held a query quantised to zeros and were
#: answered by the bf16 search (a process-wide counter)
q8_degenerate_fallbacks = 0

#: batches that overflowed the candidate buffer of the q8 path and were
#: answered by the bf16 search instead (a process-wide counter)
q8_overflow_fallbacks = 0


def _q8_check_dim(D: int) -> None:
    if D < Q8_SEG or D % Q8_SEG != 0:
        raise ValueError(
            f"the int8 mirror needs D to be a multiple of {Q8_SEG}, got D = {D}"
        )


def _q8_roundup(D: int) -> float:
    """Factor that rounds an fp32 norm of D terms up past its real value
    (derived in q8_plan.h)."""
    return 1.0 + (D + 16) * 2.0 ** -24


def quantize_rows_q8_ref(
    rows: torch.Tensor, out_codes: torch.Tensor, out_meta: torch.Tensor, first_row: int = 0
) -> None:
    """Reference of ``quantize_rows_q8`` in torch, to the contract of
    q8_plan.h: per row ``amax = max|c_i|``, ``scale = amax / 127`` and
    ``inv = 127 / amax`` in fp32, ``n_i = clamp(round_half_even(c_i * inv),
    -127, 127)`` from one fp32 multiply, and ``err >= ||c - scale * n||``
    (here: the float64 norm, rounded up by the kernel's factor). Codes and
    scales are bit-equal to the kernel's; ``err`` obeys the same bound."""
    n, D = int(rows.shape[0]), int(rows.shape[1])
    _q8_check_dim(D)
    if n == 0:
        return
    x = rows.detach().float().cpu()
    amax = x.abs().amax(dim=1)
    amax = torch.where(torch.isnan(amax), torch.zeros_like(amax), amax)
    livef = amax >= _Q8_MIN_AMAX
    safe = torch.where(livef, amax, torch.ones_like(amax))
    # tensor / tensor: a Python scalar on the left would be computed as
    # reciprocal(safe) * 127, two roundings where the contract has one
    c127 = torch.full_like(safe, 127.0)
    scale = torch.where(livef, safe / c127, torch.zeros_like(amax))
    inv = torch.where(livef, c127 / safe, torch.zeros_like(amax))
    codes = torch.round(x * inv[:, None]).clamp_(-127.0, 127.0)
    codes = torch.where(torch.isnan(codes), torch.zeros_like(codes), codes)
    resid = (x.double() - scale.double()[:, None] * codes.double()).norm(dim=1)
    err = torch.where(
        livef,
        resid * _q8_roundup(D) + _Q8_ERR_ABS,
        amax.double() * (D ** 0.5) * _q8_roundup(D) * (1.0 + 2.0 ** -20),
    )
    # the cast rounds to nearest: step up where it landed below
    err32 = err.float()
    err32 = torch.where(err32.double() < err, torch.nextafter(err32, err32.new_tensor(float("inf"))), err32)
    sl = slice(int(first_row), int(first_row) + n)
    out_codes[sl] = codes.to(torch.int8).to(out_codes.device)
    out_meta[sl] = torch.stack([scale, err32], dim=1).to(out_meta.device)


def q8_cnorm_ref(rows: torch.Tensor) -> torch.Tensor:
    """Reference of the ``cnorm`` of ``rows``: fp32 [1], at least the largest
    row norm (the float64 norm, rounded up by the kernel's factor; 0 for no
    rows)."""
    n, D = int(rows.shape[0]), int(rows.shape[1])
    if n == 0:
        return torch.zeros(1, dtype=torch.float32)
    top = rows.detach().double().cpu().norm(dim=1).max() * _q8_roundup(D) + _Q8_ERR_ABS
    t32 = top.float()
    if t32.double() < top:
        t32 = torch.nextafter(t32, t32.new_tensor(float("inf")))
    return t32.reshape(1)


def new_q8_cnorm(device) -> torch.Tensor:
    """A fresh ``cnorm`` scalar (fp32 [1], 0: no rows yet) for one mirror."""
    return torch.zeros(1, dtype=torch.float32, device=device)


def quantize_rows_q8(
    rows: torch.Tensor,
    out_codes: torch.Tensor,
    out_meta: torch.Tensor,
    first_row: int = 0,
    cnorm: Optional[torch.Tensor] = None,
) -> None:
    """Quantise ``rows`` [n, D] into the int8 mirror: codes int8 go to
    ``out_codes[first_row : first_row + n]`` ([*, D]) and (scale, err) fp32
    pairs to ``out_meta[first_row : first_row + n]`` ([*, 2]), where
    ``scale * codes`` approximates the row and ``err`` is an upper bound of
    the L2 norm of what it misses (contract: ops/hip/q8_plan.h). ``cnorm``
    (fp32 [1], ``new_q8_cnorm``) is raised to at least the largest norm of
    these rows: the mirror's scalar the batched screen needs. D must be a
    multiple of Q8_SEG. GPU: HIP kernels over bf16 rows; CPU: the reference."""
    _q8_check_dim(int(rows.shape[1]))
    if rows.device.type == "cuda":
        _require_ext().quantize_rows_q8(
            rows.contiguous(), out_codes, out_meta, int(first_row), cnorm
        )
        return
    quantize_rows_q8_ref(rows, out_codes, out_meta, first_row)
    if cnorm is not None:
        torch.maximum(cnorm, q8_cnorm_ref(rows).to(cnorm.device), out=cnorm)


def new_q8_mirror(n: int, D: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Empty mirror tensors for ``n`` rows: (codes int8 [n, D], meta f32 [n, 2])."""
    _q8_check_dim(int(D))
    return (
        torch.zeros(n, D, dtype=torch.int8, device=device),
        torch.zeros(n, 2, dtype=torch.float32, device=device),
    )


def q8_in_plan(B: int, N: int, k: int, filtered: bool) -> bool:
    """Whether the default dispatch plan (knn_plan.h plan_cosine_topk) gives
    this request to the streaming small-batch kernel, which is where
    ``cosine_topk_q8`` scans the mirror: N >= 65,536 and B <= 8, and k > 1 on
    the unfiltered table."""
    return N >= 65536 and B <= 8 and (filtered or k > 1)


def _q8_batch_env() -> bool:
    """KAKVEDA_Q8_BATCH as the extension reads it (knn_plan.h parse_knn_env):
    unset or 1 is on, 0 forces the bf16 path, anything else is refused."""
    v = os.environ.get("KAKVEDA_Q8_BATCH", "")
    if v in ("", "1"):
        return True
    if v == "0":
        return False
    raise ValueError(
        f"KAKVEDA_Q8_BATCH='{v}' is not a setting; accepted: 1 (default: "
        "cosine_topk_q8 screens batches with int8), 0 (it answers them with "
        "the bf16 search)"
    )


def q8_batch_in_plan(
    B: int,
    N: int,
    k: int,
    D: int,
    filtered: bool,
    min_b: Optional[int] = None,
    min_rows: Optional[int] = None,
) -> bool:
    """Whether ``cosine_topk_q8`` screens this request with int8 in the place
    of the 8-phase bf16 emission scan: unfiltered, N >= 65,536, k > 1, more
    queries than the streaming kernel takes and at least ``min_b`` (default
    ``Q8_BATCH_MIN_B``), at least ``min_rows`` rows (default
    ``Q8_BATCH_MIN_ROWS``), D a multiple of Q8_SEG up to Q8_SCREEN_MAX_D, and
    KAKVEDA_Q8_BATCH not 0. The two defaults are speed thresholds: the path is
    exact wherever the other conditions hold."""
    floor_b = Q8_BATCH_MIN_B if min_b is None else int(min_b)
    floor_n = Q8_BATCH_MIN_ROWS if min_rows is None else int(min_rows)
    return (
        not filtered
        and N >= 65536
        and N >= floor_n
        and k > 1
        and B > 8
        and floor_b > 0
        and B >= floor_b
        and D >= Q8_SEG
        and D % Q8_SEG == 0
        and D <= Q8_SCREEN_MAX_D
        and _q8_batch_env()
    )


def _q8_sample_rows(N: int, filtered: bool, B: int = 1) -> int:
    """Rows the emission prepass of a request samples under the default plan
    (knn_plan.h: preg sampled chunks of PRE_TILES 128-column tiles), for the
    reference's floors. ``B`` matters above 8 queries, where the chunking is
    the 8-phase kernel's over ceil(B / 256) row tiles."""
    tile, target = (128, 2048) if filtered else (256, 512)
    ntiles = -(-N // tile)
    row_tiles = -(-B // tile)
    chunk_tiles = max(4, min(-(-ntiles * row_tiles // target), 128))
    nchunks = (-(-ntiles // chunk_tiles) + 7) & ~7
    preg = min(256, nchunks) & ~7
    return min(N, preg * 8 * 128)


def q8_scores_ref(queries: torch.Tensor, codes: torch.Tensor, meta: torch.Tensor) -> torch.Tensor:
    """fp32 stage-1 scores ``scale_r * sum_i q_i n_i`` of every (query, row)."""
    return (queries.float() @ codes.float().t()) * meta[:, 0][None, :]


def q8_emit_mask_ref(
    queries: torch.Tensor,
    corpus: torch.Tensor,
    codes: torch.Tensor,
    meta: torch.Tensor,
    valid_n: int,
    labels: Optional[torch.Tensor] = None,
    want: Optional[torch.Tensor] = None,
    margin: bool = True,
) -> torch.Tensor:
    """Stages 0 and 1 of ``cosine_topk_q8_ref``: bool [B, valid_n], the rows
    emitted for each query. Stage 0: the floor of query b is the 8th best
    fp32 score over the eligible rows among the first ``_q8_sample_rows``
    (none with fewer than 8), lowered by D * 2^-22. Stage 1: row r is emitted
    iff it is eligible and ``scale_r * q.n_r + qn_b * err_r + D * 2^-22 >=
    floor``. ``margin=False`` drops the ``qn * err`` term: the broken search
    the tests show the planted input to catch."""
    n = int(valid_n)
    D = int(queries.shape[1])
    q = queries.float()
    filtered = want is not None
    elig = torch.ones(q.shape[0], n, dtype=torch.bool, device=q.device)
    if filtered:
        w = want.to(q.device).long()[:, None]
        elig = (w < 0) | (labels[:n].to(q.device).long()[None, :] == w)
    ns = _q8_sample_rows(n, filtered)
    samp = (q @ corpus[:ns].float().t()).masked_fill(~elig[:, :ns], float("-inf"))
    kth = torch.topk(samp, min(KMAX, ns), dim=1).values[:, -1] if ns >= KMAX else samp.new_full(
        (q.shape[0],), float("-inf"))
    slack = D * 2.0 ** -22
    floor = kth - slack
    s8 = q8_scores_ref(q, codes[:n], meta[:n])
    if margin:
        qn = (q.double().norm(dim=1) * _q8_roundup(D) + _Q8_ERR_ABS).float()
        s8 = s8 + qn[:, None] * meta[:n, 1][None, :]
    return elig & (s8 + slack >= floor[:, None])


def q8_screen_params_ref(
    queries: torch.Tensor, floors: torch.Tensor, cnorm: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """The per-call side of the batched screen (q8_plan.h "Screening test"),
    in torch: the queries quantised by the corpus quantiser, ``T`` fp32 [B]
    (``q8_screen_threshold`` of each row's ``floors`` entry, evaluated in fp32
    step by step), ``kappa`` fp32 [1] (the largest ``q8_screen_kappa``) and
    the number of degenerate queries (scale 0: their T is +1e38). Returns
    (qcodes int8 [B, D] on the CPU, T, kappa, degenerate)."""
    B, D = int(queries.shape[0]), int(queries.shape[1])
    qcodes = torch.zeros(B, D, dtype=torch.int8)
    qmeta = torch.zeros(B, 2, dtype=torch.float32)
    quantize_rows_q8_ref(queries, qcodes, qmeta)
    sq, errq = qmeta[:, 0], qmeta[:, 1]
    live = sq > 0
    safe = torch.where(live, sq, torch.ones_like(sq))
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    up = f32(_q8_roundup(D))
    sumsq = (qcodes.long() ** 2).sum(dim=1).float()
    nqh = safe * torch.sqrt(sumsq) * up + f32(_Q8_ERR_ABS)
    kap = (nqh / safe) * f32(1.0 + 2.0 ** -22)
    kappa = torch.where(live, kap, torch.zeros_like(kap)).max().reshape(1)
    slack = f32(D * 2.0 ** -22)
    fl = floors.detach().float().cpu()
    e = errq * cnorm.detach().float().cpu().reshape(()) * f32(1.0 + 2.0 ** -22)
    mag = fl.abs() + e + slack
    num = fl - e - slack - mag * f32(2.0 ** -21)
    t = num / safe
    t = t - t.abs() * f32(2.0 ** -22)
    T = torch.where(live, t, torch.full_like(t, 1e38))
    return qcodes, T, kappa, int((~live).sum())


def q8_screen_mask_ref(
    qcodes: torch.Tensor,
    codes: torch.Tensor,
    meta: torch.Tensor,
    T: torch.Tensor,
    kappa: torch.Tensor,
    valid_n: int,
    band: bool = False,
):
    """The batched screen's candidate mask in torch: bool [B, valid_n], true
    where ``v = acc * scale_c + kappa * err_c >= T_r`` with ``acc`` the exact
    dot of the codes (q8_plan.h q8_screen_fast; the kernel rounds v once, here
    it is formed in float64 from the fp32 product ``kappa * err_c``). With
    ``band`` also the pairs whose v lies within one fp32 rounding of T_r, where
    the kernel's single rounding may decide either way."""
    n = int(valid_n)
    dev = codes.device
    # products and partial sums are integers below 2^24: exact in fp32
    acc = qcodes.to(dev).float() @ codes[:n].float().t()
    ke = (kappa.to(dev).float().reshape(()) * meta[:n, 1]).double()
    v = acc.double() * meta[:n, 0].double()[None, :] + ke[None, :]
    Td = T.to(dev).double()[:, None]
    mask = v >= Td
    if not band:
        return mask
    near = (v - Td).abs() <= torch.maximum(v.abs(), Td.abs()) * 2.0 ** -23
    return mask, near


def _q8_batch_ref(queries, corpus, codes, meta, cnorm, k, n):
    """The batched path of ``cosine_topk_q8_ref``: (scores, idx), or None when
    the batch falls back (and which counter it bumped)."""
    global q8_overflow_fallbacks, q8_degenerate_fallbacks
    B = queries.shape[0]
    q = queries.float()
    ns = _q8_sample_rows(n, False, B)
    samp = q @ corpus[:ns].float().t()
    seeds = torch.topk(samp, min(KMAX, ns), dim=1)
    floors = seeds.values[:, -1] if ns >= KMAX else samp.new_full((B,), -1e30)
    if cnorm is None:
        cnorm = q8_cnorm_ref(corpus[:n])
    qcodes, T, kappa, degenerate = q8_screen_params_ref(queries, floors, cnorm)
    if degenerate:
        q8_degenerate_fallbacks += 1
        return None
    mask = q8_screen_mask_ref(qcodes, codes, meta, T, kappa, n).to(q.device)
    if ns < n:
        # the main launch starts after the sample; its top-KMAX are seeded
        mask[:, :ns] = False
        mask[:, :ns].scatter_(1, seeds.indices, True)
    if int(mask.sum(dim=1).max()) > _Q8_CAP:
        q8_overflow_fallbacks += 1
        return None
    sims = (q @ corpus[:n].float().t()).masked_fill(~mask, float("-inf"))
    scores, idx = torch.topk(sims, min(k, n), dim=1)
    idx = torch.where(torch.isinf(scores) & (scores < 0), torch.full_like(idx, -1), idx)
    return _pad_topk(scores.float(), idx.long(), k)


def cosine_topk_q8_ref(
    queries: torch.Tensor,
    corpus: torch.Tensor,
    codes: torch.Tensor,
    meta: torch.Tensor,
    k: int,
    valid_n: Optional[int] = None,
    labels: Optional[torch.Tensor] = None,
    want: Optional[torch.Tensor] = None,
    cnorm: Optional[torch.Tensor] = None,
    batch_min_b: Optional[int] = None,
    batch_min_rows: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``cosine_topk_q8`` in torch (fp32 accumulate): floors from the sampled
    rows, emission from the int8 mirror with each row's error margin
    (``q8_emit_mask_ref``), exact scores of the emitted rows from ``corpus``,
    top-k of those. A query with more than the candidate buffer's capacity
    of emitted rows sends the batch to the plain reference search and bumps
    ``q8_overflow_fallbacks``, as on the GPU. A request of the batched screen
    (``q8_batch_in_plan``) takes that path's reference: floors and seeds from
    the sample, ``q8_screen_mask_ref`` over the rest, exact scores of the
    survivors. Other requests outside ``q8_in_plan`` run the plain reference
    search."""
    global q8_overflow_fallbacks
    n = int(valid_n) if valid_n is not None else corpus.shape[0]
    B = queries.shape[0]
    _q8_check_dim(int(queries.shape[1]))
    filtered = want is not None

    def plain():
        if filtered:
            return cosine_topk_filtered_ref(queries, corpus, labels, want, k, n)
        return cosine_topk_ref(queries, corpus, k, n)

    if n > 0 and q8_batch_in_plan(
        B, n, min(int(k), KMAX), int(queries.shape[1]), filtered, batch_min_b,
        batch_min_rows,
    ):
        got = _q8_batch_ref(queries, corpus, codes, meta, cnorm, k, n)
        return plain() if got is None else got
    if n <= 0 or not q8_in_plan(B, n, min(int(k), KMAX), filtered):
        return plain()
    mask = q8_emit_mask_ref(queries, corpus, codes, meta, n, labels, want)
    if int(mask.sum(dim=1).max()) > _Q8_CAP:
        q8_overflow_fallbacks += 1
        return plain()
    sims = (queries.float() @ corpus[:n].float().t()).masked_fill(~mask, float("-inf"))
    kk = min(k, n)
    scores, idx = torch.topk(sims, kk, dim=1)
    idx = torch.where(torch.isinf(scores) & (scores < 0), torch.full_like(idx, -1), idx)
    return _pad_topk(scores.float(), idx.long(), k)


def q8_cnorm(rows: torch.Tensor) -> torch.Tensor:
    """``cnorm`` of ``rows`` (fp32 [1] on their device): at least their largest
    L2 norm. One pass over the rows; a store keeps it beside its mirror."""
    if rows.device.type != "cuda":
        return q8_cnorm_ref(rows)
    D = int(rows.shape[1])
    _q8_check_dim(D)
    out = new_q8_cnorm(rows.device)
    # the quantiser's companion kernel, without keeping the codes
    codes, meta = new_q8_mirror(min(int(rows.shape[0]), 1 << 16), D, rows.device)
    for a in range(0, int(rows.shape[0]), 1 << 16):
        b = min(a + (1 << 16), int(rows.shape[0]))
        _require_ext().quantize_rows_q8(rows[a:b].contiguous(), codes, meta, 0, out)
    return out


#: most stages of the batched screen's main launch (knn_plan.h Q8_MAX_STAGES)
Q8_MAX_STAGES = 4


def _q8_stages_arg(stages: Optional[int]) -> int:
    """``stages`` as the extension takes it: 0 for None (the plan's rule)."""
    if stages is None:
        return 0
    n = int(stages)
    if not 1 <= n <= Q8_MAX_STAGES:
        raise ValueError(f"stages must be in [1, {Q8_MAX_STAGES}] or None, got {stages}")
    return n


def q8_stage_plan(B: int, N: int, k: int, stages: Optional[int] = None):
    """The stage plan of the batched screen for a request of ``B`` queries over
    ``N`` rows (knn_plan.h ``plan_q8_stages``; host only, no GPU needed): a
    dict with ``first`` (n + 1 bounds in 256-row tiles: stage i scans the rows
    ``[256 * first[i], min(N, 256 * first[i + 1]))``), ``chunk_tiles`` and
    ``nchunks`` (n each: the stage's launch geometry). ``first[0]`` rows are
    left to the prepass sample."""
    first, chunk_tiles, nchunks = _require_ext().q8_stage_plan(
        int(B), int(N), min(int(k), KMAX), _q8_stages_arg(stages)
    )
    return dict(first=list(first), chunk_tiles=list(chunk_tiles), nchunks=list(nchunks))


def q8_screen_probe(
    queries: torch.Tensor,
    corpus: torch.Tensor,
    codes: torch.Tensor,
    meta: torch.Tensor,
    cnorm: torch.Tensor,
    k: int,
    valid_n: Optional[int] = None,
    cap: Optional[int] = None,
):
    """The batched screen up to the merge, on the GPU: a dict with ``counts``
    and ``first`` (i32 [B]: entries per row, and how many of them are seeds),
    ``before`` and ``after`` (i64 [B, cap]: the candidate lists ahead of and
    behind the rescore, packed ``enc(score) << 32 | 0x7fffffff - column``),
    ``T`` (fp32 [B]), ``kappa`` (fp32 [1]) and ``floors`` (fp32 [B], the
    prepass floors)."""
    n = int(valid_n) if valid_n is not None else corpus.shape[0]
    counts, first, before, after, T, kappa, rowthr = _require_ext().q8_screen_probe(
        queries, corpus, codes, meta, cnorm, min(int(k), KMAX), n, int(cap or 0)
    )
    return dict(counts=counts, first=first, before=before, after=after, T=T,
                kappa=kappa, floors=_dec_f32(rowthr.long() & 0xFFFFFFFF))


def _dec_f32(u: torch.Tensor) -> torch.Tensor:
    """kernels_impl.h dec_f32 on order-encoded words held in int64."""
    bits = torch.where(u >= 2 ** 31, u ^ 0x80000000, ~u & 0xFFFFFFFF)
    bits = bits - ((bits >= 2 ** 31).long() << 32)  # as signed 32-bit
    return bits.to(torch.int32).view(torch.float32)


def q8_unpack(entries: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores fp32, columns i64) of packed candidate entries (i64)."""
    return _dec_f32((entries >> 32) & 0xFFFFFFFF), 0x7FFFFFFF - (entries & 0xFFFFFFFF)


def cosine_topk_q8(
    queries: torch.Tensor,
    corpus: torch.Tensor,
    codes: torch.Tensor,
    meta: torch.Tensor,
    k: int,
    valid_n: Optional[int] = None,
    labels: Optional[torch.Tensor] = None,
    want: Optional[torch.Tensor] = None,
    cnorm: Optional[torch.Tensor] = None,
    batch_min_b: Optional[int] = None,
    cap: Optional[int] = None,
    batch_min_rows: Optional[int] = None,
    stages: Optional[int] = None,
    return_counts: bool = False,
):
    """``cosine_topk`` (``cosine_topk_filtered`` when ``labels``/``want`` are
    given) that reads the int8 mirror of the corpus where the request is one
    of the streaming small-batch kernel's (``q8_in_plan``): the scan over all
    rows reads ``codes``/``meta`` (``quantize_rows_q8`` of ``corpus``: D + 8
    bytes a row against 2D), emits every row whose int8 score plus its known
    quantisation error could reach the emission floor, and the emitted rows
    are scored again from the bf16 ``corpus``. The result is exact - the
    candidates are a superset of the bf16 scan's and carry its scores. Every
    other request runs the bf16 search unchanged, and so does a batch whose
    candidates overflow their buffer (``q8_overflow_fallbacks`` counts them).
    Shapes, padding and the KMAX clamp as ``cosine_topk``/``_filtered``; D
    must be a multiple of Q8_SEG.

    Batches (``q8_batch_in_plan``: the unfiltered 8-phase emission request
    with at least ``batch_min_b`` queries and ``batch_min_rows`` rows, default
    ``Q8_BATCH_MIN_B`` and ``Q8_BATCH_MIN_ROWS``) are
    screened instead: the emission kernel runs on int8 codes of queries and
    rows with ``v_mfma_i32_16x16x64_i8``, every (query, row) whose int8 score
    plus the known errors of both sides could reach the prepass floor is
    rescored with the bf16 kernel's own MFMA chain, and the unchanged merge
    follows: scores and ids are bit-equal to ``cosine_topk``'s. ``cnorm`` is
    the mirror's largest row norm (``quantize_rows_q8``); None computes it
    from ``corpus`` on every call. ``cap`` overrides the per-query candidate
    capacity of that path (tests). A batch holding a query that quantises to
    zeros is answered by the bf16 search (``q8_degenerate_fallbacks``).

    The screen runs its main launch in stages and raises each query's floor
    between them to the k-th best exact score found so far (knn_plan.h
    ``plan_q8_stages``): later stages pass fewer candidates and the result is
    the same. ``stages`` forces their number (1: one launch; up to
    ``Q8_MAX_STAGES``); None leaves it to KAKVEDA_Q8_STAGES, else to the
    plan's rule. ``return_counts`` (GPU only) adds a third result: the
    candidates per query (i32 [B]; empty where the request is not screened)."""
    global q8_overflow_fallbacks, q8_degenerate_fallbacks
    _q8_check_dim(int(queries.shape[1]))
    if (labels is None) != (want is None):
        raise ValueError("labels and want go together")
    n = int(valid_n) if valid_n is not None else corpus.shape[0]
    B = queries.shape[0]
    if n <= 0:
        return (
            torch.full((B, k), float("-inf"), dtype=torch.float32, device=queries.device),
            torch.full((B, k), -1, dtype=torch.int64, device=queries.device),
        )
    if queries.device.type != "cuda":
        return cosine_topk_q8_ref(
            queries, corpus, codes, meta, k, n, labels, want, cnorm, batch_min_b,
            batch_min_rows,
        )
    ext = _require_ext()
    kk = min(int(k), KMAX)
    filt = {}
    if want is not None:
        filt = dict(
            labels=labels.to(device=corpus.device, dtype=torch.int32).contiguous(),
            want=want.to(device=queries.device, dtype=torch.int32).contiguous(),
        )
    min_b = Q8_BATCH_MIN_B if batch_min_b is None else int(batch_min_b)
    if q8_batch_in_plan(
        B, n, kk, int(queries.shape[1]), want is not None, min_b, batch_min_rows
    ):
        if cnorm is None:
            cnorm = q8_cnorm(corpus[:n])
        filt.update(cnorm=cnorm, batch_min_b=min_b, cap=int(cap or 0),
                    stages=_q8_stages_arg(stages))
    scores, idx, fallback, counts = ext.cosine_topk_q8(
        queries, corpus, codes, meta, kk, n, **filt
    )
    q8_overflow_fallbacks += int(fallback == 1)
    q8_degenerate_fallbacks += int(fallback == 2)
    if want is not None:
        scores = torch.where(idx < 0, torch.full_like(scores, float("-inf")), scores)
    if return_counts:
        return _pad_topk(scores, idx, k) + (counts,)
    return _pad_topk(scores, idx, k)


# ---------------------------------------------------------------------------
# row L2 normalisation
# ---------------------------------------------------------------------------

def l2normalize_(t: torch.Tensor, start_row: int = 0, end_row: Optional[int] = None) -> torch.Tensor:
    """In-place L2-normalise rows [start_row, end_row) of a [N, D] tensor."""
    end = int(end_row) if end_row is not None else t.shape[0]
    if end <= start_row:
        return t
    if t.device.type == "cuda":
        ext = _require_ext()
        ext.l2normalize_(t, int(start_row), end)
        return t
    seg = t[start_row:end]
    norm = seg.float().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    seg.copy_((seg.float() / norm).to(t.dtype))
    return t


# ---------------------------------------------------------------------------
# embedding bag (hashed-feature gather-sum)
# ---------------------------------------------------------------------------

def embedding_bag(table: torch.Tensor, idx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """out[b] = sum_l w[b,l] * table[idx[b,l]]  -> [B, D] float32.

    table bf16 [V, D], idx integer [B, L], w [B, L]; L <= 128 on GPU. An
    index outside [0, V) contributes nothing, whatever its weight (-1 pads
    a short bag).
    """
    if table.device.type == "cuda":
        ext = _require_ext()
        return ext.embedding_bag(table, idx.to(torch.int32), w.float())
    ix = idx.long()
    live = (ix >= 0) & (ix < table.shape[0])
    flat = table[ix.clamp(0, table.shape[0] - 1).reshape(-1)].reshape(*idx.shape, table.shape[1]).float()
    return (flat * (w.float() * live).unsqueeze(-1)).sum(dim=1)


# ---------------------------------------------------------------------------
# device featurizer (signature-text bytes -> hashed n-gram rows)
# ---------------------------------------------------------------------------

#: capacity of one text on the device (mirror of featurize_plan.h; pinned by
#: tests/test_device_featurize.py): bytes, and uni+bigrams before
#: de-duplication. A text over either gets status 1 and a zero row.
FEATURIZE_MAX_BYTES = 1024
FEATURIZE_MAX_GRAMS = 256

#: row status of featurize_bytes
FEATURIZE_OK = 0
FEATURIZE_TOO_MANY_GRAMS = 1  # over FEATURIZE_MAX_BYTES or FEATURIZE_MAX_GRAMS
FEATURIZE_TOO_MANY_FEATURES = 2  # more than max_features buckets

_HIGH_TO_SPACE = bytes(range(128)) + b" " * 128


def featurize_start_state(seed: int) -> int:
    """Start state of every gram hash for ``seed`` (featurizer._fnv1a)."""
    from kakveda_amd.encoder.featurizer import _FNV_OFFSET, _MASK64

    return (_FNV_OFFSET ^ (seed * 0x9E3779B97F4A7C15)) & _MASK64


def featurize_bytes(
    buf: torch.Tensor, offsets: torch.Tensor, hash_dim: int, seed: int, max_features: int
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``featurize_batch`` over texts given as bytes.

    buf: uint8, every text back to back with nothing between them; offsets:
    int32 [B+1], text b being ``buf[offsets[b]:offsets[b+1]]``. ``hash_dim``
    in [1, 2^31), ``max_features`` in [1, 128] (``embedding_bag``'s limit).
    Returns (idx i32 [B, max_features], w f32 [B, max_features], status i32
    [B], flagged i32 [1]): the rows ``featurize_batch`` gives for the decoded
    texts - indices equal, weights to fp32 rounding - where status is 0.
    Status 1 marks a text over FEATURIZE_MAX_BYTES bytes or
    FEATURIZE_MAX_GRAMS grams, status 2 one with more than ``max_features``
    buckets (``featurize_batch`` then keeps the largest by an unstable sort,
    which cannot be reproduced): such a row is all zeros and the caller
    recomputes it on the host. ``flagged`` is the number of such rows.

    Bytes are tokenised as ASCII: the result equals ``featurize_batch`` only
    for texts that are ``str.isascii()`` (``featurizer.pack_texts`` routes
    the others to the host).
    """
    hash_dim, max_features = int(hash_dim), int(max_features)
    if not 1 <= hash_dim < 1 << 31:
        raise ValueError(f"hash_dim must be in [1, 2^31), got {hash_dim}")
    if not 1 <= max_features <= 128:
        raise ValueError(f"max_features must be in [1, 128], got {max_features}")
    if buf.device.type == "cuda":
        ext = _require_ext()
        idx, w, status, flagged = ext.featurize_bytes(
            buf, offsets, hash_dim, featurize_start_state(int(seed)), max_features
        )
        return idx, w, status, flagged
    return featurize_bytes_ref(buf, offsets, hash_dim, seed, max_features)


def featurize_bytes_ref(
    buf: torch.Tensor, offsets: torch.Tensor, hash_dim: int, seed: int, max_features: int
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Reference of ``featurize_bytes`` on the host: decode each text, set
    the status by the kernel's rules, and take the rows from
    ``featurize_batch``. A flagged row is all zeros, as from the kernel."""
    import numpy as np

    from kakveda_amd.encoder.featurizer import featurize, featurize_batch, tokenize

    raw = buf.detach().cpu().numpy().tobytes()
    off = [int(o) for o in offsets.detach().cpu().tolist()]
    B = len(off) - 1
    status = np.zeros(B, dtype=np.int32)
    texts = []
    for b in range(B):
        lo, hi = off[b], off[b + 1]
        if not 0 <= lo <= hi <= len(raw):
            raise ValueError(f"offsets of text {b} ({lo}, {hi}) lie outside the buffer")
        # latin-1 keeps one character per byte; bytes >= 0x80 are separators
        # on the device, so they become spaces before the str tokeniser
        # (whose lower() could turn them into token characters) sees them
        text = raw[lo:hi].translate(_HIGH_TO_SPACE).decode("ascii")
        n_tok = len(tokenize(text))
        if hi - lo > FEATURIZE_MAX_BYTES or 2 * n_tok - 1 > FEATURIZE_MAX_GRAMS:
            status[b] = FEATURIZE_TOO_MANY_GRAMS
        elif len(featurize(text, hash_dim=hash_dim, seed=seed)[0]) > max_features:
            status[b] = FEATURIZE_TOO_MANY_FEATURES
        texts.append(text if status[b] == FEATURIZE_OK else "")
    idx, w = featurize_batch(texts, hash_dim=hash_dim, seed=seed, max_features=max_features)
    return (
        torch.from_numpy(idx),
        torch.from_numpy(w),
        torch.from_numpy(status),
        torch.tensor([int((status != 0).sum())], dtype=torch.int32),
    )


# ---------------------------------------------------------------------------
# k-means (pattern detector)
# ---------------------------------------------------------------------------

#: LDS a block of the dedicated assignment kernel may use for its 64-row
#: centroid image (kernels_impl.h ASSIGN_LDS_BYTES)
_ASSIGN_LDS_BYTES = 160 * 1024

#: rows per cosine_topk call on the general route of kmeans_assign_scored:
#: one launch holds at most 65535 row tiles of 128 rows (knn_plan.h
#: plan_fits_grid), the 10M-point detector has more
_ASSIGN_CHUNK_ROWS = 1 << 20


def assign_pitch(D: int) -> int:
    """Row pitch in bytes of the assignment kernel's centroid LDS image
    (mirror of kernels_impl.h assign_pitch; the header pins the resulting
    D limit with a static_assert, tests/test_aux_cases_ref.py pins it here)."""
    return D * 2 + ((64 - (D * 2) % 256) + 256) % 256


def assign_kernel_fits(C: int, D: int) -> bool:
    """Whether the dedicated C<=64 assignment kernel takes this shape: its
    64 centroid rows of D dims must fit the block's LDS, which holds for
    D <= KMEANS_ASSIGN_MAX_D."""
    return C <= 64 and 64 * assign_pitch(D) <= _ASSIGN_LDS_BYTES


#: widest row (a multiple of 64) the dedicated assignment kernel accepts
KMEANS_ASSIGN_MAX_D = max(d for d in range(64, 4096 + 1, 64) if assign_kernel_fits(1, d))


def kmeans_assign_scored(
    points: torch.Tensor, centroids: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(top-1 cosine f32 [N], nearest centroid id i64 [N]) per point.

    GPU, C<=64 and D<=KMEANS_ASSIGN_MAX_D (1152): the dedicated
    LDS-resident-centroid kernel (point stream straight from HBM to MFMA,
    no per-window barriers — built for the pattern detector's
    N-huge/C-tiny shape). GPU otherwise (C>64, or rows too wide for the
    LDS image): the general fused cosine_topk with k=1, in calls of at most
    2^20 points so that no N exceeds one launch's row tiles. CPU: eager
    matmul+argmax.

    Ties: the dedicated kernel and the CPU path return the lowest index
    among equal best scores. The general route returns one of them, which
    one is unspecified (see cosine_topk).
    """
    if points.device.type == "cuda":
        ext = _require_ext()
        C, D = int(centroids.shape[0]), int(centroids.shape[1])
        if assign_kernel_fits(C, D):
            scores, idx = ext.kmeans_assign(points, centroids)
            return scores, idx.long()
        N = int(points.shape[0])
        if N <= _ASSIGN_CHUNK_ROWS:
            scores, idx = ext.cosine_topk(points, centroids, 1, C)
            return scores[:, 0], idx[:, 0]
        scores = torch.empty(N, dtype=torch.float32, device=points.device)
        idx = torch.empty(N, dtype=torch.int64, device=points.device)
        for r0 in range(0, N, _ASSIGN_CHUNK_ROWS):
            r1 = min(r0 + _ASSIGN_CHUNK_ROWS, N)
            s, i = ext.cosine_topk(points[r0:r1], centroids, 1, C)
            scores[r0:r1] = s[:, 0]
            idx[r0:r1] = i[:, 0]
        return scores, idx
    sims = points.float() @ centroids.float().t()
    top = sims.max(dim=1)
    return top.values, top.indices


def kmeans_assign(points: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """Nearest (max-cosine) centroid id per point -> int64 [N]."""
    return kmeans_assign_scored(points, centroids)[1]


def kmeans_update(
    points: torch.Tensor, assign: torch.Tensor, n_clusters: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Segmented reduction: per-cluster sum + count -> ([C, D] f32, [C] f32).

    GPU: LDS-partial segmented-reduction HIP kernel (points read once per
    64-dim tile). CPU fallback: index_add_.

    A point whose assignment is outside [0, n_clusters) is dropped from
    sums and counts (-1 marks an unassigned point). ``counts`` is float32 and counts by adding 1.0: it is exact up to 2^24
    points per cluster and loses the odd counts above that.
    """
    if points.device.type == "cuda" and n_clusters <= 512:
        ext = _require_ext()
        return ext.kmeans_update(
            points.to(torch.bfloat16), assign.to(torch.int32), int(n_clusters)
        )
    D = points.shape[1]
    a = assign.long()
    live = (a >= 0) & (a < n_clusters)
    if not bool(live.all()):
        a, points = a[live], points[live]
    sums = torch.zeros(n_clusters, D, dtype=torch.float32, device=points.device)
    sums.index_add_(0, a, points.float())
    counts = torch.zeros(n_clusters, dtype=torch.float32, device=points.device)
    counts.index_add_(0, a, torch.ones_like(a, dtype=torch.float32))
    return sums, counts


# ---------------------------------------------------------------------------
# cluster-routed (IVF) search
# ---------------------------------------------------------------------------

def _pad_topk(scores: torch.Tensor, idx: torch.Tensor, k: int):
    kk = scores.shape[1]
    if kk >= k:
        return scores, idx
    B = scores.shape[0]
    pad_s = torch.full((B, k - kk), float("-inf"), dtype=scores.dtype, device=scores.device)
    pad_i = torch.full((B, k - kk), -1, dtype=idx.dtype, device=idx.device)
    return torch.cat([scores, pad_s], dim=1), torch.cat([idx, pad_i], dim=1)


def _segment_list(segments) -> list:
    return [segments] if isinstance(segments, torch.Tensor) else list(segments)


def _gather_rows(segments: list, rows: torch.Tensor) -> torch.Tensor:
    """Rows (global ids, int64) of a segmented store as one [n, D] tensor."""
    if len(segments) == 1:
        return segments[0][rows]
    out = torch.empty(rows.shape[0], segments[0].shape[1], dtype=segments[0].dtype,
                      device=segments[0].device)
    base = 0
    for seg in segments:
        n = int(seg.shape[0])
        m = (rows >= base) & (rows < base + n)
        if bool(m.any()):
            out[m] = seg[rows[m] - base]
        base += n
    return out


def ivf_route_scores(queries: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """Dense fp32 scores [B, L] of the queries against the IVF centroids."""
    if queries.device.type == "cuda":
        return _require_ext().ivf_route_scores(queries, centroids)
    return queries.float() @ centroids.float().t()


#: queries per tile of the list-major scan (ivf_batch_plan.h IVF_BATCH_QTILE)
IVF_BATCH_QTILE = 16

#: batch size from which ``batched=None`` selects the list-major scan (None
#: would mean never). Measured, profiles/routed_search.md "List-major scan":
#: the smallest B from which it beats the per-query scan by more than the
#: spread on both corpora at nprobe 32 and 64 (10M mixture: from 64 and 32,
#: 200k encoder: from 128 and 64); never below 64
IVF_BATCHED_MIN_B: Optional[int] = 128


def ivf_batch_tile_bound(n_pairs: int, n_lists: int) -> int:
    """Tiles that ``n_pairs`` (query, probe) pairs over ``n_lists`` lists and
    the tail can make at most, whatever the grouping (mirror of
    ivf_batch_plan.h ivf_batch_tile_bound)."""
    return min(n_pairs, n_pairs // IVF_BATCH_QTILE + n_lists + 1)


def ivf_group_probes(probes: torch.Tensor, n_lists: int):
    """Group the (query, probe) pairs of a batch by list, for the list-major
    scan. ``probes`` is integer [B, nprobe]; every query also probes the
    tail, pseudo-list ``n_lists``, as its pair nprobe. Probes outside
    [0, n_lists) are discarded. Returns

    - ``pair_query``, ``pair_slot`` int32 [P], P = B * (nprobe + 1): the
      query b and the probe rank y of each pair, sorted by list (discarded
      pairs last);
    - ``tiles`` int32 [3, T]: per tile its list, its first pair and its
      pair count (1..IVF_BATCH_QTILE; 0 from the tile count on), T =
      ``ivf_batch_tile_bound(P, n_lists)``. A tile never spans two lists;
    - ``n_tiles`` int32 [1], on the probes' device.

    Torch ops only, on any device, and none of them reads device memory on
    the host: the launch is sized by the bound T. The extension runs the
    same sequence (ivf_group_probes_op) inside ``ivf_scan_topk_batched``.
    """
    B, S = int(probes.shape[0]), int(probes.shape[1]) + 1
    P, L, QT = B * S, int(n_lists), IVF_BATCH_QTILE
    T = ivf_batch_tile_bound(P, L)
    dev = probes.device
    pl = probes.long()
    pl = torch.where((pl >= 0) & (pl < L), pl, torch.full_like(pl, L + 1))
    tail = torch.full((B, 1), L, dtype=torch.int64, device=dev)
    keys = torch.cat([pl, tail], dim=1).reshape(P)
    order = torch.sort(keys, stable=True).indices
    counts = torch.zeros(L + 2, dtype=torch.int64, device=dev).scatter_add_(
        0, keys, torch.ones(P, dtype=torch.int64, device=dev)
    )[: L + 1]
    starts = counts.cumsum(0) - counts
    ntl = (counts + (QT - 1)) // QT
    tend = ntl.cumsum(0)
    n_tiles = tend[L : L + 1]
    t = torch.arange(T, dtype=torch.int64, device=dev)
    li = torch.searchsorted(tend, t, right=True).clamp_max(L)
    within = t - (tend[li] - ntl[li])
    live = t < n_tiles
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    tfirst = torch.where(live, starts[li] + within * QT, zero)
    tcnt = torch.where(live, (counts[li] - within * QT).clamp(0, QT), zero)
    tiles = torch.stack([li, tfirst, tcnt]).to(torch.int32).contiguous()
    return (
        (order // S).to(torch.int32),
        (order % S).to(torch.int32),
        tiles,
        n_tiles.to(torch.int32),
    )


#: widest row the list-major scan's LDS query tile holds (ivf_batch_plan.h
#: IVF_BATCH_MAX_D); ``batched=None`` keeps wider rows on the per-query scan
IVF_BATCH_MAX_D = 1472


def _use_batched(batched: Optional[bool], B: int, D: int) -> bool:
    if batched is None:
        return (
            IVF_BATCHED_MIN_B is not None
            and B >= IVF_BATCHED_MIN_B
            and D <= IVF_BATCH_MAX_D
        )
    return bool(batched)


def _label_list(labels, segments: list) -> list:
    """``labels`` as one tensor per segment: a list is taken as it is, one
    tensor is split at the segment boundaries."""
    if not isinstance(labels, torch.Tensor):
        return list(labels)
    if len(segments) == 1:
        return [labels]
    return list(torch.split(labels, [int(s.shape[0]) for s in segments]))


def _ivf_scan_ref(queries, segments, offsets, ids, probes, k, valid_n, tail_lo,
                  tail_hi, labels=None, want=None):
    """The routed scan in plain PyTorch (fp32 accumulate); ``labels=None,
    want=None`` means unfiltered."""
    segs = _segment_list(segments)
    dev = queries.device
    B = queries.shape[0]
    L = int(offsets.shape[0]) - 1
    off = offsets.to("cpu").long().tolist()
    ids_l = ids.to(dev).long()
    if labels is not None:
        lab = torch.cat([l.to(dev).long().reshape(-1) for l in _label_list(labels, segs)])
        w = want.to("cpu").long().tolist()
    tail = torch.arange(int(tail_lo), int(tail_hi), dtype=torch.int64, device=dev)
    out_s = torch.full((B, k), float("-inf"), dtype=torch.float32, device=dev)
    out_i = torch.full((B, k), -1, dtype=torch.int64, device=dev)
    for b, row in enumerate(probes.to("cpu").long().tolist()):
        parts = [ids_l[off[l] : off[l + 1]] for l in row if 0 <= l < L]
        rows = torch.cat(parts + [tail])
        rows = rows[(rows >= 0) & (rows < int(valid_n))]
        if labels is not None and w[b] >= 0:
            rows = rows[lab[rows] == w[b]]
        if rows.numel() == 0:
            continue
        sims = _gather_rows(segs, rows).float() @ queries[b].float()
        kk = min(k, int(rows.numel()))
        s, sel = torch.topk(sims, kk)
        out_s[b, :kk] = s
        out_i[b, :kk] = rows[sel]
    return out_s, out_i


def _ivf_search_ref(queries, segments, centroids, offsets, ids, nprobe, k, valid_n,
                    n_indexed, labels=None, want=None):
    """The routed search in plain PyTorch: route, then ``_ivf_scan_ref``."""
    route = queries.float() @ centroids.float().t()
    probes = torch.topk(route, min(int(nprobe), route.shape[1]), dim=1).indices
    return _ivf_scan_ref(
        queries, segments, offsets, ids, probes, k, valid_n,
        min(int(n_indexed), int(valid_n)), valid_n, labels, want,
    )


def _ivf_gpu(op, batched, queries, segments, labels, want, pre, offsets, ids, mid, k, post):
    """Run the extension's routed op ``op`` ("ivf_scan_topk" or "ivf_search",
    its ``_batched`` form as ``batched`` says, its ``_filtered`` form when
    ``labels`` is given) and normalise what it returns. The arguments follow
    the extension's order: ``pre`` stands before ``offsets``, ``mid`` between
    ``ids`` and ``k``, ``post`` (integers) after ``k``."""
    ext = _require_ext()
    dev = queries.device

    def i32(t):
        return t.to(device=dev, dtype=torch.int32).contiguous() if isinstance(t, torch.Tensor) else t

    segs = _segment_list(segments)
    if _use_batched(batched, queries.shape[0], queries.shape[1]):
        op += "_batched"
    filt = ()
    if labels is not None:
        op += "_filtered"
        filt = ([i32(l) for l in _label_list(labels, segs)], i32(want))
    scores, idx = getattr(ext, op)(
        queries,
        segs,
        *filt,
        *pre,
        offsets.to(device=dev, dtype=torch.int64).contiguous(),
        i32(ids),
        i32(mid),
        min(int(k), KMAX),
        *(int(v) for v in post),
    )
    scores = torch.where(idx < 0, torch.full_like(scores, float("-inf")), scores)
    return _pad_topk(scores, idx, k)


def ivf_scan_topk_ref(
    queries: torch.Tensor,
    segments,
    offsets: torch.Tensor,
    ids: torch.Tensor,
    probes: torch.Tensor,
    k: int,
    valid_n: int,
    tail_lo: int,
    tail_hi: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain-PyTorch reference of ``ivf_scan_topk`` (fp32 accumulate)."""
    return _ivf_scan_ref(queries, segments, offsets, ids, probes, k, valid_n, tail_lo, tail_hi)


def ivf_scan_topk(
    queries: torch.Tensor,
    segments,
    offsets: torch.Tensor,
    ids: torch.Tensor,
    probes: torch.Tensor,
    k: int,
    valid_n: int,
    tail_lo: int,
    tail_hi: int,
    max_list_len: int = 0,
    batched: Optional[bool] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k of each query over a candidate set given as inverted lists.

    segments: the store's row tensors in order ([n_i, D]; one tensor is
    accepted too); ``ids`` int32 holds global row ids, list l being
    ``ids[offsets[l]:offsets[l+1]]``; ``probes`` int32 [B, nprobe] names the
    lists each query scans (entries outside [0, L) are skipped, so -1 pads;
    the others must be distinct per query). Every query also scans the
    contiguous rows [tail_lo, tail_hi). Row ids outside [0, valid_n) are
    ignored. Returns (scores f32 [B, k], idx i64 [B, k]) sorted descending,
    padded with (-inf, -1) where the candidate set is shorter than k and
    past KMAX columns on GPU. ``max_list_len`` (the longest list, if known)
    only sizes the GPU grid.

    ``batched`` picks the GPU scan: False the per-query kernel, True the
    list-major one (each probed list gathered once per tile of
    IVF_BATCH_QTILE queries, MFMA scoring; D <= IVF_BATCH_MAX_D), None the
    list-major one from IVF_BATCHED_MIN_B queries on where D allows it. Both compute the same contract; scores may
    differ by the fp32 summation order (<= D * 2^-22 for unit rows). On CPU
    every value runs the reference.
    """
    if queries.device.type != "cuda":
        return _ivf_scan_ref(queries, segments, offsets, ids, probes, k, valid_n, tail_lo, tail_hi)
    return _ivf_gpu(
        "ivf_scan_topk", batched, queries, segments, None, None, (), offsets, ids,
        probes, k, (valid_n, tail_lo, tail_hi, max_list_len),
    )


def ivf_search_ref(
    queries: torch.Tensor,
    segments,
    centroids: torch.Tensor,
    offsets: torch.Tensor,
    ids: torch.Tensor,
    nprobe: int,
    k: int,
    valid_n: int,
    n_indexed: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain-PyTorch reference of ``ivf_search`` (fp32 accumulate)."""
    return _ivf_search_ref(
        queries, segments, centroids, offsets, ids, nprobe, k, valid_n, n_indexed
    )


def ivf_search(
    queries: torch.Tensor,
    segments,
    centroids: torch.Tensor,
    offsets: torch.Tensor,
    ids: torch.Tensor,
    nprobe: int,
    k: int,
    valid_n: int,
    n_indexed: int,
    max_list_len: int = 0,
    batched: Optional[bool] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Cluster-routed approximate top-k: score the L centroids, scan the
    ``nprobe`` best lists of each query plus the tail [n_indexed, valid_n)
    of rows appended since the index was built, return the exact top-k of
    that candidate set. With ``nprobe == L`` the candidate set is every row
    and the result is the exact search's. Shapes, padding and
    ``batched`` as ``ivf_scan_topk``."""
    L = int(centroids.shape[0])
    nprobe = max(1, min(int(nprobe), L))
    if queries.device.type != "cuda":
        return _ivf_search_ref(
            queries, segments, centroids, offsets, ids, nprobe, k, valid_n, n_indexed
        )
    return _ivf_gpu(
        "ivf_search", batched, queries, segments, None, None, (centroids,), offsets,
        ids, nprobe, k, (valid_n, n_indexed, max_list_len),
    )


# ---------------------------------------------------------------------------
# label-filtered routed search
# ---------------------------------------------------------------------------

#: a batch whose every query is filtered to a label that at most this share
#: of the rows carry is "sparse": the per-query scan skips almost every row
#: (no load, no multiply) while the list-major scan still gathers them all,
#: so the crossover moves. Measured, profiles/routed_filtered.md "Crossover":
#: at 1% and 0.1% the list-major scan wins only from 1024 queries on (at 512
#: the per-query scan is 15% / 31% faster, spread <= 4.7%), against 128 at
#: 50%. Only a caller that knows the labels' row counts can apply it
#: (``EmbeddingStore.search``); the ops themselves go by IVF_BATCHED_MIN_B.
IVF_FILTERED_SPARSE_SHARE = 0.01
IVF_FILTERED_SPARSE_MIN_B = 1024


def ivf_scan_topk_filtered_ref(
    queries: torch.Tensor,
    segments,
    labels,
    want: torch.Tensor,
    offsets: torch.Tensor,
    ids: torch.Tensor,
    probes: torch.Tensor,
    k: int,
    valid_n: int,
    tail_lo: int,
    tail_hi: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain-PyTorch reference of ``ivf_scan_topk_filtered`` (fp32
    accumulate): ``ivf_scan_topk_ref`` over the candidates whose label the
    query wants."""
    return _ivf_scan_ref(
        queries, segments, offsets, ids, probes, k, valid_n, tail_lo, tail_hi, labels, want
    )


def ivf_scan_topk_filtered(
    queries: torch.Tensor,
    segments,
    labels,
    want: torch.Tensor,
    offsets: torch.Tensor,
    ids: torch.Tensor,
    probes: torch.Tensor,
    k: int,
    valid_n: int,
    tail_lo: int,
    tail_hi: int,
    max_list_len: int = 0,
    batched: Optional[bool] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ivf_scan_topk`` with a per-query label predicate pushed into the scan.

    labels: int32, one per store row (-1 = unlabelled), as one tensor or as
    one tensor per segment; want: int32 [B]. A candidate row r is eligible
    for query b iff ``want[b] < 0 or label(r) == want[b]`` (the rule of
    ``cosine_topk_filtered``), so a batch may mix filtered and unfiltered
    queries in one launch. An ineligible row is treated as a row id outside
    [0, valid_n) is: never inserted (and, in the per-query scan, not read
    from memory; the list-major scan scores a row for its whole tile of
    queries and filters at the insert). Everything else -
    shapes, the (-inf, -1) padding, the KMAX clamp, ``max_list_len`` and
    ``batched`` - is as ``ivf_scan_topk``; with ``want < 0`` everywhere the
    result is that op's.
    """
    if queries.device.type != "cuda":
        return _ivf_scan_ref(
            queries, segments, offsets, ids, probes, k, valid_n, tail_lo, tail_hi, labels, want
        )
    return _ivf_gpu(
        "ivf_scan_topk", batched, queries, segments, labels, want, (), offsets, ids,
        probes, k, (valid_n, tail_lo, tail_hi, max_list_len),
    )


def ivf_search_filtered_ref(
    queries: torch.Tensor,
    segments,
    labels,
    want: torch.Tensor,
    centroids: torch.Tensor,
    offsets: torch.Tensor,
    ids: torch.Tensor,
    nprobe: int,
    k: int,
    valid_n: int,
    n_indexed: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain-PyTorch reference of ``ivf_search_filtered`` (fp32 accumulate)."""
    return _ivf_search_ref(
        queries, segments, centroids, offsets, ids, nprobe, k, valid_n, n_indexed, labels, want
    )


def ivf_search_filtered(
    queries: torch.Tensor,
    segments,
    labels,
    want: torch.Tensor,
    centroids: torch.Tensor,
    offsets: torch.Tensor,
    ids: torch.Tensor,
    nprobe: int,
    k: int,
    valid_n: int,
    n_indexed: int,
    max_list_len: int = 0,
    batched: Optional[bool] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ivf_search`` restricted per query to the rows of one label: route on
    the centroids as the unfiltered search does (the lists know nothing of
    labels), scan the ``nprobe`` best lists plus the tail, and return the
    top-k of the eligible rows among them. ``labels`` and ``want`` as
    ``ivf_scan_topk_filtered``. A query comes back short of k when its
    label's rows sit in lists it did not probe; ``EmbeddingStore.search``
    fills such rows from the exact filtered search. With ``nprobe == L`` the
    result is ``cosine_topk_filtered``'s."""
    L = int(centroids.shape[0])
    nprobe = max(1, min(int(nprobe), L))
    if queries.device.type != "cuda":
        return _ivf_search_ref(
            queries, segments, centroids, offsets, ids, nprobe, k, valid_n, n_indexed, labels, want
        )
    return _ivf_gpu(
        "ivf_search", batched, queries, segments, labels, want, (centroids,), offsets,
        ids, nprobe, k, (valid_n, n_indexed, max_list_len),
    )
