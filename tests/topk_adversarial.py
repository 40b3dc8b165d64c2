"""Shared helper of the adversarial exact-top-k tests (ties, duplicates,
masked columns): the tie-aware float64 checker, the data families, and the
child-process entry for the settings that are read once per process.

Imported by tests/test_topk_adversarial_ref.py (CPU: the plain-torch
references under the checker) and tests/test_gpu_topk_adversarial.py (the
HIP kernels under the same checker). Not a test module and not a conftest.

The checker's tolerance is E = D * 2^-23: for unit rows an fp32 sum of the
exact bf16 products is within (D-1) * 2^-24 of the true inner product
(kakveda_amd/ops/hip/kernels_impl.h), and E is twice that. Everything is
generated with seeded CPU generators; planted rows and queries are small
CPU tensors that the caller copies to its device next to a clone of the
shared base corpus.
"""

from __future__ import annotations

import os
import re
import sys
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_BASE = 65_700  # whole corpus sampled by the prepass; 36 real columns in the last tile
COSINES = [0.95 - 0.05 * j for j in range(8)]  # the near-duplicate run


# ---------------------------------------------------------------------------
# dispatch-plan constants, read from the header the kernels are built from
# ---------------------------------------------------------------------------

def plan_constants() -> Dict[str, int]:
    text = open(os.path.join(REPO, "kakveda_amd", "ops", "hip", "knn_plan.h")).read()

    def const(pattern):
        return int(re.search(pattern, text).group(1))

    pc = {
        name: const(r"constexpr int %s = (\d+);" % name)
        for name in ("BM", "BN", "BM8", "BN8", "KMAX", "PRE_TILES", "PREG_WARM",
                     "PREG_EMIT", "MIN_N_8P", "MIN_N_EMIT", "SMALLB_MAX")
    }
    pc["cap"] = const(r"long cap = (\d+);")
    m = re.search(r"tile == BM8 \? (\d+) : (\d+);", text)
    pc["target8"], pc["target"] = int(m.group(1)), int(m.group(2))
    return pc


def chunk_columns(B: int, N: int, tile: int, pc: Dict[str, int]) -> int:
    """Corpus columns per main-launch block (knn_plan.h chunking())."""
    row_tiles = (B + tile - 1) // tile
    ntiles = (N + tile - 1) // tile
    target = pc["target8"] if tile == pc["BM8"] else pc["target"]
    want = (ntiles * row_tiles + target - 1) // target
    return max(4, min(want, 128)) * tile


def tolerance(d: int) -> float:
    return d * 2.0 ** -23


# ---------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------

def _first(mask: torch.Tensor):
    nz = mask.nonzero()
    return None if nz.numel() == 0 else tuple(int(v) for v in nz[0].tolist())


def check_topk(scores, idx, sims64, k, d, eligible=None, what="") -> None:
    """Tie-aware check of an exact top-k result against float64 scores.

    scores f32 [B, k], idx i64 [B, k]; sims64 f64 [B, n] over the valid
    columns only; d the row dimension (E = d * 2^-23); eligible bool [B, n]
    or None. With m = min(k, #eligible) per row: (1) idx[:m] in [0, n), eligible, pairwise distinct, and
    idx[m:] == -1, scores[m:] == -inf; (2) every claimed score within E of
    its column's true score; (3) scores non-increasing; (4) the j-th score
    within E of the j-th best eligible true score; (5) every eligible column
    more than E above the m-th best is returned. Raises AssertionError.
    """
    B, n = sims64.shape
    assert scores.shape == (B, k) and idx.shape == (B, k), (what, scores.shape, idx.shape)
    assert scores.dtype == torch.float32 and idx.dtype == torch.int64, (what, scores.dtype, idx.dtype)
    dev = sims64.device
    scores, idx = scores.to(dev), idx.to(dev)
    D_E = tolerance(d)
    elig = torch.ones(B, n, dtype=torch.bool, device=dev) if eligible is None else eligible.to(dev)
    m = elig.sum(dim=1).clamp(max=k)
    col = torch.arange(k, device=dev)[None, :]
    live = col < m[:, None]

    def fail(mask, msg, detail=lambda r, j: ""):
        hit = _first(mask)
        if hit is not None:
            r, j = hit
            raise AssertionError(
                "%s: row %d rank %d: %s (idx=%s scores=%s)%s"
                % (what, r, j, msg, idx[r].tolist(), scores[r].tolist(), detail(r, j))
            )

    # 1. index validity
    fail(live & ((idx < 0) | (idx >= n)), "index outside [0, %d)" % n)
    safe = idx.clamp(0, n - 1)
    fail(live & ~elig.gather(1, safe), "ineligible column returned")
    srt = torch.where(live, idx, -1 - col.expand(B, k)).sort(dim=1).values
    dup = srt[:, 1:] == srt[:, :-1]
    fail(dup, "repeated index", lambda r, j: " repeated: %d" % int(srt[r, j]))
    fail(~live & (idx != -1), "pad index is not -1")
    fail(~live & (scores != float("-inf")), "pad score is not -inf")
    # 2. claimed scores
    claimed = sims64.gather(1, safe)
    err = (scores.double() - claimed).abs()
    fail(live & ~(err <= D_E), "claimed score off its column's true score by more than E=%.3g" % D_E,
         lambda r, j: " true=%.9g" % float(claimed[r, j]))
    # 3. ordering as returned
    if k > 1:
        fail(~(scores[:, :-1] >= scores[:, 1:]), "scores increase after this rank")
    # 4. rank values
    masked = sims64.masked_fill(~elig, float("-inf"))
    kk = min(k, n)
    ref = torch.topk(masked, kk, dim=1).values
    if kk < k:
        ref = torch.cat([ref, ref.new_full((B, k - kk), float("-inf"))], dim=1)
    rerr = (scores.double() - ref).abs()
    fail(live & ~(rerr <= D_E), "score differs from the true score of its rank by more than E=%.3g" % D_E,
         lambda r, j: " true rank scores=%s" % ref[r].tolist())
    # 5. clear winners
    has = m > 0
    kth = ref.gather(1, (m - 1).clamp(min=0)[:, None])[:, 0]
    winners = elig & (sims64 > (kth + D_E)[:, None]) & has[:, None]
    present = torch.zeros(B, n + 1, dtype=torch.bool, device=dev)
    present.scatter_(1, torch.where(live, idx, torch.full_like(idx, n)), True)
    missing = winners & ~present[:, :n]
    hit = _first(missing)
    if hit is not None:
        r, c = hit
        raise AssertionError(
            "%s: row %d: column %d (true score %.9g) beats the rank-%d score %.9g by more than "
            "E=%.3g but is missing; %d such columns in this row (idx=%s scores=%s)"
            % (what, r, c, float(sims64[r, c]), int(m[r]), float(kth[r]), D_E,
               int(missing[r].sum()), idx[r].tolist(), scores[r].tolist())
        )


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------

def rand_unit(n: int, d: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float32)
    x /= x.norm(dim=-1, keepdim=True)
    return x.to(torch.bfloat16)


def near_rows(q: torch.Tensor, gen: torch.Generator, cosines=COSINES) -> torch.Tensor:
    """[nq, len(cosines), D] bf16 rows a*q + sqrt(1-a^2)*u with u a unit
    vector orthogonal to q, one run per query row of q [nq, D]."""
    qd = q.double()
    qd = qd / qd.norm(dim=-1, keepdim=True)
    u = torch.randn(q.shape[0], len(cosines), q.shape[1], generator=gen, dtype=torch.float64)
    u -= (u * qd[:, None, :]).sum(-1, keepdim=True) * qd[:, None, :]
    u /= u.norm(dim=-1, keepdim=True)
    a = torch.tensor(cosines, dtype=torch.float64)[None, :, None]
    return (a * qd[:, None, :] + (1 - a * a).sqrt() * u).to(torch.bfloat16)


@dataclass
class Case:
    name: str
    q: torch.Tensor  # [B, D] bf16, CPU
    n: int  # valid rows
    k: int
    rows: int = 0  # allocated rows (>= n; 0: n)
    plant_pos: Optional[torch.Tensor] = None  # int64 [p]
    plant_rows: Optional[torch.Tensor] = None  # bf16 [p, D]
    corpus: Optional[torch.Tensor] = None  # replaces the base corpus, CPU or device
    labels: Optional[torch.Tensor] = None  # int32 [rows]
    want: Optional[torch.Tensor] = None  # int32 [B]
    within: Dict[int, Sequence[int]] = field(default_factory=dict)  # every returned idx of the row lies in it
    contains: Dict[int, Sequence[int]] = field(default_factory=dict)  # all of it is returned for the row
    exact: Optional[torch.Tensor] = None  # int64 [B, k]: idx must equal it
    ordered: Dict[int, Sequence[int]] = field(default_factory=dict)  # the row's idx, in order
    min_gap_E: float = 0.0  # precondition: consecutive top-(k+1) gaps of sims64 >= this many E
    all_below: Optional[float] = None  # precondition: every true score below it
    idx_below: Optional[int] = None  # every returned idx below it


def contiguous_positions(start: int, count: int) -> List[int]:
    assert start % 64 == 0
    return list(range(start, start + count))


def scattered_positions(n: int, count: int, B: int, pc, gen) -> List[int]:
    """Tile and chunk edges first (last column, column 0, both sides of the
    first 128 boundary, both sides of a chunk boundary of the 128- and the
    256-tile plan), then seeded random positions elsewhere."""
    c128 = chunk_columns(B, n, pc["BN"], pc)
    c256 = chunk_columns(B, n, pc["BN8"], pc)
    edges = []
    for p in (n - 1, 0, 128, 127, c256 - 1, c256, c128 - 1, c128):
        if 0 <= p < n and p not in edges:
            edges.append(p)
    pos = edges[:count]
    taken = set(edges)
    while len(pos) < count:
        p = int(torch.randint(0, n, (1,), generator=gen))
        if p not in taken:
            taken.add(p)
            pos.append(p)
    return pos


def dup_sizes(k: int) -> List[int]:
    return sorted({s for s in (k - 1, k, 8, 9, 24) if s > 0})


def dup_case(d, n, B, k, size, placement, pc, seed, filtered_half=False) -> Case:
    """|S| = size bit-identical copies of one row; query row B-1 is that row.
    filtered_half: every second copy gets label 1 and the query wants label 0,
    so only the other copies are eligible."""
    g = torch.Generator().manual_seed(seed)
    q = rand_unit(B, d, seed + 1)
    row = rand_unit(1, d, seed + 2)
    qr = B - 1
    q[qr] = row[0]
    if placement == "contig":
        hi = min(n, pc["MIN_N_EMIT"]) - size
        start = int(torch.randint(0, hi // 64, (1,), generator=g)) * 64
        pos = contiguous_positions(start, size)
    else:
        pos = scattered_positions(n, size, B, pc, g)
    case = Case(
        name="dup[%s,|S|=%d,k=%d,B=%d,N=%d]" % (placement, size, k, B, n), q=q, n=n, k=k,
        plant_pos=torch.tensor(pos, dtype=torch.int64), plant_rows=row.expand(size, d).contiguous(),
    )
    members = pos
    if filtered_half:
        labels = torch.zeros(n, dtype=torch.int32)
        labels[torch.tensor(pos[1::2], dtype=torch.int64)] = 1
        want = torch.full((B,), -1, dtype=torch.int32)
        want[qr] = 0
        want[0] = 0
        case.labels, case.want = labels, want
        members = pos[0::2]
        case.name += "[half labelled away]"
    if len(members) >= k:
        case.within[qr] = members
    else:
        case.contains[qr] = members
    return case


def neardup_case(d, n, B, pc, seed) -> Case:
    """8 contiguous rows at cosines 0.95 .. 0.60 to query row B-1, k = 8."""
    g = torch.Generator().manual_seed(seed)
    q = rand_unit(B, d, seed + 1)
    qr = B - 1
    rows = near_rows(q[qr : qr + 1], g)[0]
    hi = min(n, pc["MIN_N_EMIT"]) - 8
    start = int(torch.randint(0, hi // 64, (1,), generator=g)) * 64
    pos = contiguous_positions(start, 8)
    return Case(
        name="neardup[B=%d,N=%d,start=%d]" % (B, n, start), q=q, n=n, k=8,
        plant_pos=torch.tensor(pos, dtype=torch.int64), plant_rows=rows,
        ordered={qr: pos}, min_gap_E=100.0,
    )


def flooded_case(d, n, B, k, seed) -> Case:
    """Every corpus row is one row: all n columns tie for every query."""
    row = rand_unit(1, d, seed)
    q = rand_unit(B, d, seed + 1)
    q[B - 1] = row[0]
    return Case(name="flooded[B=%d,N=%d,k=%d]" % (B, n, k), q=q, n=n, k=k,
                corpus=row.expand(n, d))


def required_positions(n: int, step: int) -> List[int]:
    """Both sides of every multiple of ``step``, column 0 and every column of
    the last 128-column tile."""
    req = {0}
    for s in range(step, n, step):
        req.update((s - 1, s))
    req.update(range((n - 1) // 128 * 128, n))
    return sorted(req)


def planted_case(d, n, nq, step, seed) -> Case:
    """Each of nq queries gets its own near-duplicate run of 8 at seeded
    positions that together cover required_positions(n, step); k = 8 and the
    answer is the planted positions in order."""
    g = torch.Generator().manual_seed(seed)
    req = required_positions(n, step)
    total = nq * 8
    assert len(req) <= total <= n, (len(req), total, n)
    rest = torch.ones(n, dtype=torch.bool)
    rest[torch.tensor(req)] = False
    rest = rest.nonzero()[:, 0]
    fill = rest[torch.randperm(rest.numel(), generator=g)[: total - len(req)]]
    pos = torch.cat([torch.tensor(req, dtype=torch.int64), fill])
    pos = pos[torch.randperm(total, generator=g)].view(nq, 8)
    q = rand_unit(nq, d, seed + 1)
    rows = near_rows(q, g)
    return Case(
        name="planted[nq=%d,N=%d,step=%d]" % (nq, n, step), q=q, n=n, k=8,
        plant_pos=pos.reshape(-1), plant_rows=rows.reshape(total, d), exact=pos,
        min_gap_E=100.0,
    )


def planted_queries_needed(n: int, step: int, multiple: int = 8) -> int:
    need = (len(required_positions(n, step)) + 7) // 8
    return (need + multiple - 1) // multiple * multiple


def floor_case(d, n, nq, seed) -> Case:
    """Plain random queries at k = 8: no slack between the emission floor
    (the 8th best of the sample) and the 8th best of the corpus."""
    return Case(name="k8floor[nq=%d,N=%d]" % (nq, n), q=rand_unit(nq, d, seed), n=n, k=8)


def negative_corpus(d, n, seed):
    """(u, corpus): c_j = normalize(u + 0.5 * g_j) with unit g_j, so every
    cosine to -u is about -0.89."""
    u = rand_unit(1, d, seed).float()
    gj = rand_unit(n, d, seed + 1).float()
    c = u + 0.5 * gj
    c /= c.norm(dim=-1, keepdim=True)
    return u[0], c.to(torch.bfloat16)


def negative_case(u, corpus, n, B, k, seed) -> Case:
    """Queries -u (row 0 exactly, the others slightly perturbed): every real
    score is negative, so a padded column or an empty list slot scoring 0
    would win."""
    d = u.shape[0]
    q = -u[None, :] + 0.05 * rand_unit(B, d, seed).float()
    q[0] = -u
    q /= q.norm(dim=-1, keepdim=True)
    return Case(name="negative[B=%d,N=%d,k=%d]" % (B, n, k), q=q.to(torch.bfloat16), n=n, k=k,
                corpus=corpus[:n], all_below=-0.5)


def poison_case(d, valid_n, B, k, seed) -> Case:
    """300 rows past valid_n: for every query a copy scaled by 4 (score 4.0),
    the rest NaN rows."""
    q = rand_unit(B, d, seed)
    extra = 300
    rows = torch.full((extra, d), float("nan"), dtype=torch.bfloat16)
    reps = (extra - 8) // B
    for b in range(B):
        rows[b * reps : (b + 1) * reps] = (4.0 * q[b].float()).to(torch.bfloat16)
    return Case(
        name="poison[B=%d,valid_n=%d,k=%d]" % (B, valid_n, k), q=q, n=valid_n, k=k,
        rows=valid_n + extra, plant_pos=torch.arange(valid_n, valid_n + extra),
        plant_rows=rows, idx_below=valid_n,
    )


def zero_query_case(d, n, B, k, seed) -> Case:
    """Query row 0 is all zeros: every score is 0, any k distinct columns."""
    q = rand_unit(B, d, seed)
    q[0] = 0
    return Case(name="zeroquery[B=%d,N=%d,k=%d]" % (B, n, k), q=q, n=n, k=k)


def store_case(d, seed) -> Case:
    """1,300 rows for a three-segment store of 512-row segments: five copies
    of query row 0 in the first segment and five in the third, k = 8."""
    n = 1300
    q = rand_unit(4, d, seed)
    pos = [3, 200, 201, 510, 511, 1024, 1025, 1100, 1298, 1299]
    return Case(
        name="store[3 segments]", q=q, n=n, k=8,
        plant_pos=torch.tensor(pos, dtype=torch.int64), plant_rows=q[:1].expand(len(pos), d).contiguous(),
        within={0: pos},
    )


@dataclass
class IvfCase:
    case: Case
    offsets: torch.Tensor  # int64 [L + 1]
    ids: torch.Tensor  # int32 [n_idx]
    probes: torch.Tensor  # int32 [B, nprobe]
    tail_lo: int
    tail_hi: int
    eligible: torch.Tensor  # bool [B, n]: the rows each query scans


def ivf_case(d, seed) -> IvfCase:
    """3,000 rows: 2,400 in eight inverted lists of 300, 600 in the tail.
    Query 0 probes lists 1 and 5; three copies of it sit in each, three in
    the tail and three more in list 3, which it does not probe. k = 8: the
    answer is 8 distinct ones of the 9 scanned copies."""
    g = torch.Generator().manual_seed(seed)
    n, n_idx, L = 3000, 2400, 8
    ids = torch.randperm(n_idx, generator=g).to(torch.int32)
    off = torch.arange(L + 1, dtype=torch.int64) * (n_idx // L)
    probes = torch.tensor([[1, 5], [2, -1]], dtype=torch.int32)
    q = rand_unit(2, d, seed + 1)

    def members(l, where):
        return [int(ids[int(off[l]) + w]) for w in where]

    scanned = members(1, (0, 150, 299)) + members(5, (7, 8, 9)) + [n_idx, n_idx + 300, n - 1]
    hidden = members(3, (0, 1, 2))
    pos = scanned + hidden
    elig = torch.zeros(2, n, dtype=torch.bool)
    for b, row in enumerate(probes.tolist()):
        for l in row:
            if 0 <= l < L:
                elig[b, ids[int(off[l]) : int(off[l + 1])].long()] = True
        elig[b, n_idx:n] = True
    case = Case(
        name="ivf[copies in two probed lists, an unprobed list and the tail]", q=q, n=n, k=8,
        plant_pos=torch.tensor(pos, dtype=torch.int64), plant_rows=q[:1].expand(len(pos), d).contiguous(),
        within={0: scanned},
    )
    return IvfCase(case, off, ids, probes, n_idx, n, elig)


# ---------------------------------------------------------------------------
# running a case
# ---------------------------------------------------------------------------

def materialise(case: Case, base: torch.Tensor) -> torch.Tensor:
    """The case's corpus on base's device: a clone of the base prefix with
    the planted rows written in (the base itself is never modified)."""
    dev = base.device
    rows = case.rows or case.n
    if case.corpus is not None:
        c = case.corpus.to(dev)
        c = c.contiguous() if c.shape[0] == rows else torch.cat(
            [c, torch.zeros(rows - c.shape[0], c.shape[1], dtype=c.dtype, device=dev)])
        if case.plant_pos is None:
            return c
        c = c.clone()
    else:
        if rows <= base.shape[0]:
            c = base[:rows].clone()
        else:  # rows past the base are planted below
            c = torch.cat([base, base[: rows - base.shape[0]]], dim=0)
    if case.plant_pos is not None:
        c[case.plant_pos.to(dev)] = case.plant_rows.to(dev)
    return c


def eligibility(case: Case, dev) -> Optional[torch.Tensor]:
    if case.labels is None:
        return None
    w = case.want.to(dev).long()[:, None]
    return (w < 0) | (case.labels[: case.n].to(dev).long()[None, :] == w)


def judge(case: Case, scores, idx, sims64, eligible=None) -> None:
    """The checker plus what the case's data fixes exactly."""
    d = case.q.shape[1]
    E = tolerance(d)
    if case.all_below is not None:
        assert float(sims64.max()) < case.all_below, (case.name, float(sims64.max()))
    if case.min_gap_E:
        judged = sims64[sorted(case.ordered)] if case.ordered else sims64  # the rows with a fixed order
        top = torch.topk(judged, min(case.k + 1, sims64.shape[1]), dim=1).values
        gap = float((top[:, :-1] - top[:, 1:]).min())
        assert gap >= case.min_gap_E * E, "%s: precondition: min gap %.3g < %g E" % (
            case.name, gap, case.min_gap_E)
    check_topk(scores, idx, sims64, case.k, d, eligible, what=case.name)
    got = idx.cpu()
    if case.idx_below is not None:
        assert bool((got < case.idx_below).all()), (case.name, got.max().item())
    for r, members in case.within.items():
        outside = sorted(set(got[r].tolist()) - set(members))
        assert not outside, "%s: row %d returned %s outside the duplicate set %s (idx=%s)" % (
            case.name, r, outside, sorted(members), got[r].tolist())
    for r, members in case.contains.items():
        lost = sorted(set(members) - set(got[r].tolist()))
        assert not lost, "%s: row %d lost planted columns %s (idx=%s, scores=%s)" % (
            case.name, r, lost, got[r].tolist(), scores[r].tolist())
    for r, members in case.ordered.items():
        assert got[r].tolist() == list(members), "%s: row %d returned %s, planted order is %s (scores=%s)" % (
            case.name, r, got[r].tolist(), list(members), scores[r].tolist())
    if case.exact is not None:
        bad = (got != case.exact).any(dim=1).nonzero()[:, 0].tolist()
        assert not bad, "%s: %d queries differ from their planted positions; first row %d: got %s want %s" % (
            case.name, len(bad), bad[0], got[bad[0]].tolist(), case.exact[bad[0]].tolist())


# a search gets the queries of one call, the corpus, the case and the index
# of the call's first query row within the case
Search = Callable[[torch.Tensor, torch.Tensor, Case, int], tuple]


def _labels_want(case: Case, rows: int, b0: int, nb: int):
    """The case's labels and the call's wants; a case without labels gets
    one label everywhere and every want -1 (no restriction)."""
    labels = case.labels if case.labels is not None else torch.zeros(rows, dtype=torch.int32)
    if labels.shape[0] < rows:
        labels = torch.cat([labels, labels.new_zeros(rows - labels.shape[0])])
    want = case.want if case.want is not None else torch.full((case.q.shape[0],), -1, dtype=torch.int32)
    return labels, want[b0 : b0 + nb]


def search_topk(q, c, case, b0=0):
    from kakveda_amd import ops

    return ops.cosine_topk(q, c, case.k, valid_n=case.n)


def search_filtered(q, c, case, b0=0):
    from kakveda_amd import ops

    labels, want = _labels_want(case, c.shape[0], b0, q.shape[0])
    return ops.cosine_topk_filtered(q, c, labels.to(c.device), want.to(c.device), case.k, valid_n=case.n)


def search_topk_ref(q, c, case, b0=0):
    from kakveda_amd import ops

    return ops.cosine_topk_ref(q, c, case.k, case.n)


def search_filtered_ref(q, c, case, b0=0):
    from kakveda_amd import ops

    labels, want = _labels_want(case, c.shape[0], b0, q.shape[0])
    return ops.cosine_topk_filtered_ref(q, c, labels.to(c.device), want.to(c.device), case.k, case.n)


def run_case(case: Case, base: torch.Tensor, search: Search, batch: int = 0):
    """Materialise the case beside ``base``, search it (in calls of ``batch``
    query rows when given), compute sims64 on the same bf16 inputs and judge."""
    dev = base.device
    c = materialise(case, base)
    q = case.q.to(dev)
    B = q.shape[0]
    step = batch or B
    parts = []
    for b0 in range(0, B, step):
        parts.append(search(q[b0 : b0 + step], c, case, b0))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    scores = torch.cat([p[0] for p in parts], dim=0)
    idx = torch.cat([p[1] for p in parts], dim=0)
    sims64 = q.double() @ c[: case.n].double().t()
    judge(case, scores, idx, sims64, eligibility(case, dev))
    return scores, idx


# ---------------------------------------------------------------------------
# child process: settings the extension reads once per process
# ---------------------------------------------------------------------------

def child_cases(d, n, batches, pc, seed=7000):
    """The duplicate-block and k = 8 families at the given batch sizes."""
    cases = []
    for B in batches:
        for k in (5, 8):
            for placement in ("contig", "scattered"):
                for size in dup_sizes(k):
                    seed += 10
                    cases.append((dup_case(d, n, B, k, size, placement, pc, seed), 0))
    cases.append((floor_case(d, n, 64, seed + 10), 8))
    return cases


def child_main(argv) -> int:
    """``python tests/topk_adversarial.py D B[,B...]``: run child_cases on
    cuda:0 under whatever KAKVEDA_* environment the parent set; print one FAIL
    line per failing case and a CHILD summary; exit 1 on any failure."""
    sys.path.insert(0, REPO)
    d = int(argv[0])
    batches = [int(b) for b in argv[1].split(",")]
    pc = plan_constants()
    base = rand_unit(N_BASE, d, 1).to("cuda:0")
    failures = 0
    cases = child_cases(d, N_BASE, batches, pc)
    for case, batch in cases:
        try:
            run_case(case, base, search_topk, batch=batch)
        except AssertionError as exc:
            failures += 1
            print("FAIL %s" % str(exc).replace("\n", " ")[:600], flush=True)
    print("CHILD cases=%d failures=%d" % (len(cases), failures), flush=True)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1:]))
