"""GPU tests of the wide exact top-k, ops.cosine_topk_wide (8 < k <= 64).

Oracle: float64 inner products of the same bf16 inputs under
tests/topk_adversarial.py::check_topk (tie-aware, E = D * 2^-23). The shapes
walk the plan of kakveda_amd/ops/hip/knn_wide_plan.h: the streaming kernel
(B <= 8), the 8-phase kernel (B > 8, unfiltered, N >= 4,096), the groups of 8
(filtered batches, small corpora, fallback slices), with and without a floor,
and the sliced overflow fallback through both of its triggers.
"""

import pytest
import torch

import topk_adversarial as ta

pytestmark = pytest.mark.gpu

D = 128
N = ta.N_BASE  # 65,700: 36 real columns in the last 256-column tile
N_SMALL = 4_100  # below the emission gate of the k <= 8 search


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def base():
    """The shared corpus; never modified (cases that plant rows clone it)."""
    return ta.rand_unit(N, D, 1).to(_dev())


@pytest.fixture(scope="module")
def queries():
    return ta.rand_unit(130, D, 2).to(_dev())


_SIMS = {}


def _sims64(q, c, key=None):
    """float64 scores, computed once per (batch, corpus) of the shared data."""
    if key is None:
        return q.double() @ c.double().t()
    if key not in _SIMS:
        _SIMS[key] = q.double() @ c.double().t()
    return _SIMS[key]


def _wide(q, c, k, **kw):
    from kakveda_amd import ops

    out = ops.cosine_topk_wide(q, c, k, **kw)
    torch.cuda.synchronize()
    return out


def _search_wide(q, c, case, b0=0):
    from kakveda_amd import ops

    if case.labels is None:
        return ops.cosine_topk_wide(q, c, case.k, valid_n=case.n)
    labels, want = ta._labels_want(case, c.shape[0], b0, q.shape[0])
    return ops.cosine_topk_wide(q, c, case.k, valid_n=case.n, labels=labels.to(c.device),
                                want=want.to(c.device))


# ---------------------------------------------------------------------------
# paths and k
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [N, N_SMALL])
@pytest.mark.parametrize("B", [1, 8, 9, 130])
@pytest.mark.parametrize("k", [9, 16, 33, 64])
def test_paths_and_k(base, queries, k, B, n):
    q, c = queries[:B], base[:n]
    s, i = _wide(q, c, k)
    ta.check_topk(s, i, _sims64(q, c, (B, n)), k, D, what="wide[k=%d,B=%d,N=%d]" % (k, B, n))
    # the packed words are unique per column: equal scores come index-ascending
    tie = s[:, 1:] == s[:, :-1]
    assert bool((~tie | (i[:, 1:] > i[:, :-1])).all())


@pytest.mark.parametrize("B", [3, 9])
def test_d768(B):
    c = ta.rand_unit(20_000, 768, 11).to(_dev())
    q = ta.rand_unit(B, 768, 12).to(_dev())
    s, i = _wide(q, c, 33)
    ta.check_topk(s, i, _sims64(q, c), 33, 768, what="wide[D=768,B=%d]" % B)


def test_small_k_delegates_and_large_k_pads(base, queries):
    from kakveda_amd import ops

    q = queries[:9]
    s5, i5 = _wide(q, base, 5)
    r5, j5 = ops.cosine_topk(q, base, 5)
    assert torch.equal(s5, r5) and torch.equal(i5, j5)
    s, i = _wide(q, base, 70)
    assert s.shape == (9, 70)
    assert bool((i[:, 64:] == -1).all()) and bool((s[:, 64:] == float("-inf")).all())
    ta.check_topk(s[:, :64].contiguous(), i[:, :64].contiguous(), _sims64(q, base, (9, N)), 64, D,
                  what="wide[k=70 -> 64]")


# ---------------------------------------------------------------------------
# too few rows, no floor
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("n", [40, 64])
def test_fewer_rows_than_k(base, queries, n, B):
    q, c = queries[:B], base[:n]
    s, i = _wide(q, c, 64)
    ta.check_topk(s, i, _sims64(q, c), 64, D, what="wide[N=%d,k=64,B=%d]" % (n, B))
    assert int((i >= 0).sum()) == B * n
    assert bool((i[:, n:] == -1).all()) and bool((s[:, n:] == float("-inf")).all())


@pytest.mark.parametrize("B", [4, 9])
def test_valid_n_poison(B):
    """Rows past valid_n would win (each is 4 * a query, score 4) or are NaN."""
    case = ta.poison_case(D, 1_000, B, 33, seed=21)
    case.rows = 4_100
    pos = torch.arange(1_000, 4_100)
    rows = case.plant_rows[torch.arange(pos.numel()) % case.plant_rows.shape[0]]
    case.plant_pos, case.plant_rows = pos, rows
    small = ta.rand_unit(4_100, D, 22).to(_dev())
    ta.run_case(case, small, _search_wide)


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("n,k", [(500, 33), (N_SMALL, 64), (1_031, 16)])
def test_no_floor_branch(base, queries, n, k, B):
    """The prepass partials hold 8 entries per 1,024 columns: 8, 36 and 15 of
    them here, fewer than k, so no floor exists and every row is emitted."""
    q, c = queries[:B], base[:n]
    s, i = _wide(q, c, k)
    ta.check_topk(s, i, _sims64(q, c), k, D, what="wide[no floor,N=%d,k=%d,B=%d]" % (n, k, B))


# ---------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("placement", ["contig", "scattered"])
def test_duplicate_block_of_100(base, placement, B):
    """100 bit-identical best rows at k = 64, contiguous and scattered across
    tile and chunk edges: 64 distinct members of the block come back."""
    pc = ta.plan_constants()
    case = ta.dup_case(D, N, B, 64, 100, placement, pc, seed=31)
    s, i = ta.run_case(case, base, _search_wide)
    got = i[B - 1].tolist()
    assert len(set(got)) == 64 and set(got) <= set(case.within[B - 1])


# ---------------------------------------------------------------------------
# the floor must be the k-th best, not the 8th
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 9])
def test_floor_is_not_the_list_minimum(base, B):
    """8 rows at cosine 0.9 inside one 512-column half-list of the prepass
    (columns 0..7: one 128-column tile, its first 64 columns) and 56 rows at
    cosine 0.5 spread over the corpus. Precondition, checked on the data: every
    other row scores more than 100 E below the lowest planted one, so the
    answer is those 64 and nothing else. All 64 must come back. The prepass list kernel publishes the minima of its
    8-deep lists, here about 0.9, into the threshold array it is given: an
    implementation that lets those reach the main launch's floor (by handing
    the prepass the array, or by reusing it) emits nothing below 0.9 and loses
    the 56."""
    g = torch.Generator().manual_seed(41)
    q = ta.rand_unit(B, D, 42)
    qr = B - 1
    rows = ta.near_rows(q[qr:qr + 1], g, cosines=[0.9] * 8 + [0.5] * 56)[0]
    spread = torch.randperm(N - 1024, generator=g)[:56] + 1024
    pos = torch.cat([torch.arange(8), spread])
    case = ta.Case(name="pitfall1[B=%d]" % B, q=q, n=N, k=64, plant_pos=pos, plant_rows=rows,
                   contains={qr: pos.tolist()})
    s, i = ta.run_case(case, base, _search_wide)
    sims = q[qr].double().to(_dev()) @ ta.materialise(case, base).double().t()
    others = sims.clone()
    others[pos.to(_dev())] = -1
    lowest = float(sims[pos.to(_dev())].min())
    assert lowest > 0.48 and float(others.max()) < lowest - 100 * ta.tolerance(D)
    assert sorted(i[qr].tolist()) == sorted(pos.tolist())


# ---------------------------------------------------------------------------
# filtered
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [4, 20])
@pytest.mark.parametrize("k", [16, 64])
def test_filtered(base, queries, k, B):
    """Label 1 on 10% of the rows, label 2 on 30 rows only (30 results at any
    k here), want = -1 riders in the same batch. B = 20 is served in groups of
    8 queries through the filtered streaming kernel."""
    g = torch.Generator().manual_seed(51)
    labels = torch.zeros(N, dtype=torch.int32)
    labels[torch.rand(N, generator=g) < 0.1] = 1
    labels[torch.randperm(N, generator=g)[:30]] = 2
    want = torch.tensor(([1, 2, -1, 1] * 5)[:B], dtype=torch.int32)
    want[B - 1] = 2
    q = queries[:B]
    labels, want = labels.to(_dev()), want.to(_dev())
    s, i = _wide(q, base, k, labels=labels, want=want)
    elig = (want.long()[:, None] < 0) | (labels.long()[None, :] == want.long()[:, None])
    ta.check_topk(s, i, _sims64(q, base, (B, N)), k, D, eligible=elig,
                  what="wide filtered[k=%d,B=%d]" % (k, B))
    assert int((i[1] >= 0).sum()) == min(k, 30) and int((i[B - 1] >= 0).sum()) == min(k, 30)
    assert int((i[2] >= 0).sum()) == k


def test_filtered_small_corpus(base, queries):
    q = queries[:20]
    labels = (torch.arange(N_SMALL) % 7).to(torch.int32).to(_dev())
    want = torch.tensor([3, -1, 0, 99] * 5, dtype=torch.int32).to(_dev())
    s, i = _wide(q, base[:N_SMALL], 33, labels=labels, want=want)
    elig = (want.long()[:, None] < 0) | (labels.long()[None, :] == want.long()[:, None])
    ta.check_topk(s, i, _sims64(q, base[:N_SMALL]), 33, D, eligible=elig, what="wide filtered small")
    assert bool((i[3] == -1).all())


# ---------------------------------------------------------------------------
# overflow fallback
# ---------------------------------------------------------------------------

def _run_counted(case, corpus_base, **kw):
    from kakveda_amd import ops

    def search(q, c, case, b0=0):
        return ops.cosine_topk_wide(q, c, case.k, valid_n=case.n, **kw)

    before = ops.wide_overflow_fallbacks
    out = ta.run_case(case, corpus_base, search)
    return out, ops.wide_overflow_fallbacks - before


@pytest.mark.parametrize("B", [1, 9])
def test_overflow_fallback_by_count(base, B):
    """cap = 128 with 200 bit-identical rows as a query's best: every one of
    them clears any valid floor, so the query's count exceeds cap and the
    batch is answered over slices of 128 rows. The counter rising by exactly
    one is what keeps this test from passing without overflowing."""
    pc = ta.plan_constants()
    case = ta.dup_case(D, N_SMALL, B, 64, 200, "scattered", pc, seed=61)
    (s, i), rose = _run_counted(case, base, cap=128)
    assert rose == 1
    # without the small cap the same request does not overflow
    (_, i2), rose2 = _run_counted(case, base)
    assert rose2 == 0
    assert set(i2[B - 1].tolist()) <= set(case.within[B - 1])


def test_overflow_fallback_by_segment(base):
    """seg = 1, the smallest record segment, at B = 9: any block of the
    8-phase launch with two records poisons its row tile's count, and the
    batch is answered over slices of cap rows."""
    pc = ta.plan_constants()
    case = ta.dup_case(D, N, 9, 64, 200, "scattered", pc, seed=71)
    (s, i), rose = _run_counted(case, base, seg=1)
    assert rose == 1
    case2 = ta.dup_case(D, N_SMALL, 9, 64, 200, "contig", pc, seed=72)
    (_, _), rose = _run_counted(case2, base, cap=128, seg=1)
    assert rose == 1


# ---------------------------------------------------------------------------
# agreement with the k <= 8 search
# ---------------------------------------------------------------------------

def test_prefix_agrees_with_k8(base, queries):
    from kakveda_amd import ops

    q = queries[:9]
    s16, _ = _wide(q, base, 16)
    s8, _ = ops.cosine_topk(q, base, 8)
    torch.cuda.synchronize()
    assert float((s16[:, :8].double() - s8.double()).abs().max()) <= ta.tolerance(D)


# ---------------------------------------------------------------------------
# store and engine
# ---------------------------------------------------------------------------

def test_store_two_segments_and_sharded(queries):
    from kakveda_amd.gfkb.engine import EmbeddingStore
    from kakveda_amd.parallel.sharded import ShardedStore

    rows = ta.rand_unit(9_000, D, 81).to(_dev())
    q = queries[:9]
    sims = _sims64(q, rows)
    store = EmbeddingStore(D, device="cuda", capacity=5_000, segment_rows=5_000)
    store.append(rows[:4_000])
    store.append(rows[4_000:])
    assert len(store._live_segments(store.count)) == 2
    s, i = store.search(q, 20)
    torch.cuda.synchronize()
    ta.check_topk(s, i, sims, 20, D, what="store wide, two segments")
    # an nprobe without an index and the int8 mirror do not apply
    s2, i2 = store.search(q, 20, nprobe=4)
    assert torch.equal(i2, i)
    flat = EmbeddingStore(D, device="cuda", capacity=9_000)
    flat.append(rows)
    fs, fi = flat.search(q, 20)
    ta.check_topk(fs, fi, sims, 20, D, what="store wide, flat")
    assert float((fs.double() - s.double()).abs().max()) <= ta.tolerance(D)
    sharded = ShardedStore(D, device="cuda", capacity=9_000)
    assert sharded.world == 1
    sharded.append(rows)
    ss, si = sharded.search(q, 20)
    torch.cuda.synchronize()
    assert torch.equal(si, fi) and torch.equal(ss, fs)
    # filtered through the store: labels 0..2 round-robin
    lab = EmbeddingStore(D, device="cuda", capacity=5_000, segment_rows=5_000)
    labels = (torch.arange(9_000) % 3).to(torch.int32)
    lab.append(rows[:4_000], labels[:4_000])
    lab.append(rows[4_000:], labels[4_000:])
    want = torch.tensor([1, -1, 2] * 3, dtype=torch.int32)
    ls, li = lab.search(q, 20, want=want)
    elig = (want.long()[:, None] < 0) | (labels.long()[None, :] == want.long()[:, None])
    ta.check_topk(ls, li, sims, 20, D, eligible=elig.to(_dev()), what="store wide, filtered")


def test_engine_top_k_20(tmp_path):
    from kakveda_amd.gfkb.engine import GfkbEngine

    eng = GfkbEngine(data_dir=str(tmp_path), device="cuda", dim=256, hash_dim=4096)
    for j in range(30):
        eng.upsert_failure(
            "TIMEOUT" if j % 3 == 0 else "HALLUCINATION_CITATION",
            "intent_tags:intent:t%d | prompt_hint:probe number %d of the wide test | tools: | env_keys:e2e"
            % (j % 7, j), {"j": j}, app_id="app-%d" % (j % 3))
    sig = "intent_tags:intent:t3 | prompt_hint:probe number 3 of the wide test | tools: | env_keys:e2e"
    got = eng.match(sig, top_k=20)
    assert len(got) == 20 and len({m.failure_id for m in got}) == 20
    assert got[0].score > 0.98
    scores = [m.score for m in got]
    assert scores == sorted(scores, reverse=True)
    typed = eng.match(sig, failure_type="TIMEOUT", top_k=20, filter_first=True)
    assert len(typed) == 10 and all(m.failure_type == "TIMEOUT" for m in typed)
    assert len(eng.match(sig)) == 5
