"""GPU tests of the routed (IVF) search kernels: ivf_route_scores and
ivf_scan_topk_kernel behind ops.ivf_scan_topk / ops.ivf_search.

Oracle: the plain-torch references (ops.ivf_scan_topk_ref / ivf_search_ref,
fp32) on the same bf16 inputs and the same index arrays — the contract is
deterministic given the index. For every returned id the tests assert that
it lies in the query's candidate set (probed lists plus tail, below
valid_n) and achieves its score; pads must sit exactly where the oracle
pads. Every hand-built id table is validated on the CPU before it reaches a
kernel.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 768
N_ROWS = 6000
LENS = [0, 1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 3000]
N_IDX = sum(LENS)  # 3889


def _dev():
    return torch.device("cuda:0")


def _rand_unit(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float32, device=_dev())
    x = x / x.norm(dim=-1, keepdim=True)
    return x.to(torch.bfloat16)


def _hand_index(n_idx, lens, seed):
    """A seeded permutation of [0, n_idx) cut into lists of ``lens``,
    validated as an IvfIndex before any kernel sees it."""
    from kakveda_amd.gfkb.ivf import IvfIndex

    assert sum(lens) == n_idx
    g = torch.Generator().manual_seed(seed)
    ids = torch.randperm(n_idx, generator=g).to(torch.int32)
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens), 0)
    IvfIndex(
        centroids=torch.zeros(len(lens), 8), offsets=off, ids=ids, n_indexed=n_idx,
        n_lists=len(lens), max_list_len=max(lens),
    ).validate()
    return off.to(_dev()), ids.to(_dev())


def _probes(B, n_lists, nprobe, seed):
    """Distinct random lists per query with -1 padding in the odd rows; row 0
    probes only the empty list 0 and pads."""
    g = torch.Generator().manual_seed(seed)
    p = torch.stack([torch.randperm(n_lists, generator=g)[:nprobe] for _ in range(B)])
    p = p.to(torch.int32)
    p[1::2, nprobe // 2] = -1
    p[0] = -1
    p[0, 1] = 0
    if B > 2:  # the 3000-row list and the one-row list, every time
        p[2, 0], p[2, 1] = 11, 1
        p[2, 2:] = torch.tensor([i for i in range(2, n_lists) if i != 11][: nprobe - 2])
    return p.to(_dev())


@pytest.fixture(scope="module")
def corpus():
    """6,000 unit rows shared by the module; never modified."""
    return _rand_unit(N_ROWS, D, seed=2)


@pytest.fixture(scope="module")
def queries(corpus):
    """Perturbed corpus rows: one near-duplicate each, the rest noise-level."""
    g = torch.Generator(device="cuda").manual_seed(9)
    base = corpus[torch.randperm(N_ROWS, generator=g, device=_dev())[:20]].float()
    q = base + 0.03 * torch.randn(20, D, generator=g, device=_dev())
    return (q / q.norm(dim=-1, keepdim=True)).to(torch.bfloat16)


@pytest.fixture(scope="module")
def index():
    return _hand_index(N_IDX, LENS, seed=3)


def _cat(segments):
    return segments if isinstance(segments, torch.Tensor) else torch.cat(list(segments), 0)


def _candidates(B, n_rows, off, ids, probes, valid_n, tail_lo, tail_hi):
    L = off.shape[0] - 1
    mask = torch.zeros(B, n_rows, dtype=torch.bool, device=_dev())
    o = off.tolist()
    for b, row in enumerate(probes.tolist()):
        for l in row:
            if 0 <= l < L:
                mask[b, ids[o[l] : o[l + 1]].long()] = True
        mask[b, tail_lo:tail_hi] = True
    mask[:, valid_n:] = False
    return mask


def _check(q, segments, off, ids, probes, k, valid_n, tail_lo, tail_hi, max_list_len=0):
    from kakveda_amd import ops

    B = q.shape[0]
    scores, idx = ops.ivf_scan_topk(
        q, segments, off, ids, probes, k, valid_n, tail_lo, tail_hi, max_list_len
    )
    torch.cuda.synchronize()
    ref_s, ref_i = ops.ivf_scan_topk_ref(
        q, segments, off, ids, probes, k, valid_n, tail_lo, tail_hi
    )
    rows = _cat(segments)
    sims = q.float() @ rows.float().t()
    cand = _candidates(B, rows.shape[0], off, ids, probes, valid_n, tail_lo, tail_hi)

    assert scores.shape == (B, k) and idx.shape == (B, k)
    assert scores.dtype == torch.float32 and idx.dtype == torch.int64
    assert (scores[:, :-1] >= scores[:, 1:] - 1e-6).all()
    # pads exactly where the oracle pads
    ref_pad = ref_i < 0
    assert torch.equal(idx < 0, ref_pad), (idx, ref_i)
    assert (idx[ref_pad] == -1).all()
    assert (scores[ref_pad] == float("-inf")).all()
    hit = ~ref_pad
    assert torch.allclose(scores[hit], ref_s[hit], atol=2e-2, rtol=1e-2)
    # every returned id is a candidate of its query, once, and achieves its score
    safe = idx.clamp_min(0)
    assert cand.gather(1, safe)[hit].all()
    assert (idx[hit] < valid_n).all()
    if hit.any():
        assert (sims.gather(1, safe)[hit] - scores[hit]).abs().max().item() <= 1e-4
    for b in range(B):
        live = idx[b][idx[b] >= 0].tolist()
        assert len(set(live)) == len(live)
    return scores, idx


CASES = [
    # (B, k, tail_len)
    (1, 1, 0), (1, 5, 13), (1, 8, 500),
    (3, 1, 1), (3, 5, 0), (3, 8, 13),
    (8, 1, 500), (8, 5, 1), (8, 8, 0),
    (20, 1, 13), (20, 5, 500), (20, 8, 1),
]


@pytest.mark.parametrize("B,k,tail", CASES)
def test_scan_hand_built_lists(corpus, queries, index, B, k, tail):
    off, ids = index
    probes = _probes(B, len(LENS), 5, seed=B * 10 + k)
    valid_n = N_IDX + tail
    scores, idx = _check(
        queries[:B], corpus, off, ids, probes, k, valid_n, N_IDX, valid_n,
        max_list_len=max(LENS),
    )
    if tail == 0:  # query 0 probes one empty list and pads: nothing to find
        assert (idx[0] == -1).all() and torch.isinf(scores[0]).all()


def test_scan_grid_does_not_change_the_result(corpus, queries, index):
    from kakveda_amd import ops

    off, ids = index
    probes = _probes(8, len(LENS), 5, seed=4)
    valid_n = N_IDX + 13
    a = ops.ivf_scan_topk(queries[:8], corpus, off, ids, probes, 8, valid_n, N_IDX, valid_n, 3000)
    # max_list_len unknown: one slice per source, every block walks its whole list
    b = _check(queries[:8], corpus, off, ids, probes, 8, valid_n, N_IDX, valid_n, 0)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    # k past KMAX pads, as cosine_topk does
    s, i = ops.ivf_scan_topk(queries[:2], corpus, off, ids, probes[:2], 10, valid_n, N_IDX, valid_n)
    assert s.shape == (2, 10) and (i[:, 8:] == -1).all() and torch.isinf(s[:, 8:]).all()


def test_scan_snapshot_valid_n_hides_listed_rows(corpus, queries, index):
    off, ids = index
    probes = _probes(8, len(LENS), 5, seed=6)
    # a snapshot below most listed ids and an empty tail
    _, idx = _check(queries[:8], corpus, off, ids, probes, 8, 2000, 2000, 2000, max(LENS))
    assert (idx < 2000).all()
    _check(queries[:3], corpus, off, ids, probes[:3], 5, 1, 1, 1, max(LENS))


@pytest.mark.parametrize("d", [64, 320])
def test_scan_other_dims(d, index):
    off, ids = index
    rows = _rand_unit(N_IDX + 40, d, seed=20 + d)
    q = _rand_unit(8, d, seed=30 + d)
    probes = _probes(8, len(LENS), 5, seed=d)
    _check(q, rows, off, ids, probes, 5, N_IDX + 40, N_IDX, N_IDX + 40, max(LENS))


def test_scan_three_segment_store(corpus, queries):
    # first segment 1000 rows, then the 2048-row quantum: lists of a random
    # permutation straddle both boundaries
    segs = [corpus[:1000], corpus[1000:3048].clone(), corpus[3048:5096].clone()]
    n_idx = 5000
    off, ids = _hand_index(n_idx, [0, 1, 999, 1000, 1048, 1952], seed=5)
    probes = _probes(8, 6, 3, seed=8)
    _check(queries[:8], segs, off, ids, probes, 8, 5096, n_idx, 5096, 1952)


def test_scan_grown_store_layout(corpus, queries):
    # the layout EmbeddingStore grows into: a first segment that stopped
    # doubling at 4000 rows (no multiple of the quantum), then 2048-row ones
    from kakveda_amd import ops
    from kakveda_amd.gfkb.engine import EmbeddingStore

    st = EmbeddingStore(D, device="cuda", capacity=1000, segment_rows=2048)
    st.append(corpus)
    assert st.n_segments == 2 and st._segments[0].shape[0] == 4000
    assert st._segments[1].shape[0] == 2048
    st.build_index(n_lists=16)
    s, i = st.search(queries, 5, nprobe=16)
    rs, ri = ops.cosine_topk(queries, corpus, 5)
    torch.cuda.synchronize()
    assert torch.allclose(s, rs, atol=2e-2, rtol=1e-2)
    sims = queries.float() @ corpus.float().t()
    assert (sims.gather(1, i) - s).abs().max().item() <= 1e-4
    for b in range(queries.shape[0]):
        diff = set(i[b].tolist()) ^ set(ri[b].tolist())
        assert all(abs(float(sims[b, j]) - float(rs[b, -1])) <= 1e-4 for j in diff)


def test_refused_before_launch(corpus, queries, index):
    from kakveda_amd import ops

    off, ids = index
    probes = _probes(2, len(LENS), 5, seed=1)
    q = queries[:2]
    too_many = [corpus[:8]] + [corpus[8:16]] * 64
    with pytest.raises(RuntimeError, match="at most 64"):
        ops.ivf_scan_topk(q, too_many, off, ids, probes, 5, 16, 16, 16)
    uneven = [corpus[:1000], corpus[1000:3000], corpus[3000:4000]]
    with pytest.raises(RuntimeError, match="same row count"):
        ops.ivf_scan_topk(q, uneven, off, ids, probes, 5, 4000, 4000, 4000)
    with pytest.raises(RuntimeError, match="valid_n"):
        ops.ivf_scan_topk(q, corpus, off, ids, probes, 5, N_ROWS + 1, N_IDX, N_ROWS + 1)
    with pytest.raises(RuntimeError, match="tail"):
        ops.ivf_scan_topk(q, corpus, off, ids, probes, 5, N_IDX, N_IDX, N_IDX + 1)
    with pytest.raises(RuntimeError, match="k must be"):
        ops._require_ext().ivf_scan_topk(q, [corpus], off, ids, probes, 9, N_IDX, N_IDX, N_IDX)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ops.ivf_scan_topk(q[:, :32].contiguous(), corpus[:, :32].contiguous(), off, ids,
                          probes, 5, N_IDX, N_IDX, N_IDX)


@pytest.mark.parametrize("L", [16, 100, 4096])
@pytest.mark.parametrize("B", [1, 8])
def test_route_scores(corpus, queries, L, B):
    from kakveda_amd import ops

    cen = corpus[:L]
    out = ops.ivf_route_scores(queries[:B], cen)
    torch.cuda.synchronize()
    ref = queries[:B].float() @ cen.float().t()
    assert out.shape == (B, L) and out.dtype == torch.float32
    # both sides add the same exact bf16 products in fp32, each within
    # (D-1) * 2^-24 of the true value for unit rows: < D * 2^-23 apart
    assert (out - ref).abs().max().item() <= D * 2.0 ** -23


def test_route_scores_more_than_one_query_group(corpus, queries):
    from kakveda_amd import ops

    out = ops.ivf_route_scores(queries, corpus[:100])  # B=20: groups of 8, 8, 4
    ref = queries.float() @ corpus[:100].float().t()
    assert (out - ref).abs().max().item() <= D * 2.0 ** -23


def test_store_end_to_end():
    from kakveda_amd import ops
    from kakveda_amd.gfkb.engine import EmbeddingStore

    n, centres = 70_000, 64
    g = torch.Generator(device="cuda").manual_seed(11)
    cen = torch.randn(centres, D, generator=g, device=_dev())
    cen = cen / cen.norm(dim=-1, keepdim=True)
    pick = torch.randint(0, centres, (n,), generator=g, device=_dev())
    x = cen[pick] + (0.8 / D ** 0.5) * torch.randn(n, D, generator=g, device=_dev())
    x = (x / x.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
    qsel = torch.randperm(n, generator=g, device=_dev())[:32]
    q = x[qsel].float() + (0.3 / D ** 0.5) * torch.randn(32, D, generator=g, device=_dev())
    q = (q / q.norm(dim=-1, keepdim=True)).to(torch.bfloat16)

    st = EmbeddingStore(D, device="cuda")
    st.adopt(x)
    idx = st.build_index(n_lists=64)
    assert idx.n_lists == 64 and idx.n_indexed == n and idx.centroids.dtype == torch.bfloat16

    # every list probed: the exact search's answer
    s, i = st.search(q, 5, nprobe=64)
    es, ei = ops.cosine_topk(q, x, 5)
    torch.cuda.synchronize()
    assert torch.allclose(s, es, atol=2e-2, rtol=1e-2)
    sims = q.float() @ x.float().t()
    assert (sims.gather(1, i) - s).abs().max().item() <= 1e-4
    # same id sets per row, up to ties at the k-th score
    for b in range(32):
        diff = set(i[b].tolist()) ^ set(ei[b].tolist())
        assert all(abs(float(sims[b, j]) - float(es[b, -1])) <= 1e-4 for j in diff)

    # nprobe=8 against the reference on the CPU, same index
    s8, i8 = st.search(q, 5, nprobe=8)
    torch.cuda.synchronize()
    rs, ri = ops.ivf_search_ref(
        q.cpu(), x.cpu(), idx.centroids.cpu(), idx.offsets.cpu(), idx.ids.cpu(), 8, 5, n, n
    )
    assert torch.equal(i8 < 0, (ri < 0).to(_dev()))
    assert torch.allclose(s8, rs.to(_dev()), atol=2e-2, rtol=1e-2)
    assert (sims.gather(1, i8.clamp_min(0)) - s8).abs().max().item() <= 1e-4
    same = (i8.cpu() == ri).float().mean().item()
    assert same >= 0.98, same  # ties and probe-boundary ulps only

    # a row appended after the build is found at once
    new = torch.randn(1, D, generator=g, device=_dev())
    new = (new / new.norm()).to(torch.bfloat16)
    row = st.append(new)
    s1, i1 = st.search(new, 1, nprobe=1)
    assert int(i1[0, 0]) == row and float(s1[0, 0]) > 0.99
