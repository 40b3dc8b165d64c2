"""GPU tests of the list-major routed scan: ivf_scan_grouped_kernel behind
ops.ivf_scan_topk(..., batched=True) / ops.ivf_search(..., batched=True) and
EmbeddingStore.search(..., batched=True).

Oracle: ops.ivf_scan_topk_ref (plain torch, fp32) on the same bf16 inputs and
the same index arrays. For every returned id the tests assert that it lies
in the query's candidate set (probed lists plus tail, below valid_n), is
unique in its row and achieves its score within 1e-4 of the fp32 inner
product; pads must sit exactly where the oracle pads, as (-inf, -1); the id
set may differ from the oracle's only by rows tied with the k-th score
within 1e-4. Every hand-built id table is validated as an IvfIndex on the
CPU before it reaches a kernel.

The list lengths sit around the kernel's 16-row MFMA step and 64-row block
step (15/16/17, 63/64/65), its 1024-row slice (3000 rows: 3 slices) and the
batch sizes around its 16-query tile.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 768
N_ROWS = 6000
LENS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 3000]
N_IDX = sum(LENS)  # 4129
N_LISTS = len(LENS)
BIG, ONE, EMPTY = 17, 1, 0  # the 3000-row, the one-row and the empty list
QT = 16
N_QUERIES = 100


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
    probes only the empty list and pads; row 2 the longest list and the
    one-row list first."""
    g = torch.Generator().manual_seed(seed)
    p = torch.stack([torch.randperm(n_lists, generator=g)[:nprobe] for _ in range(B)])
    p = p.to(torch.int32)
    p[1::2, nprobe // 2] = -1
    p[0] = -1
    p[0, 1] = EMPTY
    if B > 2:
        big = n_lists - 1
        p[2, 0], p[2, 1] = big, ONE
        rest = [i for i in range(2, n_lists) if i != big][: nprobe - 2]
        p[2, 2:] = torch.tensor(rest)
    return p.to(_dev())


@pytest.fixture(scope="module")
def corpus():
    """6,000 unit rows shared by the module; never modified."""
    return _rand_unit(N_ROWS, D, seed=2)


@pytest.fixture(scope="module")
def queries(corpus):
    """Perturbed corpus rows: one near-duplicate each, the rest noise-level."""
    g = torch.Generator(device="cuda").manual_seed(9)
    pick = torch.randperm(N_ROWS, generator=g, device=_dev())[:N_QUERIES]
    q = corpus[pick].float() + 0.03 * torch.randn(N_QUERIES, D, generator=g, device=_dev())
    return (q / q.norm(dim=-1, keepdim=True)).to(torch.bfloat16)


@pytest.fixture(scope="module")
def index():
    return _hand_index(N_IDX, LENS, seed=3)


@pytest.fixture(scope="module")
def sims(corpus, queries):
    """fp32 inner products of every query with every row; never modified."""
    return queries.float() @ corpus.float().t()


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


def _same_up_to_ties(idx, ref_i, ref_s, sims, tol=1e-4):
    """Id sets equal per row except for rows scoring within tol of the
    oracle's last live score."""
    for b in range(idx.shape[0]):
        mine = set(i for i in idx[b].tolist() if i >= 0)
        ref = set(i for i in ref_i[b].tolist() if i >= 0)
        if mine == ref:
            continue
        kth = float(ref_s[b][ref_i[b] >= 0][-1])
        for j in mine ^ ref:
            assert abs(float(sims[b, j]) - kth) <= tol, (b, j)


def _check(q, segments, off, ids, probes, k, valid_n, tail_lo, tail_hi,
           max_list_len=0, sims=None):
    from kakveda_amd import ops

    B = q.shape[0]
    scores, idx = ops.ivf_scan_topk(
        q, segments, off, ids, probes, k, valid_n, tail_lo, tail_hi, max_list_len,
        batched=True,
    )
    torch.cuda.synchronize()
    ref_s, ref_i = ops.ivf_scan_topk_ref(
        q, segments, off, ids, probes, k, valid_n, tail_lo, tail_hi
    )
    rows = _cat(segments)
    if sims is None:
        sims = q.float() @ rows.float().t()
    sims = sims[:B]
    cand = _candidates(B, rows.shape[0], off, ids, probes, valid_n, tail_lo, tail_hi)

    assert scores.shape == (B, k) and idx.shape == (B, k)
    assert scores.dtype == torch.float32 and idx.dtype == torch.int64
    assert (scores[:, :-1] >= scores[:, 1:] - 1e-6).all()
    # pads exactly where the oracle pads, as (-inf, -1)
    ref_pad = ref_i < 0
    assert torch.equal(idx < 0, ref_pad), (idx, ref_i)
    assert (idx[ref_pad] == -1).all()
    assert (scores[ref_pad] == float("-inf")).all()
    hit = ~ref_pad
    # every returned id is a candidate of its query, once, and achieves its score
    safe = idx.clamp_min(0)
    assert cand.gather(1, safe)[hit].all()
    assert (idx[hit] < valid_n).all()
    if hit.any():
        assert (sims.gather(1, safe)[hit] - scores[hit]).abs().max().item() <= 1e-4
    for b in range(B):
        live = idx[b][idx[b] >= 0].tolist()
        assert len(set(live)) == len(live)
    _same_up_to_ties(idx, ref_i, ref_s, sims)
    return scores, idx


@pytest.mark.parametrize("tail", [0, 1, 13, 500])
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("B", [1, QT - 1, QT, QT + 1, 2 * QT + 1, 100])
def test_scan_hand_built_lists(corpus, queries, index, sims, B, k, tail):
    from kakveda_amd import ops

    assert ops._require_ext().IVF_BATCH_QTILE == QT == ops.IVF_BATCH_QTILE
    off, ids = index
    probes = _probes(B, N_LISTS, 5, seed=B * 10 + k)
    valid_n = N_IDX + tail
    scores, idx = _check(
        queries[:B], corpus, off, ids, probes, k, valid_n, N_IDX, valid_n,
        max_list_len=max(LENS), sims=sims,
    )
    if tail == 0:  # query 0 probes one empty list and pads: nothing to find
        assert (idx[0] == -1).all() and torch.isinf(scores[0]).all()


def test_one_group_of_a_hundred(corpus, queries, index, sims):
    # all 100 queries probe the 3000-row list and the one-row list: one group
    # of 100 pairs per list, seven tiles of one list (six full, one of 4)
    from kakveda_amd import ops

    off, ids = index
    probes = torch.tensor([[BIG, ONE]] * 100, dtype=torch.int32, device=_dev())
    _, _, tiles, n_tiles = ops.ivf_group_probes(probes.cpu(), N_LISTS)
    nt = int(n_tiles[0])
    assert nt == 21 and (tiles[0, :nt] == BIG).sum() == 7
    _check(queries, corpus, off, ids, probes, 8, N_IDX + 13, N_IDX, N_IDX + 13,
           max(LENS), sims=sims)


def test_every_tile_a_one_query_tile(corpus, queries, index, sims):
    # query b probes list b alone: 18 groups of one pair (and the empty tail)
    off, ids = index
    probes = torch.arange(N_LISTS, dtype=torch.int32, device=_dev()).reshape(-1, 1)
    s, i = _check(queries[:N_LISTS], corpus, off, ids, probes, 8, N_IDX, N_IDX, N_IDX,
                  max(LENS), sims=sims)
    assert (i[EMPTY] == -1).all()  # the probed empty list pads fully
    assert (i[ONE, 1:] == -1).all() and i[ONE, 0] >= 0


def test_all_pad_row_and_probed_empty_list(corpus, queries, index, sims):
    off, ids = index
    probes = _probes(QT + 1, N_LISTS, 5, seed=12)
    probes[3] = -1            # probes nothing at all
    probes[5] = -1
    probes[5, 4] = EMPTY      # probes the empty list only
    probes[7, 0] = N_LISTS    # out-of-range ids are skipped like pads
    probes[7, 1] = N_LISTS + 100
    s, i = _check(queries[:QT + 1], corpus, off, ids, probes, 5, N_IDX, N_IDX, N_IDX,
                  max(LENS), sims=sims)
    for b in (0, 3, 5):
        assert (i[b] == -1).all() and (s[b] == float("-inf")).all()


def test_snapshot_valid_n_hides_listed_rows(corpus, queries, index, sims):
    off, ids = index
    probes = _probes(QT + 1, N_LISTS, 5, seed=6)
    # a snapshot below most listed ids and an empty tail: every id < 2000
    _, idx = _check(queries[:QT + 1], corpus, off, ids, probes, 8, 2000, 2000, 2000,
                    max(LENS), sims=sims)
    assert (idx < 2000).all()
    _check(queries[:3], corpus, off, ids, probes[:3], 5, 1, 1, 1, max(LENS), sims=sims)


@pytest.mark.parametrize("d", [64, 320])
def test_scan_other_dims(d, index):
    # D = 64: one line, no load group; D = 320: one group and one odd line
    off, ids = index
    rows = _rand_unit(N_IDX + 40, d, seed=20 + d)
    q = _rand_unit(QT + 1, d, seed=30 + d)
    probes = _probes(QT + 1, N_LISTS, 5, seed=d)
    _check(q, rows, off, ids, probes, 5, N_IDX + 40, N_IDX, N_IDX + 40, max(LENS))


def test_scan_three_segments_hand_index(corpus, queries, sims):
    # first segment 1000 rows, then the 2048-row quantum: lists of a random
    # permutation straddle both boundaries
    segs = [corpus[:1000], corpus[1000:3048].clone(), corpus[3048:5096].clone()]
    n_idx = 5000
    off, ids = _hand_index(n_idx, [0, 1, 999, 1000, 1048, 1952], seed=5)
    probes = _probes(QT + 1, 6, 3, seed=8)
    _check(queries[:QT + 1], segs, off, ids, probes, 8, 5096, n_idx, 5096, 1952,
           sims=sims[:, :5096])


@pytest.mark.parametrize("capacity,layout", [(1024, [2048, 2048, 2048]),
                                              (1000, [4000, 2048])])
def test_store_layouts_all_lists_probed(corpus, queries, sims, capacity, layout):
    # the three-segment store, and the layout EmbeddingStore grows into from a
    # first segment that stopped doubling at 4000 rows (no multiple of the
    # quantum); every list probed: the exact search's answer
    from kakveda_amd import ops
    from kakveda_amd.gfkb.engine import EmbeddingStore

    st = EmbeddingStore(D, device="cuda", capacity=capacity, segment_rows=2048)
    st.append(corpus)
    assert [int(s.shape[0]) for s in st._segments] == layout
    st.build_index(n_lists=16)
    s, i = st.search(queries, 5, nprobe=16, batched=True)
    rs, ri = ops.cosine_topk(queries, corpus, 5)
    torch.cuda.synchronize()
    assert torch.allclose(s, rs, atol=2e-2, rtol=1e-2)
    assert (i >= 0).all()
    assert (sims.gather(1, i) - s).abs().max().item() <= 1e-4
    _same_up_to_ties(i, ri, rs, sims)


def test_agrees_with_the_per_query_kernel(corpus, queries, index, sims):
    from kakveda_amd import ops

    off, ids = index
    B, k = 2 * QT + 1, 8
    probes = _probes(B, N_LISTS, 5, seed=21)
    valid_n = N_IDX + 13
    args = (queries[:B], corpus, off, ids, probes, k, valid_n, N_IDX, valid_n, max(LENS))
    bs, bi = ops.ivf_scan_topk(*args, batched=True)
    ps, pi = ops.ivf_scan_topk(*args, batched=False)
    torch.cuda.synchronize()
    assert torch.equal(bi < 0, pi < 0)
    live = bi >= 0
    # two fp32 summation orders of one unit-row inner product
    assert (bs[live] - ps[live]).abs().max().item() <= D * 2.0 ** -22
    _same_up_to_ties(bi, pi, ps, sims)


def test_grid_does_not_change_the_result(corpus, queries, index, sims):
    from kakveda_amd import ops

    off, ids = index
    B = QT + 1
    probes = _probes(B, N_LISTS, 5, seed=4)
    valid_n = N_IDX + 13
    a = ops.ivf_scan_topk(queries[:B], corpus, off, ids, probes, 8, valid_n, N_IDX,
                          valid_n, 3000, batched=True)
    # max_list_len unknown: one slice per tile, every block walks its whole list
    b = _check(queries[:B], corpus, off, ids, probes, 8, valid_n, N_IDX, valid_n, 0,
               sims=sims)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    # k past KMAX pads, as cosine_topk does
    s, i = ops.ivf_scan_topk(queries[:2], corpus, off, ids, probes[:2], 10, valid_n,
                             N_IDX, valid_n, batched=True)
    assert s.shape == (2, 10) and (i[:, 8:] == -1).all() and torch.isinf(s[:, 8:]).all()
    assert (i[1, :8] >= 0).all()


def test_batch_scanned_in_chunks(corpus, index):
    # the chunk size comes from the most slices a launch can get: 65 sources x
    # 64 slices (max_list_len 2^22 only sizes the grid) are 266,240 candidate
    # bytes per query, 1008 queries fit the 256 MiB cap, so 1100 queries are
    # scanned as 1008 + 92, each chunk with its own grouping and buffers
    off, ids = index
    B = 1100
    g = torch.Generator(device="cuda").manual_seed(17)
    pick = torch.randint(0, N_ROWS, (B,), generator=g, device=_dev())
    q = corpus[pick].float() + 0.03 * torch.randn(B, D, generator=g, device=_dev())
    q = (q / q.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
    probes = torch.full((B, 64), -1, dtype=torch.int32, device=_dev())
    probes[:, :5] = _probes(B, N_LISTS, 5, seed=23)
    valid_n = N_IDX + 13
    _check(q, corpus, off, ids, probes, 5, valid_n, N_IDX, valid_n, 1 << 22)


def test_more_tiles_than_one_launch_holds():
    # 20,000 queries that each probe all 64 lists: 1,300,000 live pairs make
    # 81,250 tiles, more than the 65,535 one launch holds, so the lists from
    # about the 52nd on are scanned by a second launch and every query's
    # answer needs both. Against the per-query kernel on every query, and
    # against the oracle on a few.
    from kakveda_amd import ops

    d, B, n_lists = 64, 20_000, 64
    lens = [(7 * i) % 19 for i in range(n_lists)]
    n_idx = sum(lens)
    off, ids = _hand_index(n_idx, lens, seed=7)
    rows = _rand_unit(n_idx + 8, d, seed=41)
    q = _rand_unit(B, d, seed=42)
    g = torch.Generator().manual_seed(43)
    probes = torch.rand(B, n_lists, generator=g).argsort(dim=1).to(torch.int32).to(_dev())
    valid_n = n_idx + 8
    _, _, _, n_tiles = ops._require_ext().ivf_group_probes(probes, n_lists)
    assert int(n_tiles[0]) == 65 * (B // QT) > 65535
    args = (q, rows, off, ids, probes, 5, valid_n, n_idx, valid_n, max(lens))
    bs, bi = ops.ivf_scan_topk(*args, batched=True)
    ps, pi = ops.ivf_scan_topk(*args, batched=False)
    torch.cuda.synchronize()
    assert (bi >= 0).all() and (pi >= 0).all()
    assert (bs - ps).abs().max().item() <= d * 2.0 ** -22
    # every row is a candidate of every query: the exact top-5
    sims = q.float() @ rows.float().t()
    es, ei = torch.topk(sims, 5, dim=1)
    assert (bs - es).abs().max().item() <= 1e-4
    assert (sims.gather(1, bi) - bs).abs().max().item() <= 1e-4
    differ = (bi.sort(dim=1).values != ei.sort(dim=1).values).any(dim=1).nonzero().flatten()
    _same_up_to_ties(bi[differ], ei[differ], es[differ], sims[differ])
    sel = torch.tensor([0, 15, 16, 9999, 19984, 19999], device=_dev())
    _check(q[sel], rows, off, ids, probes[sel], 5, valid_n, n_idx, valid_n, max(lens))


def test_grouping_on_the_device_is_the_cpu_grouping():
    from kakveda_amd import ops

    g = torch.Generator().manual_seed(3)
    probes = torch.randint(-2, 40, (100, 7), generator=g, dtype=torch.int32)
    cpu = ops.ivf_group_probes(probes, 37)
    ext = ops._require_ext().ivf_group_probes(probes.to(_dev()), 37)
    py = ops.ivf_group_probes(probes.to(_dev()), 37)
    torch.cuda.synchronize()
    for a, b, c in zip(cpu, ext, py):
        assert a.dtype == b.dtype == c.dtype
        assert torch.equal(a, b.cpu()) and torch.equal(a, c.cpu())


def test_refused_before_launch(corpus, queries, index):
    from kakveda_amd import ops

    off, ids = index
    probes = _probes(2, N_LISTS, 5, seed=1)
    q = queries[:2]

    def scan(*a):
        return ops.ivf_scan_topk(*a, batched=True)

    too_many = [corpus[:8]] + [corpus[8:16]] * 64
    with pytest.raises(RuntimeError, match="at most 64"):
        scan(q, too_many, off, ids, probes, 5, 16, 16, 16)
    uneven = [corpus[:1000], corpus[1000:3000], corpus[3000:4000]]
    with pytest.raises(RuntimeError, match="same row count"):
        scan(q, uneven, off, ids, probes, 5, 4000, 4000, 4000)
    with pytest.raises(RuntimeError, match="valid_n"):
        scan(q, corpus, off, ids, probes, 5, N_ROWS + 1, N_IDX, N_ROWS + 1)
    with pytest.raises(RuntimeError, match="tail"):
        scan(q, corpus, off, ids, probes, 5, N_IDX, N_IDX, N_IDX + 1)
    with pytest.raises(RuntimeError, match="k must be"):
        ops._require_ext().ivf_scan_topk_batched(
            q, [corpus], off, ids, probes, 9, N_IDX, N_IDX, N_IDX)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        scan(q[:, :32].contiguous(), corpus[:, :32].contiguous(), off, ids,
             probes, 5, N_IDX, N_IDX, N_IDX)


def test_default_goes_by_batch_size_and_row_width(corpus, index):
    from kakveda_amd import ops

    off, ids = index
    min_b = ops.IVF_BATCHED_MIN_B
    assert min_b is not None and min_b >= 64
    q = corpus[:min_b].contiguous()
    probes = _probes(min_b, N_LISTS, 5, seed=31)

    def scan(q, rows, probes, **kw):
        return ops.ivf_scan_topk(q, rows, off, ids, probes, 8, N_IDX, N_IDX, N_IDX,
                                 max(LENS), **kw)

    # from IVF_BATCHED_MIN_B queries on: the list-major kernel's very output
    a, b = scan(q, corpus, probes), scan(q, corpus, probes, batched=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # one query fewer: the per-query kernel's
    a = scan(q[:-1], corpus, probes[:-1])
    b = scan(q[:-1], corpus, probes[:-1], batched=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # rows too wide for the LDS query tile stay with the per-query kernel
    # unless the list-major one is forced, which refuses before launch
    wide = ops.IVF_BATCH_MAX_D + 64
    assert ops._require_ext().IVF_BATCH_MAX_D == ops.IVF_BATCH_MAX_D
    rows_w = _rand_unit(N_IDX, wide, seed=51)
    q_w = rows_w[:min_b].contiguous()
    a, b = scan(q_w, rows_w, probes), scan(q_w, rows_w, probes, batched=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(RuntimeError, match="too large for the LDS query tile"):
        scan(q_w, rows_w, probes, batched=True)
    # the widest row it takes
    rows_m = _rand_unit(N_IDX, ops.IVF_BATCH_MAX_D, seed=52)
    _check(rows_m[:QT + 1].contiguous(), rows_m, off, ids, probes[:QT + 1], 5, N_IDX,
           N_IDX, N_IDX, max(LENS))


def test_search_end_to_end():
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

    def routed(nprobe):
        return ops.ivf_search(q, [x], idx.centroids, idx.offsets, idx.ids, nprobe, 5,
                              n, idx.n_indexed, idx.max_list_len, batched=True)

    # every list probed: the exact search's answer up to ties
    s, i = routed(64)
    es, ei = ops.cosine_topk(q, x, 5)
    torch.cuda.synchronize()
    assert torch.allclose(s, es, atol=2e-2, rtol=1e-2)
    sims = q.float() @ x.float().t()
    assert (sims.gather(1, i) - s).abs().max().item() <= 1e-4
    _same_up_to_ties(i, ei, es, sims)

    # nprobe=8 against the reference on the CPU, same index
    s8, i8 = routed(8)
    torch.cuda.synchronize()
    rs, ri = ops.ivf_search_ref(
        q.cpu(), x.cpu(), idx.centroids.cpu(), idx.offsets.cpu(), idx.ids.cpu(), 8, 5, n, n
    )
    assert torch.equal(i8 < 0, (ri < 0).to(_dev()))
    assert torch.allclose(s8, rs.to(_dev()), atol=2e-2, rtol=1e-2)
    assert (sims.gather(1, i8.clamp_min(0)) - s8).abs().max().item() <= 1e-4
    same = (i8.cpu() == ri).float().mean().item()
    assert same >= 0.98, same  # ties and probe-boundary ulps only

    # the store passes the keyword through: the same kernel, the same answer
    s8b, i8b = st.search(q, 5, nprobe=8, batched=True)
    assert torch.equal(i8b, i8) and torch.equal(s8b, s8)
