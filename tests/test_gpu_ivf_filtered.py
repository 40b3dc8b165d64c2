"""GPU tests of the label-filtered routed scan: ivf_scan_topk_kernel<true>
(batched=False) and ivf_scan_grouped_kernel<true> (batched=True) behind
ops.ivf_scan_topk_filtered / ops.ivf_search_filtered and
EmbeddingStore.search(..., want=..., nprobe=..., route_filtered=True).

Oracle: ops.ivf_scan_topk_filtered_ref (plain torch, fp32) on the same bf16
inputs, index arrays and labels. The assertions are those of
test_gpu_ivf_batched.py - pads exactly where the oracle pads, as (-inf, -1);
every returned id a candidate of its query, below valid_n, unique in its row
and within 1e-4 of the fp32 inner product; the id set equal to the oracle's
up to ties within 1e-4 - plus: every returned id is eligible for its query
(want < 0 or label == want).

Shapes as in test_gpu_ivf_batched.py, for the same reasons: D = 768, 6,000
rows, hand-built lists around the 8-row wave step of the per-query kernel,
the 16-row MFMA step and 64-row block step of the list-major one and its
1024-row slice; batch sizes around the 16-query tile. Every hand-built id
table is validated as an IvfIndex on the CPU before it reaches a kernel.
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
L17, L33, L65, L257 = 7, 10, 13, 16
QT = 16
N_QUERIES = 100
# (batched, B): both kernels, batch sizes around one wave / one query tile
KERNELS = [(False, 1), (False, 3), (False, 9),
           (True, 1), (True, QT - 1), (True, QT), (True, QT + 1),
           (True, 2 * QT + 1), (True, 100)]
KERNEL_IDS = [f"{'list' if b else 'query'}-B{n}" for b, n in KERNELS]
KS = [1, 5, 8]


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


def _spread_labels(n):
    """Labels r % 3, every 11th row unlabelled (-1)."""
    r = torch.arange(n, device=_dev())
    lab = (r % 3).to(torch.int32)
    lab[r % 11 == 0] = -1
    return lab


def _cycle_wants(B):
    """-1, 0, 1, 2, -1, ... : filtered and unfiltered queries in one batch."""
    return ((torch.arange(B, device=_dev()) % 4) - 1).to(torch.int32)


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


@pytest.fixture(scope="module")
def labels():
    """r % 3 with some -1, one per corpus row; never modified."""
    return _spread_labels(N_ROWS)


def _cat(x):
    return x if isinstance(x, torch.Tensor) else torch.cat(list(x), 0)


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


def _eligible(labels, want):
    lab = _cat(labels).long()
    w = want.long()
    return (w[:, None] < 0) | (lab[None, :] == w[:, None])


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


def _check(q, segments, labels, want, off, ids, probes, k, valid_n, tail_lo, tail_hi,
           batched, max_list_len=0, sims=None):
    from kakveda_amd import ops

    B = q.shape[0]
    scores, idx = ops.ivf_scan_topk_filtered(
        q, segments, labels, want, off, ids, probes, k, valid_n, tail_lo, tail_hi,
        max_list_len, batched=batched,
    )
    torch.cuda.synchronize()
    ref_s, ref_i = ops.ivf_scan_topk_filtered_ref(
        q, segments, labels, want, off, ids, probes, k, valid_n, tail_lo, tail_hi
    )
    rows = _cat(segments)
    if sims is None:
        sims = q.float() @ rows.float().t()
    sims = sims[:B]
    elig = _eligible(labels, want)
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
    # every returned id is a candidate of its query, eligible for it, once,
    # and achieves its score
    safe = idx.clamp_min(0)
    assert cand.gather(1, safe)[hit].all()
    assert elig.gather(1, safe)[hit].all()
    assert (idx[hit] < valid_n).all()
    if hit.any():
        assert (sims.gather(1, safe)[hit] - scores[hit]).abs().max().item() <= 1e-4
    for b in range(B):
        live = idx[b][idx[b] >= 0].tolist()
        assert len(set(live)) == len(live)
    _same_up_to_ties(idx, ref_i, ref_s, sims)
    return scores, idx


# 1. three labels spread r % 3, some rows -1; wants cycle -1, 0, 1, 2
@pytest.mark.parametrize("tail", [0, 1, 13, 500])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("batched,B", KERNELS, ids=KERNEL_IDS)
def test_spread_labels_mixed_wants(corpus, queries, index, sims, labels, batched, B, k, tail):
    off, ids = index
    probes = _probes(B, N_LISTS, 5, seed=B * 10 + k)
    valid_n = N_IDX + tail
    scores, idx = _check(
        queries[:B], corpus, labels, _cycle_wants(B), off, ids, probes, k, valid_n,
        N_IDX, valid_n, batched, max(LENS), sims=sims,
    )
    if tail == 0:  # query 0 probes one empty list and pads: nothing to find
        assert (idx[0] == -1).all() and torch.isinf(scores[0]).all()


# 2. a rare label on exactly three rows
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("batched,B", KERNELS, ids=KERNEL_IDS)
def test_rare_label_on_three_rows(corpus, queries, index, sims, labels, batched, B, k):
    off, ids = index
    o = off.tolist()
    in_big = int(ids[o[BIG] + 2990])    # last 32 positions: the third slice
    in_tail = N_IDX + 5
    unprobed = int(ids[o[L257] + 100])  # a list the queries do not probe
    lab = labels.clone()
    lab[torch.tensor([in_big, in_tail, unprobed], device=_dev())] = 7
    assert int((lab == 7).sum()) == 3
    probes = torch.tensor([[BIG, ONE, 3, 4, 5]] * B, dtype=torch.int32, device=_dev())
    want = torch.full((B,), 7, dtype=torch.int32, device=_dev())
    valid_n = N_IDX + 13
    _, idx = _check(queries[:B], corpus, lab, want, off, ids, probes, k, valid_n, N_IDX,
                    valid_n, batched, max(LENS), sims=sims)
    for b in range(B):
        live = [i for i in idx[b].tolist() if i >= 0]
        assert len(live) == min(k, 2) and set(live) <= {in_big, in_tail}
        assert (idx[b, len(live):] == -1).all()


# 3. the wave-skip edge: one eligible row at a position around the 16th / 64th
EDGE = [(L17, 15), (L17, 16), (L33, 15), (L33, 16), (L33, 17),
        (L65, 15), (L65, 16), (L65, 17), (L65, 63), (L65, 64)]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("batched,B", KERNELS, ids=KERNEL_IDS)
def test_single_eligible_row_at_the_step_edge(corpus, queries, index, sims, labels,
                                              batched, B, k):
    off, ids = index
    o = off.tolist()
    lab = labels.clone()
    rows = [int(ids[o[l] + p]) for l, p in EDGE]
    for e, r in enumerate(rows):
        lab[r] = 100 + e  # the only row of its list (and of the store) so labelled
    for start in range(0, len(EDGE), B):
        case = [(start + b) % len(EDGE) for b in range(B)]
        probes = torch.tensor([[EDGE[c][0]] for c in case], dtype=torch.int32, device=_dev())
        want = torch.tensor([100 + c for c in case], dtype=torch.int32, device=_dev())
        _, idx = _check(queries[:B], corpus, lab, want, off, ids, probes, k, N_IDX, N_IDX,
                        N_IDX, batched, max(LENS), sims=sims)
        for b, c in enumerate(case):
            assert idx[b, 0] == rows[c] and (idx[b, 1:] == -1).all()


# 4. a want no row carries; a probed empty list and an all -1 probe row
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("batched,B", KERNELS, ids=KERNEL_IDS)
def test_unknown_want_pads_fully(corpus, queries, index, sims, labels, batched, B, k):
    off, ids = index
    probes = _probes(B, N_LISTS, 5, seed=12 + B)
    want = _cycle_wants(B)
    want[1::2] = 55  # no row carries it
    if B > 5:
        probes[3] = -1        # probes nothing at all
        probes[5] = -1
        probes[5, 4] = EMPTY  # probes the empty list only
    s, i = _check(queries[:B], corpus, labels, want, off, ids, probes, k, N_IDX + 13,
                  N_IDX, N_IDX + 13, batched, max(LENS), sims=sims)
    assert (i[1::2] == -1).all() and (s[1::2] == float("-inf")).all()
    # the same with no tail: an empty candidate set pads as it does today
    s, i = _check(queries[:B], corpus, labels, want, off, ids, probes, k, N_IDX, N_IDX,
                  N_IDX, batched, max(LENS), sims=sims)
    empty = [0] + ([3, 5] if B > 5 else [])
    for b in empty:
        assert (i[b] == -1).all() and (s[b] == float("-inf")).all()


# 5. want = -1 for every query: the unfiltered op's very output
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("batched,B", KERNELS, ids=KERNEL_IDS)
def test_all_unfiltered_equals_the_unfiltered_op(corpus, queries, index, labels,
                                                 batched, B, k):
    from kakveda_amd import ops

    off, ids = index
    probes = _probes(B, N_LISTS, 5, seed=40 + B)
    want = torch.full((B,), -1, dtype=torch.int32, device=_dev())
    valid_n = N_IDX + 13
    fs, fi = ops.ivf_scan_topk_filtered(
        queries[:B], corpus, labels, want, off, ids, probes, k, valid_n, N_IDX, valid_n,
        max(LENS), batched=batched,
    )
    us, ui = ops.ivf_scan_topk(
        queries[:B], corpus, off, ids, probes, k, valid_n, N_IDX, valid_n, max(LENS),
        batched=batched,
    )
    torch.cuda.synchronize()
    assert torch.equal(fs, us) and torch.equal(fi, ui)


# 6. three segments, one label tensor per segment
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("batched,B", KERNELS, ids=KERNEL_IDS)
def test_three_segments_label_per_segment(corpus, queries, sims, labels, batched, B, k):
    # first segment 1000 rows, then the 2048-row quantum: lists and labels of
    # a random permutation straddle both boundaries
    segs = [corpus[:1000], corpus[1000:3048].clone(), corpus[3048:5096].clone()]
    labs = [labels[:1000].clone(), labels[1000:3048].clone(), labels[3048:5096].clone()]
    n_idx = 5000
    off, ids = _hand_index(n_idx, [0, 1, 999, 1000, 1048, 1952], seed=5)
    probes = _probes(B, 6, 3, seed=8 + B)
    _check(queries[:B], segs, labs, _cycle_wants(B), off, ids, probes, k, 5096, n_idx,
           5096, batched, 1952, sims=sims[:, :5096])


# 7. a valid_n snapshot below most listed ids
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("batched,B", KERNELS, ids=KERNEL_IDS)
def test_snapshot_valid_n_hides_listed_rows(corpus, queries, index, sims, labels,
                                            batched, B, k):
    off, ids = index
    probes = _probes(B, N_LISTS, 5, seed=6 + B)
    _, idx = _check(queries[:B], corpus, labels, _cycle_wants(B), off, ids, probes, k,
                    2000, 2000, 2000, batched, max(LENS), sims=sims)
    assert (idx < 2000).all()


# 8. the two kernels agree on a mixed batch of 33
def test_the_two_kernels_agree(corpus, queries, index, sims, labels):
    from kakveda_amd import ops

    off, ids = index
    B, k = 2 * QT + 1, 8
    probes = _probes(B, N_LISTS, 5, seed=21)
    valid_n = N_IDX + 13
    args = (queries[:B], corpus, labels, _cycle_wants(B), off, ids, probes, k, valid_n,
            N_IDX, valid_n, max(LENS))
    bs, bi = ops.ivf_scan_topk_filtered(*args, batched=True)
    ps, pi = ops.ivf_scan_topk_filtered(*args, batched=False)
    torch.cuda.synchronize()
    assert torch.equal(bi < 0, pi < 0)
    live = bi >= 0
    # two fp32 summation orders of one unit-row inner product
    assert (bs[live] - ps[live]).abs().max().item() <= D * 2.0 ** -22
    _same_up_to_ties(bi, pi, ps, sims)


# 9. D = 64 (one line, no load group) and D = 320 (one group and one odd line)
@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("d", [64, 320])
def test_other_dims(d, index, batched):
    off, ids = index
    rows = _rand_unit(N_IDX + 40, d, seed=20 + d)
    q = _rand_unit(QT + 1, d, seed=30 + d)
    probes = _probes(QT + 1, N_LISTS, 5, seed=d)
    _check(q, rows, _spread_labels(N_IDX + 40), _cycle_wants(QT + 1), off, ids, probes, 5,
           N_IDX + 40, N_IDX, N_IDX + 40, batched, max(LENS))


# 10. refused before launch
@pytest.mark.parametrize("name", ["ivf_scan_topk_filtered", "ivf_scan_topk_batched_filtered"])
def test_refused_before_launch(corpus, queries, index, labels, name):
    from kakveda_amd import ops

    scan = getattr(ops._require_ext(), name)
    off, ids = index
    probes = _probes(2, N_LISTS, 5, seed=1)
    q = queries[:2]
    want = torch.tensor([0, -1], dtype=torch.int32, device=_dev())
    tail = (5, N_IDX, N_IDX, N_IDX)
    segs = [corpus[:1000], corpus[1000:3048].clone(), corpus[3048:5096].clone()]
    labs = [labels[:1000].clone(), labels[1000:3048].clone(), labels[3048:5096].clone()]
    # the well-formed call goes through
    scan(q, segs, labs, want, off, ids, probes, 5, 5096, 5000, 5096)
    with pytest.raises(RuntimeError, match="one tensor per segment"):
        scan(q, segs, labs[:2], want, off, ids, probes, 5, 5096, 5000, 5096)
    with pytest.raises(RuntimeError, match="exactly its"):
        scan(q, [corpus], [labels[: N_ROWS - 1].clone()], want, off, ids, probes, *tail)
    with pytest.raises(RuntimeError, match="labels must be contiguous 1-D i32"):
        scan(q, [corpus], [labels.long()], want, off, ids, probes, *tail)
    with pytest.raises(RuntimeError, match="labels must be contiguous 1-D i32"):
        scan(q, [corpus], [labels.cpu()], want, off, ids, probes, *tail)
    with pytest.raises(RuntimeError, match="one entry per query"):
        scan(q, [corpus], [labels], want[:1].clone(), off, ids, probes, *tail)
    with pytest.raises(RuntimeError, match="want must be contiguous 1-D i32"):
        scan(q, [corpus], [labels], want.long(), off, ids, probes, *tail)
    # the search entry points refuse the same before they route
    search = getattr(ops._require_ext(), name.replace("scan_topk", "search"))
    cen = _rand_unit(N_LISTS, D, seed=77)
    with pytest.raises(RuntimeError, match="exactly its"):
        search(q, [corpus], [labels[: N_ROWS - 1].clone()], want, cen, off, ids, 2, 5,
               N_IDX, N_IDX)
    with pytest.raises(RuntimeError, match="one entry per query"):
        search(q, [corpus], [labels], want[:1].clone(), cen, off, ids, 2, 5, N_IDX, N_IDX)
    torch.cuda.synchronize()


# 11. the store end to end at 70,000 clustered rows
@pytest.mark.parametrize("batched", [False, True])
def test_store_end_to_end(batched):
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
    lab = (torch.arange(n, device=_dev()) % 7).to(torch.int32)
    want = (torch.arange(32, device=_dev()) % 8 - 1).to(torch.int32)  # -1, 0 .. 6

    st = EmbeddingStore(D, device="cuda")
    st.adopt(x, lab)
    assert st.label_rows(0) == 10_000 and st.label_rows(6) == 10_000
    st.build_index(n_lists=64)
    elig = _eligible(lab, want)
    sims = q.float() @ x.float().t()

    # every list probed: the exact filtered search's answer up to ties
    s, i = st.search(q, 5, want=want, nprobe=64, route_filtered=True, batched=batched)
    es, ei = ops.cosine_topk_filtered(q, x, lab, want, 5)
    torch.cuda.synchronize()
    assert (i >= 0).all() and (ei >= 0).all()
    assert torch.allclose(s, es, atol=2e-2, rtol=1e-2)
    assert elig.gather(1, i).all()
    assert (sims.gather(1, i) - s).abs().max().item() <= 1e-4
    _same_up_to_ties(i, ei, es, sims)

    # nprobe=8 with the exact fill: no short row for any label
    s8, i8 = st.search(q, 5, want=want, nprobe=8, route_filtered=True, batched=batched)
    torch.cuda.synchronize()
    assert (i8 >= 0).all()
    assert elig.gather(1, i8).all()
    assert (sims.gather(1, i8) - s8).abs().max().item() <= 1e-4
