"""CPU checks of the grouping step of the list-major routed scan
(ops.ivf_group_probes) and of the ``batched`` keyword on CPU tensors.

The grouping sorts the B x (nprobe + 1) (query, probe) pairs by list and
cuts every list's group into tiles of at most IVF_BATCH_QTILE pairs. The
kernel trusts four things, asserted here for every case: each valid (b, y)
pair is in exactly one tile, no tile is larger than QTILE or mixes lists, the
tile count stays within the plan's bound (the launch is sized by it), and a
discarded pair is in no tile.
"""

import pytest
import torch

from kakveda_amd import ops

QT = ops.IVF_BATCH_QTILE
N_LISTS = 12
NPROBE = 5
EVERYONE = 3  # a list every query probes
NOBODY = 7    # a list nobody probes


def _probes(B, seed):
    """Distinct lists per query, never NOBODY, always EVERYONE in column 0;
    -1 pads in the odd rows, out-of-range ids (n_lists, n_lists + 5, -7) in
    every third row."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.tensor([l for l in range(N_LISTS) if l not in (EVERYONE, NOBODY)])
    rows = []
    for _ in range(B):
        pick = pool[torch.randperm(pool.numel(), generator=g)[: NPROBE - 1]]
        rows.append(torch.cat([torch.tensor([EVERYONE]), pick]))
    p = torch.stack(rows).to(torch.int32)
    p[1::2, 2] = -1
    p[2::3, 4] = N_LISTS
    p[2::3, 3] = N_LISTS + 5
    p[::3, 1] = -7
    return p


def _check_grouping(probes, n_lists):
    B, nprobe = probes.shape
    S = nprobe + 1
    P = B * S
    pair_query, pair_slot, tiles, n_tiles = ops.ivf_group_probes(probes, n_lists)
    T = ops.ivf_batch_tile_bound(P, n_lists)
    assert pair_query.shape == (P,) and pair_slot.shape == (P,)
    assert pair_query.dtype == torch.int32 and pair_slot.dtype == torch.int32
    assert tiles.shape == (3, T) and tiles.dtype == torch.int32
    assert n_tiles.shape == (1,) and n_tiles.dtype == torch.int32
    nt = int(n_tiles[0])
    assert 0 <= nt <= T  # the launch is sized by the bound

    # the pair arrays are a permutation of all (b, y)
    flat = (pair_query.long() * S + pair_slot.long()).tolist()
    assert sorted(flat) == list(range(P))

    def list_of(b, y):  # the list pair (b, y) scans; None: discarded
        if y == nprobe:
            return n_lists
        l = int(probes[b, y])
        return l if 0 <= l < n_lists else None

    seen = {}
    per_list_tiles = {}
    for t in range(nt):
        l, first, cnt = (int(v) for v in tiles[:, t])
        assert 1 <= cnt <= QT
        assert 0 <= l <= n_lists
        assert 0 <= first and first + cnt <= P
        per_list_tiles.setdefault(l, []).append(cnt)
        for i in range(first, first + cnt):
            b, y = int(pair_query[i]), int(pair_slot[i])
            assert list_of(b, y) == l, (t, i, b, y)  # no tile mixes lists
            assert (b, y) not in seen  # in exactly one tile
            seen[(b, y)] = t
    assert (tiles[2, nt:] == 0).all()  # tiles past the count are empty
    valid = {(b, y) for b in range(B) for y in range(S) if list_of(b, y) is not None}
    assert set(seen) == valid  # every valid pair, no discarded one
    # a list's group is cut into full tiles and at most one short one
    for l, cnts in per_list_tiles.items():
        assert sum(1 for c in cnts if c < QT) <= 1
    return per_list_tiles


@pytest.mark.parametrize("B", [1, QT - 1, QT, QT + 1, 100])
def test_grouping_invariants(B):
    probes = _probes(B, seed=B)
    per_list = _check_grouping(probes, N_LISTS)
    assert NOBODY not in per_list
    # the list everyone probes (column 0 never pads) and the tail: B pairs
    # each, ceil(B / QTILE) tiles
    want = [QT] * (B // QT) + ([B % QT] if B % QT else [])
    assert sorted(per_list[EVERYONE]) == sorted(want)
    assert sorted(per_list[N_LISTS]) == sorted(want)


def test_grouping_adversarial_shapes():
    # all pairs in one list (L = 1), one pair per list, P < QTILE, every
    # probe discarded, nprobe = 0 (tail only)
    _check_grouping(torch.zeros(100, 1, dtype=torch.int32), 1)
    _check_grouping(torch.arange(40, dtype=torch.int32).reshape(40, 1), 40)
    _check_grouping(torch.tensor([[2, 0]], dtype=torch.int32), 3)
    only_tail = _check_grouping(torch.full((20, 3), -1, dtype=torch.int32), 5)
    assert list(only_tail) == [5]
    _check_grouping(torch.zeros(5, 0, dtype=torch.int32), 4)
    _check_grouping(torch.tensor([[0, 1], [1, 0]], dtype=torch.int64), 2)


def test_grouping_is_deterministic():
    probes = _probes(33, seed=1)
    a = ops.ivf_group_probes(probes, N_LISTS)
    b = ops.ivf_group_probes(probes.clone(), N_LISTS)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_batched_keyword_on_cpu_is_the_reference():
    g = torch.Generator().manual_seed(4)
    lens = [0, 1, 7, 16, 17, 40, 3, 0, 9, 5, 12, 30]
    n_idx = sum(lens)
    rows = torch.randn(n_idx + 20, 64, generator=g)
    rows = rows / rows.norm(dim=-1, keepdim=True)
    q = torch.randn(QT + 3, 64, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    ids = torch.randperm(n_idx, generator=g).to(torch.int32)
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens), 0)
    probes = _probes(QT + 3, seed=2)
    args = (q, rows, off, ids, probes, 5, n_idx + 20, n_idx, n_idx + 20)
    ref_s, ref_i = ops.ivf_scan_topk_ref(*args)
    for batched in (True, False, None):
        s, i = ops.ivf_scan_topk(*args, max_list_len=40, batched=batched)
        assert torch.equal(s, ref_s) and torch.equal(i, ref_i)
    cen = torch.randn(len(lens), 64, generator=g)
    rs, ri = ops.ivf_search_ref(q, rows, cen, off, ids, 4, 5, n_idx + 20, n_idx)
    for batched in (True, False, None):
        s, i = ops.ivf_search(q, rows, cen, off, ids, 4, 5, n_idx + 20, n_idx,
                              batched=batched)
        assert torch.equal(s, rs) and torch.equal(i, ri)


def test_store_search_takes_batched_on_cpu():
    from kakveda_amd.gfkb.engine import EmbeddingStore

    g = torch.Generator().manual_seed(6)
    x = torch.randn(600, 64, generator=g)
    x = x / x.norm(dim=-1, keepdim=True)
    st = EmbeddingStore(64, device="cpu")
    st.append(x)
    st.build_index(n_lists=8)
    a = st.search(x[:20], 3, nprobe=8, batched=True)
    b = st.search(x[:20], 3, nprobe=8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
