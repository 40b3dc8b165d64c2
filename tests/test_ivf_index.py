"""Routed (IVF) search on CPU: index build, the plain-torch references of
ops.ivf_scan_topk / ops.ivf_search, and EmbeddingStore.search(nprobe=...)."""

import logging

import pytest
import torch

from kakveda_amd import ops
from kakveda_amd.gfkb.engine import EmbeddingStore
from kakveda_amd.gfkb.ivf import IvfIndex, default_n_lists

N, D, CENTRES = 4096, 64, 16


def _unit(x):
    return torch.nn.functional.normalize(x, dim=1)


def _mixture(n=N, d=D, centres=CENTRES, seed=0, spread=0.1):
    g = torch.Generator().manual_seed(seed)
    cen = _unit(torch.randn(centres, d, generator=g))
    pick = torch.randint(0, centres, (n,), generator=g)
    return _unit(cen[pick] + spread * torch.randn(n, d, generator=g))


@pytest.fixture(scope="module")
def corpus():
    return _mixture()


@pytest.fixture(scope="module")
def queries(corpus):
    g = torch.Generator().manual_seed(1)
    pick = torch.randint(0, N, (64,), generator=g)
    return _unit(corpus[pick] + 0.05 * torch.randn(64, D, generator=g))


def _store(rows, **kw):
    st = EmbeddingStore(D, **kw)
    st.append(rows)
    return st


@pytest.fixture()
def store(corpus):
    st = _store(corpus)
    st.build_index(n_lists=16)
    return st


def test_default_n_lists():
    assert default_n_lists(1) == 16
    assert default_n_lists(1_000_000) == 1000
    assert default_n_lists(10_000_000) % 8 == 0
    assert abs(default_n_lists(10_000_000) - 3162) <= 4
    assert default_n_lists(10**12) == 16384


def test_build_validates_and_partitions(store):
    idx = store.index
    assert isinstance(idx, IvfIndex)
    idx.validate()
    assert idx.n_lists == 16 and idx.n_indexed == N
    assert idx.centroids.dtype == store.dtype and idx.centroids.shape == (16, D)
    assert idx.ids.dtype == torch.int32 and idx.offsets.shape == (17,)
    # every row in exactly one list
    assert torch.equal(idx.ids.long().sort().values, torch.arange(N))
    lens = idx.offsets[1:] - idx.offsets[:-1]
    assert int(lens.sum()) == N and int(lens.max()) == idx.max_list_len
    assert torch.allclose(idx.centroids.float().norm(dim=1), torch.ones(16), atol=1e-4)
    for key in ("list_min", "list_median", "list_max", "empty_lists", "build_seconds"):
        assert key in idx.stats
    # rows of a list are nearest to that list's centroid
    assign = (store.data[:N] @ idx.centroids.t()).argmax(dim=1)
    for l in (0, 7, 15):
        rows = idx.ids[int(idx.offsets[l]) : int(idx.offsets[l + 1])].long()
        assert bool((assign[rows] == l).all())


def test_validate_rejects_bad_tables(store):
    idx = store.index
    dup = idx.ids.clone()
    dup[0] = dup[1]
    with pytest.raises(ValueError):
        IvfIndex(idx.centroids, idx.offsets, dup, N, 16, idx.max_list_len).validate()
    off = idx.offsets.clone()
    off[3], off[4] = idx.offsets[4].item() + 1, idx.offsets[3].item()
    with pytest.raises(ValueError):
        IvfIndex(idx.centroids, off, idx.ids, N, 16, idx.max_list_len).validate()
    off = idx.offsets.clone()
    off[-1] = N - 1
    with pytest.raises(ValueError):
        IvfIndex(idx.centroids, off, idx.ids, N, 16, idx.max_list_len).validate()


def test_all_lists_is_exact(store, corpus, queries):
    ref_s, ref_i = ops.cosine_topk_ref(queries, corpus, 5)
    s, i = store.search(queries, 5, nprobe=16)
    assert torch.equal(i, ref_i)
    assert torch.allclose(s, ref_s, atol=1e-5)
    # clamped above n_lists
    s2, i2 = store.search(queries, 5, nprobe=1000)
    assert torch.equal(i2, ref_i)


def test_recall_at_nprobe_4(store, corpus, queries):
    _, ref_i = ops.cosine_topk_ref(queries, corpus, 5)
    _, i = store.search(queries, 5, nprobe=4)
    hits = sum(len(set(a) & set(b)) for a, b in zip(i.tolist(), ref_i.tolist()))
    recall = hits / ref_i.numel()
    print(f"recall@5 at nprobe=4: {recall:.3f}")
    assert recall >= 0.95


def test_unrouted_search_unchanged_by_index(store, corpus, queries):
    ref_s, ref_i = ops.cosine_topk_ref(queries, corpus, 5)
    for kw in ({}, {"nprobe": None}, {"nprobe": 0}):
        s, i = store.search(queries, 5, **kw)
        assert torch.equal(i, ref_i) and torch.equal(s, ref_s)


def test_appended_row_found_before_rebuild(store):
    g = torch.Generator().manual_seed(5)
    new = _unit(torch.randn(1, D, generator=g))  # far from every centre
    row = store.append(new)
    assert row == N and store.index.n_indexed == N
    s, i = store.search(new, 3, nprobe=1)
    assert int(i[0, 0]) == N and float(s[0, 0]) > 0.999


def test_stale_fraction_and_single_warning(corpus, caplog):
    st = _store(corpus[:1000])
    assert st.stale_fraction == 0.0  # no index
    st.build_index(n_lists=16)
    assert st.stale_fraction == 0.0
    st.append(corpus[1000:1100])
    assert st.stale_fraction == pytest.approx(0.1)
    q = corpus[:2]
    with caplog.at_level(logging.WARNING, logger="kakveda_amd.gfkb.engine"):
        st.search(q, 5, nprobe=4)
        assert not [r for r in caplog.records if "stale" in r.getMessage()]
        st.append(corpus[1100:1101])  # past 10%
        st.search(q, 5, nprobe=4)
        st.search(q, 5, nprobe=4)
    assert len([r for r in caplog.records if "stale" in r.getMessage()]) == 1
    st.build_index(n_lists=16)
    assert st.stale_fraction == 0.0 and st.index.n_indexed == 1101


def test_nprobe_without_index_raises(corpus):
    st = _store(corpus[:100])
    assert st.index is None
    with pytest.raises(ValueError, match="index"):
        st.search(corpus[:1], 5, nprobe=4)
    with pytest.raises(ValueError):
        st.search(corpus[:1], 5, nprobe=-1)


def test_filtered_request_takes_exact_filtered_path(corpus, queries, monkeypatch):
    st = EmbeddingStore(D)
    labels = torch.arange(N) % 3
    st.append(corpus, labels)
    st.build_index(n_lists=16)

    def boom(*a, **kw):
        raise AssertionError("a filtered query must not be routed")

    monkeypatch.setattr(ops, "ivf_search", boom)
    want = torch.full((queries.shape[0],), 1, dtype=torch.int32)
    s, i = st.search(queries, 5, want=want, nprobe=1)
    ref_s, ref_i = ops.cosine_topk_filtered_ref(queries, corpus, labels, want, 5)
    assert torch.equal(i, ref_i) and torch.allclose(s, ref_s)


def test_adopt_drops_the_index(store, corpus):
    store.adopt(corpus[:10].clone())
    assert store.index is None


def test_segmented_store_matches_exact(corpus, queries):
    st = _store(corpus, capacity=1000, segment_rows=1000)
    assert st.n_segments > 2
    st.build_index(n_lists=16)
    ref_s, ref_i = ops.cosine_topk_ref(queries, corpus, 5)
    s, i = st.search(queries, 5, nprobe=16)
    assert torch.equal(i, ref_i) and torch.allclose(s, ref_s, atol=1e-5)


# -- hand-built lists through the reference ops ------------------------------


def _hand_index(n, lens, seed=3):
    """ids: a seeded permutation of [0, n) cut into lists of ``lens``."""
    assert sum(lens) == n
    g = torch.Generator().manual_seed(seed)
    ids = torch.randperm(n, generator=g).to(torch.int32)
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens), 0)
    return off, ids


def test_scan_empty_short_and_padded(corpus):
    n = 20
    rows = corpus[:n]
    off, ids = _hand_index(n, [0, 3, 17])
    q = corpus[100:103]
    probes = torch.tensor([[0, -1], [1, 0], [1, 2]], dtype=torch.int32)
    s, i = ops.ivf_scan_topk(q, rows, off, ids, probes, 5, n, n, n)
    assert s.shape == (3, 5) and i.shape == (3, 5)
    assert s.dtype == torch.float32 and i.dtype == torch.int64
    # an empty list and a -1 pad: nothing but pads
    assert bool((i[0] == -1).all()) and bool(torch.isinf(s[0]).all())
    # a list shorter than k: its 3 rows, then pads
    assert sorted(i[1, :3].tolist()) == sorted(ids[:3].tolist())
    assert i[1, 3:].tolist() == [-1, -1] and bool(torch.isinf(s[1, 3:]).all())
    # both non-empty lists: every row is a candidate
    ref_s, ref_i = ops.cosine_topk_ref(q[2:], rows, 5)
    assert torch.equal(i[2:], ref_i) and torch.allclose(s[2:], ref_s, atol=1e-6)


def test_scan_tail_and_valid_n(corpus):
    n = 40
    rows = corpus[:n]
    off, ids = _hand_index(30, [10, 20])
    q = corpus[200:202]
    probes = torch.tensor([[0], [1]], dtype=torch.int32)
    # tail [30, 40) is scanned for both queries
    s, i = ops.ivf_scan_topk(q, rows, off, ids, probes, 8, n, 30, n)
    for b, l in enumerate((0, 1)):
        cand = set(ids[int(off[l]) : int(off[l + 1])].tolist()) | set(range(30, 40))
        assert set(i[b].tolist()) <= cand
        sims = rows[sorted(cand)] @ q[b]
        assert torch.allclose(s[b], sims.topk(8).values, atol=1e-6)
    # a snapshot valid_n below some listed ids: those rows never appear
    s, i = ops.ivf_scan_topk(q, rows, off, ids, probes, 8, 12, 12, 12)
    assert bool(((i < 12)).all())
    for b, l in enumerate((0, 1)):
        live = [r for r in ids[int(off[l]) : int(off[l + 1])].tolist() if r < 12]
        got = [x for x in i[b].tolist() if x >= 0]
        assert set(got) <= set(live) and len(set(got)) == len(got)
        assert len(got) == min(8, len(live))


def test_search_ref_candidate_set_shorter_than_k(corpus):
    rows = corpus[:6]
    st = _store(rows)
    st.build_index(n_lists=6, iters=2)
    s, i = st.search(corpus[:2], 5, nprobe=1)
    assert s.shape == (2, 5)
    pads = i < 0
    assert bool(torch.isinf(s[pads]).all()) and bool((s[~pads] > -1).all())
    # each row is found in its own list
    assert i[:, 0].tolist() == [0, 1]
