"""Exact GPU tests of the kernels around the search: kmeans_update_kernel,
kmeans_assign_kernel (and the cosine_topk k = 1 route of
kmeans_assign_scored), embedding_bag_kernel and l2normalize_rows.

The cases and oracles are those of tests/aux_cases.py, proven on the CPU by
tests/test_aux_cases_ref.py. Inputs are small integers (or multiples of
1/8), so every product and every partial sum is exact in fp32 in any order:
the k-means and embedding-bag kernels must be bit-equal to the int64 /
float64 oracle (torch.equal, no tolerance). l2normalize_ faces the derived
bound of aux_cases.norm_bound. Shapes are the smallest that reach each code
path of the kernels; the comments in aux_cases.py name the paths.
"""

import pytest
import torch

import aux_cases as ac
from kakveda_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"

ASSIGN_DIMS = (64, 128, 192, 256, 320, 768, 1152)
ASSIGN_CS = (1, 16, 17, 63)
ASSIGN_NS = (1, 31, 255, 256, 257)
GRID_STRIDE_N = 2048 * 256 + 300  # one block more than the grid-stride loop's first sweep
ROUTE_CS = (65, 200, 513)
NORM_DIMS = (8, 64, 520, 768, 1536)


def _sync(*t):
    torch.cuda.synchronize()
    return t[0] if len(t) == 1 else t


# -- kmeans_update -------------------------------------------------------------

@pytest.mark.parametrize("C,D,N,bad,empty", ac.UPDATE_CASES)
def test_kmeans_update_exact(C, D, N, bad, empty):
    case = ac.update_case(C, D, N, bad, empty)
    sums, counts = _sync(*ops.kmeans_update(case.points.to(DEV), case.assign.to(DEV), C))
    ac.check_update(case, sums, counts)


def test_kmeans_update_twice_gives_the_same_sums():
    """The outputs are fresh zeroed tensors per call: nothing accumulates
    across calls, and the LDS attribute latch of the first call holds."""
    case = ac.update_case(129, 64, 150001)
    p, a = case.points.to(DEV), case.assign.to(DEV)
    ops.kmeans_update(p, a, case.C)
    sums, counts = _sync(*ops.kmeans_update(p, a, case.C))
    ac.check_update(case, sums, counts)


# -- kmeans_assign, C <= 64: the dedicated kernel --------------------------------

def _gpu_assign(case):
    return _sync(*ops.kmeans_assign_scored(case.points.to(DEV), case.centroids.to(DEV)))


@pytest.mark.parametrize("D", ASSIGN_DIMS)
def test_kmeans_assign_exact_dims(D):
    """D / 64 = 1, 2, 3, 4, 5, 12, 18 windows: the clamped prefetch at one
    window, each tail statement of the 3-buffer loop, and whole triples."""
    assert ops.assign_kernel_fits(64, D)
    case = ac.assign_case(777, D, 64)
    ac.check_assign(case, *_gpu_assign(case), lowest_index=True)


@pytest.mark.parametrize("C", ASSIGN_CS)
def test_kmeans_assign_exact_centroid_counts(C):
    case = ac.assign_case(777, 128, C)
    ac.check_assign(case, *_gpu_assign(case), lowest_index=True)


@pytest.mark.parametrize("N", ASSIGN_NS)
def test_kmeans_assign_exact_point_counts(N):
    case = ac.assign_case(N, 64, 33)
    ac.check_assign(case, *_gpu_assign(case), lowest_index=True)


def test_kmeans_assign_exact_grid_stride():
    """2048 blocks of 256 rows and 300 rows more: block 0 and 1 loop a second
    time. Every row is checked, the last 300 included."""
    case = ac.assign_case(GRID_STRIDE_N, 64, 64, keep_sims=False)
    ac.check_assign(case, *_gpu_assign(case), lowest_index=True)


def test_kmeans_assign_exact_all_negative():
    """Columns >= C hold zero rows in LDS and score 0, above every real dot."""
    case = ac.assign_case(300, 128, 17, negative=True)
    ac.check_assign(case, *_gpu_assign(case), lowest_index=True)


def test_kmeans_assign_returns_ids_only():
    case = ac.assign_case(257, 64, 33)
    idx = _sync(ops.kmeans_assign(case.points.to(DEV), case.centroids.to(DEV)))
    assert torch.equal(idx.cpu(), case.lowest)


# -- kmeans_assign_scored off the dedicated kernel: cosine_topk with k = 1 --------

@pytest.mark.parametrize("C", ROUTE_CS)
def test_kmeans_assign_scored_general_route_exact(C):
    """B = 66000 points against a handful of centroids: 516 row tiles, one to
    five column tiles. Exact max score; the index achieves it (tie order is
    unspecified on this route)."""
    assert not ops.assign_kernel_fits(C, 64)
    case = ac.assign_case(66000, 64, C)
    ac.check_assign(case, *_gpu_assign(case), lowest_index=False)


def test_kmeans_assign_scored_general_route_in_chunks(monkeypatch):
    """The route cuts N into calls of at most _ASSIGN_CHUNK_ROWS points (2^20
    in production); 30000 here gives two whole calls and a ragged third."""
    assert ops._ASSIGN_CHUNK_ROWS == 1 << 20
    monkeypatch.setattr(ops, "_ASSIGN_CHUNK_ROWS", 30000)
    case = ac.assign_case(66000, 64, 200)
    ac.check_assign(case, *_gpu_assign(case), lowest_index=False)


def test_kmeans_assign_scored_rows_too_wide_for_the_dedicated_kernel():
    """C = 8, D = 1536: 64 centroid rows of 1536 dims do not fit the
    assignment kernel's LDS, the general route answers. Before the fallback
    this raised "D too large for LDS-resident centroids"."""
    assert ops.KMEANS_ASSIGN_MAX_D == 1152 and not ops.assign_kernel_fits(8, 1536)
    case = ac.assign_case(1000, 1536, 8)
    ac.check_assign(case, *_gpu_assign(case), lowest_index=False)


def test_assign_limit_matches_the_extension():
    ext = ops._require_ext()
    assert ext.KMEANS_ASSIGN_MAX_D == ops.KMEANS_ASSIGN_MAX_D == 1152
    z = torch.zeros(4, 1216, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="D too large"):
        ext.kmeans_assign(z, z)


def test_cosine_topk_refuses_more_rows_than_grid_y_holds():
    """65535 row tiles of 128 rows fit grid.y; one row more is refused before
    anything is allocated or launched (the queries are never read)."""
    q = torch.empty((65535 * 128 + 1, 64), dtype=torch.bfloat16, device=DEV)
    c = torch.zeros((200, 64), dtype=torch.bfloat16, device=DEV)
    for k in (1, 5):
        with pytest.raises(RuntimeError, match="row tiles"):
            ops.cosine_topk(q, c, k)
    torch.cuda.synchronize()


# -- embedding_bag --------------------------------------------------------------

def _gpu_bag(case):
    return _sync(ops.embedding_bag(case.table.to(DEV), case.idx.to(DEV), case.w.to(DEV)))


@pytest.mark.parametrize("B,L,D,V", ac.BAG_CASES)
def test_embedding_bag_exact(B, L, D, V):
    ac.check_bag(ac.bag_case(B, L, D, V), _gpu_bag(ac.bag_case(B, L, D, V)))


def test_embedding_bag_exact_int64_indices():
    case = ac.bag_case(64, 48, 1000, 5000, torch.int64)
    ac.check_bag(case, _gpu_bag(case))


def test_embedding_bag_refuses_more_than_128_indices_per_bag():
    table = torch.zeros(7, 64, dtype=torch.bfloat16, device=DEV)
    idx = torch.zeros(2, 129, dtype=torch.int32, device=DEV)
    w = torch.ones(2, 129, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="L must be <= 128"):
        ops.embedding_bag(table, idx, w)


# -- l2normalize_ ----------------------------------------------------------------

def _gpu_norm(case):
    t = case.x.to(DEV)
    ret = ops.l2normalize_(t, case.start, case.end)
    assert ret is t
    return _sync(t)


@pytest.mark.parametrize("D", NORM_DIMS)
def test_l2normalize_bound_dims(D):
    """D = 8: one live lane; 520: 65 vectors, so lane 0 loops twice and 63
    lanes idle; 1536: three passes. Rows scaled by 2^30 and 2^-30 and an
    all-zero row are part of every case."""
    ac.check_norm(ac.norm_case(37, D), _gpu_norm(ac.norm_case(37, D)))


def test_l2normalize_bound_grid_stride_rows():
    """2048 blocks of 4 waves take 8192 rows per sweep; 5 rows more."""
    case = ac.norm_case(8192 + 5, 64)
    ac.check_norm(case, _gpu_norm(case))


def test_l2normalize_row_window_leaves_every_other_row_alone():
    case = ac.norm_case(9000, 64, 3, 8193)
    ac.check_norm(case, _gpu_norm(case))


def test_l2normalize_empty_window_changes_nothing():
    case = ac.norm_case(9000, 64, 3, 8193)
    t = case.x.to(DEV)
    ops.l2normalize_(t, 8, 8)
    ops.l2normalize_(t, 9, 3)
    _sync(t)
    assert torch.equal(t.cpu().view(torch.int16), case.x.view(torch.int16))
