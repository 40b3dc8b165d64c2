"""GPU tests of the label-filtered exact top-k (ops.cosine_topk_filtered).

Oracle: fp32 torch on the same bf16 inputs with ineligible columns set to
-inf. Score tolerances are those of tests/test_gpu_ops.py. For every
returned index the tests assert that it is eligible, below valid_n and
achieves its score; pads must sit exactly where the oracle runs out of
eligible rows. Unless a case says otherwise its batch mixes filtered
queries with unfiltered ones (want = -1).
"""

import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 768
N_BIG = 300_000
N_STREAM = 70_000  # >= MIN_N_EMIT: B <= 8 takes the streaming kernel


def _dev():
    return torch.device("cuda:0")


def _rand_unit(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float32, device=_dev())
    x = x / x.norm(dim=-1, keepdim=True)
    return x.to(torch.bfloat16)


def _rand_labels(n, seed, n_labels=4):
    """n_labels random labels plus unlabelled (-1) rows, about 1/(n+1) each."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-1, n_labels, (n,), generator=g, dtype=torch.int32).to(_dev())


def _mixed_want(B, seed, n_labels=4):
    """Random wants over {-1, 0..n_labels-1}; rows 0/1 pinned so every batch
    of two or more rows has a filtered and an unfiltered query."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randint(-1, n_labels, (B,), generator=g, dtype=torch.int32)
    w[0] = 2
    if B > 1:
        w[1] = -1
    return w.to(_dev())


@pytest.fixture(scope="module")
def corpus():
    """One 300k-row corpus for the whole module; never modified (cases that
    plant rows clone the slice they need)."""
    return _rand_unit(N_BIG, D, seed=2)


@pytest.fixture(scope="module")
def queries():
    return _rand_unit(300, D, seed=1)


def _oracle(q, c, labels, want, k, n):
    sims = q.float() @ c[:n].float().t()
    w = want.long()[:, None]
    eligible = (w < 0) | (labels[:n].long()[None, :] == w)
    ref_scores, _ = torch.topk(sims.masked_fill(~eligible, float("-inf")), k, dim=1)
    return sims, eligible, ref_scores


def _check(q, c, labels, want, k, valid_n=None):
    from kakveda_amd import ops

    n = c.shape[0] if valid_n is None else valid_n
    B = q.shape[0]
    scores, idx = ops.cosine_topk_filtered(q, c, labels, want, k, valid_n=valid_n)
    torch.cuda.synchronize()
    sims, eligible, ref_scores = _oracle(q, c, labels, want, k, n)

    assert scores.shape == (B, k) and idx.shape == (B, k)
    assert scores.dtype == torch.float32 and idx.dtype == torch.int64
    assert (scores[:, :-1] >= scores[:, 1:] - 1e-6).all()
    # pads exactly where the oracle has fewer than k eligible rows
    ref_pad = torch.isinf(ref_scores)
    assert torch.equal(idx < 0, ref_pad), (idx, ref_scores)
    assert (idx[ref_pad] == -1).all()
    assert (scores[ref_pad] == float("-inf")).all()
    hit = ~ref_pad
    assert (idx[hit] < n).all()
    assert torch.allclose(scores[hit], ref_scores[hit], atol=2e-2, rtol=1e-2), (
        (scores[hit] - ref_scores[hit]).abs().max().item()
    )
    # every returned index is eligible and achieves its claimed score
    safe = idx.clamp_min(0)
    assert eligible.gather(1, safe)[hit].all()
    gathered = sims.gather(1, safe)
    assert torch.allclose(gathered[hit], scores[hit], atol=1e-4), (
        (gathered[hit] - scores[hit]).abs().max().item()
    )
    return scores, idx


# -- list kernel, with row and column tails ---------------------------------

@pytest.mark.parametrize("B,N,k", [(1, 100, 5), (100, 1000, 5), (130, 4100, 8)])
def test_list_kernel_tails(corpus, queries, B, N, k):
    # B=1 cannot mix: its one query is filtered
    _check(queries[:B], corpus[:N], _rand_labels(N, 10 + B), _mixed_want(B, 20 + B), k)


def test_list_kernel_d128():
    q = _rand_unit(70, 128, seed=3)
    c = _rand_unit(1000, 128, seed=4)
    _check(q, c, _rand_labels(1000, 5), _mixed_want(70, 6), 5)


# -- few eligible rows ------------------------------------------------------

@pytest.mark.parametrize("N", [1000, N_STREAM])
def test_few_eligible_rows_pad(corpus, queries, N):
    labels = _rand_labels(N, 30)
    labels[torch.tensor([7, N // 2, N - 1])] = 7  # exactly 3 rows carry 7
    want = torch.tensor([7, 9, -1, 0], dtype=torch.int32, device=_dev())  # 9: nobody
    scores, idx = _check(queries[:4], corpus[:N], labels, want, 5)
    assert sorted(idx[0, :3].tolist()) == [7, N // 2, N - 1]
    assert idx[0, 3:].tolist() == [-1, -1]
    assert idx[1].tolist() == [-1] * 5
    assert (idx[2:] >= 0).all()


# -- planted duplicates -----------------------------------------------------

@pytest.mark.parametrize("N", [5000, N_STREAM])
def test_ineligible_copy_hidden_eligible_near_copy_first(corpus, queries, N):
    q = queries[:4]
    c = corpus[:N].clone()
    labels = _rand_labels(N, 31)
    want = torch.tensor([2, -1, 0, 3], dtype=torch.int32, device=_dev())
    c[1234] = q[0]  # exact copy, score ~1.0, wrong label
    labels[1234] = 1
    near = q[0].float() + 0.02 * _rand_unit(1, D, seed=32)[0].float()
    c[N - 77] = (near / near.norm()).to(torch.bfloat16)
    labels[N - 77] = 2
    scores, idx = _check(q, c, labels, want, 5)
    assert 1234 not in idx[0].tolist()
    assert idx[0, 0].item() == N - 77 and scores[0, 0].item() > 0.9
    # the unfiltered query in the same batch is not affected by others' wants
    c[4321] = q[1]
    scores, idx = _check(q, c, labels, want, 5)
    assert idx[1, 0].item() == 4321


def test_valid_n_hides_eligible_match(corpus, queries):
    q = queries[:16]
    c = corpus[:1000].clone()
    labels = _rand_labels(1000, 33)
    want = _mixed_want(16, 34)
    c[900] = q[0]
    labels[900] = int(want[0])  # eligible, but beyond the valid prefix
    scores, idx = _check(q, c, labels, want, 5, valid_n=800)
    assert (idx < 800).all()
    assert scores[0, 0].item() < 0.9


# -- streaming kernel and the shapes just past it ---------------------------

@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("B", [1, 4, 8])
def test_streaming_kernel(corpus, queries, B, k):
    # B=1 cannot mix: its one query is filtered
    _check(queries[:B], corpus[:N_STREAM], _rand_labels(N_STREAM, 40), _mixed_want(B, 41 + B), k)


@pytest.mark.parametrize("B", [9, 300])
def test_past_streaming_limit(corpus, queries, B):
    _check(queries[:B], corpus[:N_STREAM], _rand_labels(N_STREAM, 42), _mixed_want(B, 43 + B), 5)


# -- emission floors --------------------------------------------------------

def _plan_constants():
    """PRE_TILES, BN, the emission prepass width and the default candidate
    cap, read from the dispatch plan header."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(here, "kakveda_amd", "ops", "hip", "knn_plan.h")).read()

    def const(pattern):
        return int(re.search(pattern, text).group(1))

    return {
        "PRE_TILES": const(r"constexpr int PRE_TILES = (\d+);"),
        "BN": const(r"constexpr int BN = (\d+);"),
        "PREG_EMIT": const(r"constexpr int PREG_EMIT = (\d+);"),
        "cap": const(r"long cap = (\d+);"),
    }


def test_floor_degenerate_label_at_far_end(corpus, queries):
    """A label carried only by 20 rows at the end of the store: the prepass
    sample holds none, no floor is published for those queries, and all 20
    are emitted (far below the candidate cap)."""
    labels = _rand_labels(N_BIG, 50)
    labels[N_BIG - 20 :] = 5
    want = torch.tensor([5, -1, 0, 5], dtype=torch.int32, device=_dev())
    scores, idx = _check(queries[:4], corpus, labels, want, 8)
    assert (idx[0] >= N_BIG - 20).all() and (idx[3] >= N_BIG - 20).all()


def test_overflow_falls_back_exactly(corpus, queries):
    """One label on every row past the prepass sample, another below: the
    filtered floor stays unset, more eligible rows than the candidate cap are
    emitted, and the batch reruns through the filtered list kernel."""
    pc = _plan_constants()
    sampled = pc["PREG_EMIT"] * pc["PRE_TILES"] * pc["BN"]
    assert sampled < N_BIG and N_BIG - sampled > pc["cap"], (sampled, pc)
    labels = torch.zeros(N_BIG, dtype=torch.int32, device=_dev())
    labels[sampled:] = 1
    want = torch.tensor([1, -1, 0, 1], dtype=torch.int32, device=_dev())
    scores, idx = _check(queries[:4], corpus, labels, want, 5)
    assert (idx[0] >= sampled).all() and (idx[3] >= sampled).all()
    assert (idx[2] < sampled).all()


# -- segmented store --------------------------------------------------------

def test_segmented_store_filtered_search(corpus, queries):
    from kakveda_amd.gfkb.engine import EmbeddingStore

    n = 1300
    store = EmbeddingStore(D, device="cuda", capacity=256, segment_rows=512)
    labels = _rand_labels(n, 60)
    labels[n - 3 :] = 6  # a label living only in the last segment
    store.append(corpus[:700], labels[:700])
    store.append(corpus[700:n], labels[700:n])
    assert store.n_segments == 3 and store.count == n
    assert torch.equal(store.label_range(0, n), labels)

    q = queries[:6]
    want = torch.tensor([2, -1, 6, 0, 3, 6], dtype=torch.int32, device=_dev())
    scores, idx = store.search(q, 5, want=want)
    torch.cuda.synchronize()
    sims, eligible, ref_scores = _oracle(q, corpus[:n], labels, want, 5, n)
    ref_pad = torch.isinf(ref_scores)
    assert torch.equal(idx < 0, ref_pad)
    hit = ~ref_pad
    assert torch.allclose(scores[hit], ref_scores[hit], atol=2e-2, rtol=1e-2)
    safe = idx.clamp_min(0)
    assert eligible.gather(1, safe)[hit].all()  # global row ids
    assert torch.allclose(sims.gather(1, safe)[hit], scores[hit], atol=1e-4)
    assert sorted(idx[2, :3].tolist()) == [n - 3, n - 2, n - 1]
    assert idx[2, 3:].tolist() == [-1, -1]
    # want=None is the unfiltered search
    s0, i0 = store.search(q, 5)
    s1, i1 = store.search(q, 5, want=torch.full((6,), -1, dtype=torch.int32))
    assert torch.equal(i0, i1) and torch.allclose(s0, s1, atol=1e-4)
