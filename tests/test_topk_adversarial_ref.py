"""CPU half of the adversarial exact-top-k tests.

Every data family of tests/topk_adversarial.py goes through the plain-torch
references (cosine_topk_ref, cosine_topk_filtered_ref, ivf_scan_topk_ref,
EmbeddingStore.search on the CPU) under the same tie-aware float64 checker
the HIP kernels face in tests/test_gpu_topk_adversarial.py: the references
satisfy the contract, and the checker rejects hand-broken results. D = 128
keeps it quick; the checker's tolerance scales with D.
"""

import pytest
import torch

import topk_adversarial as ta

D = 128
N = ta.N_BASE
SMALL_N = 4100


@pytest.fixture(scope="module")
def pc():
    return ta.plan_constants()


@pytest.fixture(scope="module")
def base():
    """65,700 unit rows shared by the module; cases clone what they plant into."""
    return ta.rand_unit(N, D, seed=1)


@pytest.fixture(scope="module")
def negative():
    return ta.negative_corpus(D, N, seed=40)


def test_plan_constants_match_the_shapes_the_families_assume(pc):
    # the prepass samples all of the first MIN_N_EMIT rows on both tile plans
    assert pc["PREG_WARM"] * pc["PRE_TILES"] * pc["BN"] == pc["MIN_N_EMIT"]
    assert pc["MIN_N_EMIT"] <= N <= pc["PREG_EMIT"] * pc["PRE_TILES"] * pc["BN"]
    assert N % pc["BN"] == 36 and N % pc["BN8"] != 0  # a ragged last tile on both plans
    assert N > pc["cap"]  # a flooded corpus overflows the candidate buffer
    assert ta.chunk_columns(16, N, pc["BN"], pc) == 512
    assert ta.chunk_columns(130, N, pc["BN8"], pc) == 1024


@pytest.mark.parametrize("filtered_half", [False, True])
@pytest.mark.parametrize("placement", ["contig", "scattered"])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_duplicate_block(base, pc, k, placement, filtered_half):
    sizes = [14, 24] if filtered_half else ta.dup_sizes(k)  # 7 and 12 eligible copies
    for i, size in enumerate(sizes):
        case = ta.dup_case(D, N, 4, k, size, placement, pc, 100 + 10 * i + k, filtered_half)
        ta.run_case(case, base, ta.search_filtered_ref if filtered_half else ta.search_topk_ref)


def test_duplicate_block_small_corpus(base, pc):
    for size in ta.dup_sizes(8):
        ta.run_case(ta.dup_case(D, SMALL_N, 16, 8, size, "scattered", pc, 200 + size), base,
                    ta.search_topk_ref)


def test_near_duplicate_run(base, pc):
    ta.run_case(ta.neardup_case(D, N, 4, pc, 300), base, ta.search_topk_ref)
    ta.run_case(ta.neardup_case(D, N, 4, pc, 301), base, ta.search_filtered_ref)


def test_flooded_corpus(base):
    ta.run_case(ta.flooded_case(D, N, 4, 8, 310), base, ta.search_topk_ref)
    ta.run_case(ta.flooded_case(D, N, 4, 5, 311), base, ta.search_filtered_ref)


@pytest.mark.parametrize("n,step", [(N, 128), (SMALL_N, 32)])
def test_planted_positions(base, n, step):
    nq = ta.planted_queries_needed(n, step)
    case = ta.planted_case(D, n, nq, step, 320)
    covered = set(case.exact.reshape(-1).tolist())
    assert covered >= set(ta.required_positions(n, step))
    ta.run_case(case, base, ta.search_topk_ref, batch=8 if step == 32 else 0)


def test_k8_at_the_floor(base):
    ta.run_case(ta.floor_case(D, N, 64, 330), base, ta.search_topk_ref, batch=8)


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("n", [100, 1000, N])
def test_all_negative_scores(base, negative, n, k):
    u, corpus = negative
    ta.run_case(ta.negative_case(u, corpus, n, 4, k, 340 + k), base, ta.search_topk_ref)
    ta.run_case(ta.negative_case(u, corpus, n, 4, k, 350 + k), base, ta.search_filtered_ref)


@pytest.mark.parametrize("valid_n", [1000, N])
def test_poison_past_valid_n(base, valid_n):
    ta.run_case(ta.poison_case(D, valid_n, 4, 5, 360), base, ta.search_topk_ref)
    ta.run_case(ta.poison_case(D, valid_n, 4, 8, 361), base, ta.search_filtered_ref)


def test_zero_query(base):
    ta.run_case(ta.zero_query_case(D, N, 4, 8, 370), base, ta.search_topk_ref)
    ta.run_case(ta.zero_query_case(D, SMALL_N, 1, 5, 371), base, ta.search_filtered_ref)


def test_ivf_scan_duplicates(base):
    from kakveda_amd import ops

    iv = ta.ivf_case(D, 380)
    case = iv.case
    c = ta.materialise(case, base)
    scores, idx = ops.ivf_scan_topk_ref(
        case.q, c, iv.offsets, iv.ids, iv.probes, case.k, case.n, iv.tail_lo, iv.tail_hi)
    ta.judge(case, scores, idx, case.q.double() @ c.double().t(), iv.eligible)


def test_segmented_store_duplicates(base):
    from kakveda_amd.gfkb.engine import EmbeddingStore

    case = ta.store_case(D, 390)
    c = ta.materialise(case, base)
    store = EmbeddingStore(D, device="cpu", capacity=256, segment_rows=512)
    store.append(c[:700])
    store.append(c[700:])
    assert store.n_segments == 3 and store.count == case.n
    scores, idx = store.search(case.q, case.k)
    ta.judge(case, scores.float(), idx, case.q.double() @ c.double().t())


# -- the checker rejects broken results ---------------------------------------

@pytest.fixture(scope="module")
def tied(base, pc):
    """A correct answer to a 9-copy duplicate block at k = 8."""
    case = ta.dup_case(D, N, 4, 8, 9, "contig", pc, 400)
    scores, idx = ta.run_case(case, base, ta.search_topk_ref)
    c = ta.materialise(case, base)
    return case, scores, idx, case.q.double() @ c.double().t()


def test_checker_rejects_repeated_index(tied):
    case, scores, idx, sims = tied
    r = case.q.shape[0] - 1
    bad = idx.clone()
    bad[r, 3] = bad[r, 2]  # same score: only the distinctness rule can object
    with pytest.raises(AssertionError, match="row %d rank .*repeated index" % r):
        ta.check_topk(scores, bad, sims, 8, D)


def test_checker_rejects_tie_member_swapped_for_rank_k_plus_1(base, pc):
    # 8 copies at k = 8: rank 9 is an ordinary row far below the tie
    case = ta.dup_case(D, N, 4, 8, 8, "scattered", pc, 410)
    scores, idx = ta.run_case(case, base, ta.search_topk_ref)
    c = ta.materialise(case, base)
    sims = case.q.double() @ c.double().t()
    r = case.q.shape[0] - 1
    top = torch.topk(sims[r], 9)
    bad_s, bad_i = scores.clone(), idx.clone()
    bad_i[r, 7] = top.indices[8]
    bad_s[r, 7] = top.values[8].float()
    with pytest.raises(AssertionError, match="row %d rank 7: score differs from the true score of its rank" % r):
        ta.check_topk(bad_s, bad_i, sims, 8, D)
    # the same swap with the tie's score kept: the claim no longer holds
    with pytest.raises(AssertionError, match="row %d rank 7: claimed score" % r):
        ta.check_topk(scores, bad_i, sims, 8, D)


def test_checker_names_missing_clear_winner():
    """A chain of near-ties 0.9 E apart: the answer that skips the best
    column passes every per-rank rule, and only the clear-winner rule sees
    that column 0 beats the returned third rank by 1.8 E."""
    E = ta.tolerance(D)
    sims = torch.tensor([[1.0, 1.0 - 0.9 * E, 1.0 - 1.8 * E, 1.0 - 2.7 * E, 0.0]], dtype=torch.float64)
    ta.check_topk(sims[:, :3].float(), torch.tensor([[0, 1, 2]]), sims, 3, D)
    with pytest.raises(AssertionError, match="row 0: column 0 .* is missing"):
        ta.check_topk(sims[:, 1:4].float(), torch.tensor([[1, 2, 3]]), sims, 3, D)


def test_checker_rejects_index_past_n(tied):
    case, scores, idx, sims = tied
    bad = idx.clone()
    bad[0, 0] = N
    with pytest.raises(AssertionError, match="row 0 rank 0: index outside"):
        ta.check_topk(scores, bad, sims, 8, D)
    bad[0, 0] = -1
    with pytest.raises(AssertionError, match="row 0 rank 0: index outside"):
        ta.check_topk(scores, bad, sims, 8, D)


def test_checker_rejects_wrong_pads_and_ineligible(base):
    sims = torch.tensor([[0.5, 0.4, 0.3]], dtype=torch.float64)
    elig = torch.tensor([[True, False, True]])
    ok_s = torch.tensor([[0.5, 0.3, float("-inf")]])
    ok_i = torch.tensor([[0, 2, -1]])
    ta.check_topk(ok_s, ok_i, sims, 3, D, elig)
    with pytest.raises(AssertionError, match="ineligible"):
        ta.check_topk(torch.tensor([[0.5, 0.4, float("-inf")]]), torch.tensor([[0, 1, -1]]), sims, 3, D, elig)
    with pytest.raises(AssertionError, match="pad score"):
        ta.check_topk(torch.tensor([[0.5, 0.3, -1e30]]), ok_i, sims, 3, D, elig)
    with pytest.raises(AssertionError, match="pad index"):
        ta.check_topk(ok_s, torch.tensor([[0, 2, 1]]), sims, 3, D, elig)
