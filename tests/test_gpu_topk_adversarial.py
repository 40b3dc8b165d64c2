"""GPU tests of the exact top-k on data where kernels go wrong and random
unit vectors never do: bit-identical duplicates (ties), near-duplicate runs,
a flooded corpus, matches pinned to tile and chunk edges, all-negative
scores, poison past valid_n and an all-zero query.

Oracle: float64 inner products of the same bf16 inputs under the tie-aware
checker of tests/topk_adversarial.py (tolerance E = D * 2^-23), plus set or
order equality wherever the data fixes the answer. The shapes are the
smallest that reach each dispatch path (kakveda_amd/ops/hip/knn_plan.h):

  list128      B=16,  N=4,100    List128, no prepass, topk_merge_small
  argmax128    B=16,  N=4,100    k = 1
  smallb       B=1/8, N=65,700   streaming kernel v4 behind the emission floors
  emit8p       B=9/130           8-phase emission kernel
  filt_list    B=16,  N=65,700   filtered List128 + threshold prepass + topk_merge
  filt_smallb  B=4               filtered streaming kernel
  child runs                     KAKVEDA_KNN_EMIT_CAP=4 (the overflow fallback:
                                 unfiltered List128 + prepass) and KAKVEDA_SMALLB=2

At N = 65,700 the prepass samples the whole corpus on the 128- and the
256-tile plan, and 36 columns of the last 128-tile are real.
"""

import os
import subprocess
import sys

import pytest
import torch

import topk_adversarial as ta

pytestmark = pytest.mark.gpu

D = 768
N = ta.N_BASE
SMALL_N = 4100

# name -> (search, B, N)
PATHS = {
    "list128": (ta.search_topk, 16, SMALL_N),
    "smallb_b1": (ta.search_topk, 1, N),
    "smallb_b8": (ta.search_topk, 8, N),
    "emit8p_b9": (ta.search_topk, 9, N),
    "emit8p_b130": (ta.search_topk, 130, N),
    "filt_list": (ta.search_filtered, 16, N),
    "filt_smallb": (ta.search_filtered, 4, N),
}
ARGMAX = (ta.search_topk, 16, SMALL_N)


def _seed(*parts):
    """A stable per-case seed (str hashes change between processes)."""
    h = 17
    for p in parts:
        for ch in str(p):
            h = (h * 31 + ord(ch)) % 1_000_003
    return h * 10


@pytest.fixture(scope="module")
def pc():
    pc = ta.plan_constants()
    # the shapes above reach the paths they are named for
    assert SMALL_N < pc["PREG_WARM"] * pc["PRE_TILES"] * pc["BN"] <= pc["MIN_N_EMIT"] <= N
    assert N <= pc["PREG_EMIT"] * pc["PRE_TILES"] * pc["BN"] and N > pc["cap"]
    assert pc["SMALLB_MAX"] == 8 and pc["KMAX"] == 8
    return pc


@pytest.fixture(scope="module")
def base():
    """65,700 unit rows on the GPU, built once; cases clone what they plant into."""
    return ta.rand_unit(N, D, seed=1).to("cuda:0")


@pytest.fixture(scope="module")
def negative():
    u, c = ta.negative_corpus(D, N, seed=40)
    return u, c.to("cuda:0")


def _dup_params():
    out = []
    for path in PATHS:
        for k in (5, 8):
            for placement in ("contig", "scattered"):
                for size in ta.dup_sizes(k):
                    out.append((path, k, placement, size))
    for placement in ("contig", "scattered"):
        for size in ta.dup_sizes(1):
            out.append(("argmax128", 1, placement, size))
    return out


@pytest.mark.parametrize("path,k,placement,size", _dup_params())
def test_duplicate_block(base, pc, path, k, placement, size):
    search, B, n = ARGMAX if path == "argmax128" else PATHS[path]
    case = ta.dup_case(D, n, B, k, size, placement, pc, _seed(path, k, placement, size))
    ta.run_case(case, base, search)


@pytest.mark.parametrize("size", [14, 24])  # 7 and 12 eligible copies
@pytest.mark.parametrize("placement", ["contig", "scattered"])
@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize("path", ["filt_list", "filt_smallb"])
def test_duplicate_block_half_labelled_away(base, pc, path, k, placement, size):
    search, B, n = PATHS[path]
    case = ta.dup_case(D, n, B, k, size, placement, pc, _seed("half", path, k, placement, size),
                       filtered_half=True)
    ta.run_case(case, base, search)


@pytest.mark.parametrize("path", list(PATHS))
def test_near_duplicate_run(base, pc, path):
    search, B, n = PATHS[path]
    ta.run_case(ta.neardup_case(D, n, B, pc, _seed("near", path)), base, search)


@pytest.mark.parametrize("path", list(PATHS) + ["argmax128"])
def test_flooded_corpus(base, path):
    """All N rows tie; at N = 65,700 that is more than the candidate buffer
    holds, so the batch reruns through the list kernel in-process (with its
    one-line warning on stderr)."""
    search, B, n = ARGMAX if path == "argmax128" else PATHS[path]
    k = 1 if path == "argmax128" else 8
    ta.run_case(ta.flooded_case(D, n, B, k, _seed("flood", path)), base, search)


@pytest.mark.parametrize("path,n", [("emit8p", N), ("filt_list", N), ("list128", SMALL_N)])
def test_planted_positions_mfma(base, pc, path, n):
    """B = 300: the planted rows cover both sides of every 128-column
    boundary, column 0 and the whole ragged last tile."""
    case = ta.planted_case(D, n, 300, pc["BN"], _seed("planted", path))
    assert set(case.exact.reshape(-1).tolist()) >= set(ta.required_positions(n, pc["BN"]))
    ta.run_case(case, base, ta.search_filtered if path == "filt_list" else ta.search_topk)


@pytest.mark.parametrize("filtered", [False, True])
def test_planted_positions_streaming(base, filtered):
    """B = 8 calls against one planted corpus: together the planted rows
    cover both sides of every multiple of 32 (a streaming block's row group;
    its waves' 8-row groups and the older kernel's 256-row groups start at
    such multiples), column 0 and the last tile."""
    nq = ta.planted_queries_needed(N, 32)
    case = ta.planted_case(D, N, nq, 32, _seed("planted-stream", filtered))
    assert set(case.exact.reshape(-1).tolist()) >= set(ta.required_positions(N, 32))
    ta.run_case(case, base, ta.search_filtered if filtered else ta.search_topk, batch=8)


@pytest.mark.parametrize("filtered", [False, True])
def test_k8_at_the_floor(base, filtered):
    """64 random queries as eight B = 8 calls at k = 8: the emission floor is
    the 8th best of a sample that is the whole corpus, so the 8th match sits
    exactly on it."""
    case = ta.floor_case(D, N, 64, _seed("floor", filtered))
    ta.run_case(case, base, ta.search_filtered if filtered else ta.search_topk, batch=8)


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("n", [100, 1000, N])
@pytest.mark.parametrize("path", ["topk_b1", "topk_b16", "topk_b130", "filt_b4", "filt_b16"])
def test_all_negative_scores(base, negative, path, n, k):
    u, corpus = negative
    search = ta.search_topk if path.startswith("topk") else ta.search_filtered
    B = int(path.split("_b")[1])
    ta.run_case(ta.negative_case(u, corpus, n, B, k, _seed("neg", path, n, k)), base, search)


@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize("valid_n", [1000, N])
@pytest.mark.parametrize("path", ["topk_b1", "topk_b8", "topk_b16", "topk_b130", "filt_b4", "filt_b16"])
def test_poison_past_valid_n(base, path, valid_n, k):
    search = ta.search_topk if path.startswith("topk") else ta.search_filtered
    B = int(path.split("_b")[1])
    ta.run_case(ta.poison_case(D, valid_n, B, k, _seed("poison", path, valid_n, k)), base, search)


@pytest.mark.parametrize("path", list(PATHS) + ["argmax128"])
def test_zero_query(base, path):
    search, B, n = ARGMAX if path == "argmax128" else PATHS[path]
    k = 1 if path == "argmax128" else 8
    ta.run_case(ta.zero_query_case(D, n, B, k, _seed("zero", path)), base, search)


def test_ivf_scan_duplicates(base):
    from kakveda_amd import ops

    iv = ta.ivf_case(D, 380)
    case = iv.case
    c = ta.materialise(case, base)
    q = case.q.to(c.device)
    scores, idx = ops.ivf_scan_topk(
        q, c, iv.offsets, iv.ids, iv.probes, case.k, case.n, iv.tail_lo, iv.tail_hi)
    torch.cuda.synchronize()
    ta.judge(case, scores, idx, q.double() @ c.double().t(), iv.eligible)


def test_segmented_store_duplicates(base):
    from kakveda_amd.gfkb.engine import EmbeddingStore

    case = ta.store_case(D, 390)
    c = ta.materialise(case, base)
    store = EmbeddingStore(D, device="cuda", capacity=256, segment_rows=512)
    store.append(c[:700])
    store.append(c[700:])
    assert store.n_segments == 3 and store.count == case.n
    q = case.q.to(c.device)
    scores, idx = store.search(q, case.k)
    torch.cuda.synchronize()
    ta.judge(case, scores, idx, q.double() @ c.double().t())  # global ids, distinct


def _child(env_set, batches):
    """The duplicate-block and k = 8 families in a fresh process (these
    settings are read once per process)."""
    env = dict(os.environ)
    for name in ("KAKVEDA_KNN_KERNEL", "KAKVEDA_SMALLB", "KAKVEDA_KNN_EMIT_CAP",
                 "KAKVEDA_KNN_PREPASS", "KAKVEDA_KNN_PREG", "KAKVEDA_KNN_TARGET"):
        env.pop(name, None)
    env.update(env_set)
    r = subprocess.run(
        [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "topk_adversarial.py"),
         str(D), batches],
        env=env, capture_output=True, text=True, timeout=300,
    )
    fails = [l for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert r.returncode == 0 and "failures=0" in r.stdout, (
        "%d failing cases:\n%s\n%s" % (len(fails), "\n".join(fails), r.stderr[-1500:]))
    return r


def test_overflow_fallback_list_kernel_with_prepass():
    """A candidate cap of 4 sends every batch to the fallback: the unfiltered
    128x128 list kernel behind its threshold prepass at N >= 64k."""
    r = _child({"KAKVEDA_KNN_EMIT_CAP": "4"}, "1,16,130")
    assert "emission candidate overflow" in r.stderr


def test_smallb_v2_streaming_kernel():
    _child({"KAKVEDA_SMALLB": "2"}, "1,8")
