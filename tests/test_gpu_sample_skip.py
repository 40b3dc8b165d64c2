"""GPU tests of the emission main launch that starts after the prepass sample.

The 8-phase emission plan scores the first S = preg * 1024 corpus columns in
its prepass, seeds each row's candidate list with the sample's best 8 and
launches the main kernel over the columns from S on (knn_plan.h
main_geometry). The cases sit where that can go wrong:

  B=256, N=65,536    the sample is the corpus: the whole-corpus launch stays
  B=300, N=70,000    S = 73,728 is larger than N: likewise
  B=9,   N=300,000   S = 262,144; 37,856 columns remain, the last tile partial
  B=130, N=262,145   one column remains; every query's best match planted in
                     it, at S-1, and a copy on either side of S
  straddle           nine bit-identical copies of a query's best row, five
                     below S and four from S on; and a query whose eight best
                     are all unsampled (S, the partial last tile included)

and, in child processes (the KAKVEDA_KNN_* settings are read once per
process), with KAKVEDA_KNN_PREG=8 (S = 8,192), so that most of the corpus
goes through the main kernel: N=65,700 at B=300 and N=300,000 at B=2048
(eight row tiles, several chunks per XCD, the XCD remap taken); the same
with KAKVEDA_KNN_SKIP_SAMPLE=0, whose outputs on the random-data cases must
equal the default's bit for bit; and with KAKVEDA_KNN_EMIT_CAP=4, where the
eight seeded candidates alone overflow the lists and the batch must come
out exact through the list-kernel fallback.

Oracle: the fp32 torch product of the same bf16 inputs under the tie-aware
checker of tests/topk_adversarial.py (E = D * 2^-23), D = 768 and D = 64,
k = 5 and k = 8.
"""

import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_adversarial as ta  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (768, 64)
N_MAX = 300_000
DEV = "cuda:0"


def sample_columns(B, N, pc, preg_env=0):
    """S of the unfiltered 8-phase emission plan (knn_plan.h)."""
    row_tiles = (B + pc["BM8"] - 1) // pc["BM8"]
    ntiles = (N + pc["BN8"] - 1) // pc["BN8"]
    want = (ntiles * row_tiles + pc["target8"] - 1) // pc["target8"]
    chunk_tiles = max(4, min(want, 128))
    nchunks = ((ntiles + chunk_tiles - 1) // chunk_tiles + 7) & ~7
    preg = min(preg_env if preg_env > 0 else pc["PREG_EMIT"], nchunks) & ~7
    return preg * pc["PRE_TILES"] * pc["BN"]


def gpu_unit(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, d, generator=g, device=DEV, dtype=torch.float32)
    x /= x.norm(dim=-1, keepdim=True)
    return x.to(torch.bfloat16)


def run(case, base, rows=256):
    """ta.run_case with the fp32 product as the reference, judged in slices
    of ``rows`` query rows (bounds the reference's memory)."""
    from kakveda_amd import ops

    c = ta.materialise(case, base)
    q = case.q.to(c.device)
    scores, idx = ops.cosine_topk(q, c, case.k, valid_n=case.n)
    torch.cuda.synchronize()
    cf = c[: case.n].float()
    for r0 in range(0, q.shape[0], rows):
        r1 = min(r0 + rows, q.shape[0])
        sims = (q[r0:r1].float() @ cf.t()).double()
        ordered = {r - r0: v for r, v in case.ordered.items() if r0 <= r < r1}
        part = ta.Case(
            name="%s[rows %d..%d]" % (case.name, r0, r1), q=case.q[r0:r1], n=case.n, k=case.k,
            within={r - r0: v for r, v in case.within.items() if r0 <= r < r1},
            contains={r - r0: v for r, v in case.contains.items() if r0 <= r < r1},
            ordered=ordered, min_gap_E=case.min_gap_E if ordered else 0.0,
        )
        ta.judge(part, scores[r0:r1], idx[r0:r1], sims)
    return scores, idx


def random_case(d, B, n, k, seed):
    return ta.Case(name="random[D=%d,B=%d,N=%d,k=%d]" % (d, B, n, k),
                   q=gpu_unit(B, d, seed).cpu(), n=n, k=k)


def common_best_case(d, B, n, k, positions, seed):
    """Queries normalize(u + 0.5 g_b): the row u, planted at ``positions``,
    has cosine about 0.89 to every query, far above any random row."""
    u = gpu_unit(1, d, seed).float()
    q = u + 0.5 * gpu_unit(B, d, seed + 1).float()
    q /= q.norm(dim=-1, keepdim=True)
    return ta.Case(
        name="commonbest[D=%d,B=%d,N=%d,k=%d,at=%s]" % (d, B, n, k, positions),
        q=q.to(torch.bfloat16).cpu(), n=n, k=k,
        plant_pos=torch.tensor(positions, dtype=torch.int64),
        plant_rows=u.to(torch.bfloat16).cpu().expand(len(positions), d).contiguous(),
        contains={b: positions for b in range(B)},
    )


def straddle_case(d, B, n, k, S, seed):
    """Row B-1: nine copies of the query at S-5 .. S+3. Row 0: a
    near-duplicate run of eight at unsampled columns only."""
    g = torch.Generator().manual_seed(seed)
    q = gpu_unit(B, d, seed).cpu()
    dup = list(range(S - 5, S + 4))
    far = [S + 4, S + 255, S + 256, S + 1000, n - 300, n - 33, n - 2, n - 1]
    assert S + 1000 < n - 300 and all(S <= p < n for p in far)
    near = ta.near_rows(q[0:1], g)[0]
    if k < 8:
        far, near = far[:k], near[:k]
    # at D = 64 random rows reach cosine 0.6: only then is the run's order the answer
    fixed = {0: far} if d >= 256 else {}
    return ta.Case(
        name="straddle[D=%d,B=%d,N=%d,k=%d,S=%d]" % (d, B, n, k, S), q=q, n=n, k=k,
        plant_pos=torch.tensor(dup + far, dtype=torch.int64),
        plant_rows=torch.cat([q[B - 1 : B].expand(9, d), near], dim=0).contiguous(),
        within={B - 1: dup}, ordered=fixed, min_gap_E=100.0 if fixed else 0.0,
    )


@pytest.fixture(scope="module")
def pc():
    return ta.plan_constants()


@pytest.fixture(scope="module")
def bases():
    """300,000 unit rows per dimension, built once on the GPU; cases clone
    the prefix they plant into."""
    return {d: gpu_unit(N_MAX, d, seed=11 + d) for d in DIMS}


@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("B,n", [(256, 65_536), (300, 70_000), (9, 300_000)])
def test_random_queries(bases, pc, B, n, d, k):
    S = sample_columns(B, n, pc)
    assert {65_536: S == n, 70_000: S > n, 300_000: S == 262_144}[n]
    run(random_case(d, B, n, k, 1000 + B + k), bases[d])


@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("where", ["S", "S-1", "S-1 and S"])
def test_best_match_at_the_sample_edge(bases, pc, where, d, k):
    B, n = 130, 262_145
    S = sample_columns(B, n, pc)
    assert S == n - 1
    positions = {"S": [S], "S-1": [S - 1], "S-1 and S": [S - 1, S]}[where]
    run(common_best_case(d, B, n, k, positions, 2000 + k), bases[d])


@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize("d", DIMS)
def test_duplicates_straddle_the_sample_edge(bases, pc, d, k):
    B, n = 9, 300_000
    S = sample_columns(B, n, pc)
    assert S == 262_144
    run(straddle_case(d, B, n, k, S, 3000 + k), bases[d])


# ---------------------------------------------------------------------------
# child processes: a forced small sample, the off switch, the overflow fallback
# ---------------------------------------------------------------------------

CHILD_PREG = 8
CHILD_SHAPES = {"small": [(300, 65_700)], "full": [(300, 65_700), (2048, 300_000)]}


def child_main(argv):
    """``python tests/test_gpu_sample_skip.py SHAPES OUT``: the random and the
    straddling cases at the SHAPES under the caller's KAKVEDA_* environment;
    saves the random cases' outputs to OUT; exit 1 on any failure."""
    sys.path.insert(0, ta.REPO)
    shapes, out = CHILD_SHAPES[argv[0]], argv[1]
    pc = ta.plan_constants()
    preg = int(os.environ.get("KAKVEDA_KNN_PREG", "0"))
    bases = {d: gpu_unit(N_MAX, d, seed=11 + d) for d in DIMS}
    failures, ncases, saved = 0, 0, {}
    for B, n in shapes:
        S = sample_columns(B, n, pc, preg)
        for d in DIMS:
            for k in (5, 8):
                cases = [random_case(d, B, n, k, 4000 + B + k)]
                if S + 2000 < n:
                    cases.append(straddle_case(d, B, n, k, S, 5000 + k))
                for case in cases:
                    ncases += 1
                    try:
                        scores, idx = run(case, bases[d])
                        if case.name.startswith("random"):
                            saved[case.name] = (scores.cpu(), idx.cpu())
                    except AssertionError as exc:
                        failures += 1
                        print("FAIL %s" % str(exc).replace("\n", " ")[:600], flush=True)
    torch.save(saved, out)
    print("CHILD cases=%d failures=%d" % (ncases, failures), flush=True)
    return 1 if failures else 0


def _child(env_set, shapes, out):
    env = dict(os.environ)
    for name in list(env):
        if name.startswith("KAKVEDA_KNN_") or name == "KAKVEDA_SMALLB":
            env.pop(name)
    env.update(env_set)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), shapes, str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    fails = [l for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert r.returncode == 0 and "failures=0" in r.stdout, (
        "%d failing cases:\n%s\n%s" % (len(fails), "\n".join(fails), r.stderr[-1500:]))
    return r


@pytest.fixture(scope="module")
def small_sample_outputs(tmp_path_factory):
    out = tmp_path_factory.mktemp("skip") / "default.pt"
    _child({"KAKVEDA_KNN_PREG": str(CHILD_PREG)}, "full", out)
    return torch.load(out)


def test_small_sample_reaches_the_main_kernel(small_sample_outputs):
    """KAKVEDA_KNN_PREG=8: S = 8,192, the rest of the corpus is scanned by
    the main kernel from tile 32 on."""
    assert len(small_sample_outputs) == 2 * len(DIMS) * 2


def test_off_switch_is_bit_identical(small_sample_outputs, tmp_path):
    """KAKVEDA_KNN_SKIP_SAMPLE=0 scans the whole corpus over the old chunks;
    on random data (no ties) its outputs equal the default's bit for bit."""
    out = tmp_path / "off.pt"
    _child({"KAKVEDA_KNN_PREG": str(CHILD_PREG), "KAKVEDA_KNN_SKIP_SAMPLE": "0"}, "full", out)
    off = torch.load(out)
    assert sorted(off) == sorted(small_sample_outputs)
    for name, (scores, idx) in small_sample_outputs.items():
        assert torch.equal(scores.view(torch.int32), off[name][0].view(torch.int32)), name
        assert torch.equal(idx, off[name][1]), name


def test_seeded_overflow_takes_the_fallback(tmp_path):
    """A candidate cap of 4: the eight seeded candidates alone exceed it, so
    every batch reruns through the list kernel and is still exact."""
    r = _child({"KAKVEDA_KNN_PREG": str(CHILD_PREG), "KAKVEDA_KNN_EMIT_CAP": "4"},
               "small", tmp_path / "cap4.pt")
    assert "emission candidate overflow" in r.stderr


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1:]))
