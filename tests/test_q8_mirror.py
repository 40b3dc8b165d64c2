"""CPU tests of the int8 row mirror: the quantiser's contract, the bound the
two-stage search rests on, the two-stage reference against the exact one on
the adversarial families, and the store / engine / config plumbing.

Inputs and checks shared with tests/test_gpu_q8.py are in tests/q8_cases.py.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_adversarial as ta  # noqa: E402
from q8_cases import (  # noqa: E402
    D, PLANT_B, PLANT_K, PLANT_RUN, check_quantised, encoder_rows, planted_q8_case,
    quantise_ref, quantiser_rows,
)

from kakveda_amd import ops  # noqa: E402
from kakveda_amd.gfkb.engine import EmbeddingStore, GfkbEngine  # noqa: E402

N = ta.N_BASE


# ---------------------------------------------------------------------------
# quantiser
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", [128, 384, 768])
def test_quantiser_spec(d):
    rows = torch.cat([quantiser_rows(d, 200, 11), encoder_rows(40, d)])
    codes, meta = quantise_ref(rows)
    check_quantised(rows, codes, meta)
    # the tie row: inv == 1, so the codes are the values rounded half to even
    tie = rows[1].float()
    assert meta[1, 0].item() == 1.0
    assert codes[1].tolist() == torch.round(tie).to(torch.int8).tolist()
    assert codes[1, :8].tolist() == [0, 2, 2, 0, -2, -2, 64, -126]
    # the huge element takes the whole range; the rest of that row rounds to 0
    assert codes[2, 3].item() == 127 and int(codes[2].abs().sum()) == 127
    # the row of +-amax is represented exactly
    assert meta[4, 1].item() <= 1e-7 and set(codes[4].tolist()) == {-127, 127}


def test_quantiser_first_row_and_dim_check():
    rows = quantiser_rows(128, 9, 12)
    codes, meta = ops.new_q8_mirror(20, 128, "cpu")
    ops.quantize_rows_q8(rows, codes, meta, 5)
    want_c, want_m = quantise_ref(rows)
    assert torch.equal(codes[5:14], want_c) and torch.equal(meta[5:14], want_m)
    assert int(codes[:5].abs().sum()) == 0 and int(codes[14:].abs().sum()) == 0
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.new_q8_mirror(4, 192, "cpu")
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.quantize_rows_q8(torch.zeros(2, 64), torch.zeros(2, 64, dtype=torch.int8),
                             torch.zeros(2, 2), 0)


# ---------------------------------------------------------------------------
# the bound, and the planted input
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def base():
    return ta.rand_unit(N, D, seed=1)


@pytest.fixture(scope="module")
def planted(base):
    case = planted_q8_case()
    c = ta.materialise(case, base)
    codes, meta = quantise_ref(c)
    return case, c, codes, meta


def test_bound_holds_for_every_pair(planted):
    case, c, codes, meta = planted
    q = case.q
    exact = q.double() @ c.double().t()
    approx = (q.double() @ codes.double().t()) * meta[:, 0].double()[None, :]
    qn = q.double().norm(dim=1)
    bound = qn[:, None] * meta[:, 1].double()[None, :] + D * 2.0 ** -22
    assert int(((exact - approx).abs() > bound).sum()) == 0


def test_planted_input_discriminates(planted):
    case, c, codes, meta = planted
    exact = case.q.double() @ c.double().t()
    top = torch.topk(exact, PLANT_K, dim=1).indices
    # (bf16 rounding moves each planted cosine by about as much as the runs
    # are spaced, so the true order is what float64 says, not 0, 1, 2, ...)
    own = torch.arange(PLANT_B)[:, None] * PLANT_RUN
    assert bool(((top >= own) & (top < own + PLANT_RUN)).all())
    with_margin = ops.q8_emit_mask_ref(case.q, c, codes, meta, case.n)
    without = ops.q8_emit_mask_ref(case.q, c, codes, meta, case.n, margin=False)
    assert bool(with_margin.gather(1, top).all())
    lost = int((~without.gather(1, top)).sum())
    print("true top-8 rows lost without the margin:", lost,
          "candidates per query with it:", with_margin.sum(dim=1).tolist())
    assert lost >= 1
    # without stage 2 the order would be the int8 scores': it differs
    s8 = ops.q8_scores_ref(case.q, codes, meta)
    differs = 0
    for b in range(PLANT_B):
        run = slice(b * PLANT_RUN, (b + 1) * PLANT_RUN)
        differs += int(torch.argsort(s8[b, run], descending=True).tolist()
                       != torch.argsort(exact[b, run], descending=True).tolist())
    print("queries whose int8 order of the planted run differs:", differs)
    assert differs >= 1


def q8_search_ref(q, c, case, b0=0):
    codes, meta = quantise_ref(c)
    if case.labels is None:
        return ops.cosine_topk_q8_ref(q, c, codes, meta, case.k, case.n)
    labels, want = ta._labels_want(case, c.shape[0], b0, q.shape[0])
    return ops.cosine_topk_q8_ref(q, c, codes, meta, case.k, case.n, labels, want)


def test_two_stage_ref_planted(planted):
    case, c, codes, meta = planted
    scores, idx = ops.cosine_topk_q8_ref(case.q, c, codes, meta, case.k, case.n)
    ta.judge(case, scores, idx, case.q.double() @ c.double().t())


def test_two_stage_ref_families(base):
    pc = ta.plan_constants()
    u, neg = ta.negative_corpus(D, N, seed=40)
    cases = [
        ta.dup_case(D, N, 4, 5, 9, "scattered", pc, 910),
        ta.dup_case(D, N, 4, 8, 24, "contig", pc, 911),
        ta.dup_case(D, N, 4, 8, 14, "scattered", pc, 912, filtered_half=True),
        ta.neardup_case(D, N, 4, pc, 913),
        ta.negative_case(u, neg, N, 4, 5, 914),
        ta.poison_case(D, N, 4, 5, 915),
        ta.zero_query_case(D, N, 4, 8, 916),
    ]
    for case in cases:
        ta.run_case(case, base, q8_search_ref)


def test_two_stage_ref_flooded_falls_back(base):
    before = ops.q8_overflow_fallbacks
    ta.run_case(ta.flooded_case(D, N, 4, 8, 920), base, q8_search_ref)
    assert ops.q8_overflow_fallbacks == before + 1


def test_out_of_plan_is_the_plain_search(base):
    q = ta.rand_unit(9, D, 930)
    c = base[:4096]
    codes, meta = quantise_ref(c)
    for qq, cc, k in ((q, c, 5), (q[:4], c, 5)):
        got = ops.cosine_topk_q8(qq, cc, codes, meta, k)
        ref = ops.cosine_topk_ref(qq, cc, k)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert not ops.q8_in_plan(9, N, 5, False) and not ops.q8_in_plan(8, 4096, 5, False)
    assert not ops.q8_in_plan(8, N, 1, False) and ops.q8_in_plan(8, N, 1, True)
    assert ops.q8_in_plan(8, 65536, 2, False)


# ---------------------------------------------------------------------------
# store, engine, config
# ---------------------------------------------------------------------------

def _unit_rows(n, seed):
    return ta.rand_unit(n, D, seed).float()


def test_store_mirror_follows_the_rows():
    store = EmbeddingStore(D, device="cpu", capacity=256, segment_rows=2048, int8_mirror=True)
    rows = _unit_rows(5000, 940)
    labels = (torch.arange(5000) % 3).to(torch.int32)
    done = 0
    for n in (100, 300, 1500, 700, 2400):  # doubles in place, then crosses into segments 2 and 3
        store.append(rows[done : done + n], labels[done : done + n])
        done += n
    assert store.count == 5000 and store.n_segments == 3
    for lo, hi in ((0, 5000), (2000, 2100), (4090, 4100)):
        codes, meta = store.mirror_range(lo, hi)
        want_c, want_m = quantise_ref(store.row_range(lo, hi))
        assert torch.equal(codes, want_c) and torch.equal(meta, want_m)

    plain = EmbeddingStore(D, device="cpu", capacity=256, segment_rows=2048)
    plain.append(rows, labels)
    assert plain._codes == [] and plain._meta == [] and not plain.int8_mirror
    with pytest.raises(RuntimeError):
        plain.mirror_range(0, 10)
    q = rows[[5, 2500, 4999]] + 0.01 * _unit_rows(3, 941)
    want = torch.tensor([0, -1, 2], dtype=torch.int32)
    for kw in ({}, {"want": want}, {"valid_n": 1000}):
        a, b = store.search(q, 5, **kw), plain.search(q, 5, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    # enable_mirror on a filled store gives the same mirror
    plain.enable_mirror()
    for x, y in zip(plain.mirror_range(0, 5000), store.mirror_range(0, 5000)):
        assert torch.equal(x, y)

    fresh = _unit_rows(300, 942)
    store.adopt(fresh)
    codes, meta = store.mirror_range(0, 300)
    want_c, want_m = quantise_ref(fresh)
    assert store.count == 300 and torch.equal(codes, want_c) and torch.equal(meta, want_m)
    assert store._codes[0].shape[0] == 300


def test_store_search_takes_the_mirror_when_in_plan(monkeypatch):
    store = EmbeddingStore(D, device="cpu", capacity=1024, segment_rows=1 << 17, int8_mirror=True)
    store.append(ta.rand_unit(N, D, seed=1).float())
    calls = []
    real = ops.cosine_topk_q8

    def spy(*a, **kw):
        calls.append(a[0].shape[0])
        return real(*a, **kw)

    monkeypatch.setattr(ops, "cosine_topk_q8", spy)
    q = store.row_range(10, 14).clone()
    s, i = store.search(q, 5)
    assert i[:, 0].tolist() == [10, 11, 12, 13]
    store.search(_unit_rows(ops.Q8_MAX_B + 1, 950), 5)
    assert calls == ([4] if ops.Q8_MAX_B >= 4 else [])


def test_engine_and_config_defaults(tmp_path):
    import yaml

    from kakveda_amd.core.config import DEFAULT_CONFIG

    assert DEFAULT_CONFIG["gfkb"]["int8_mirror"] is False
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shipped = yaml.safe_load(open(os.path.join(repo, "config", "config.yaml")))
    assert shipped["gfkb"]["int8_mirror"] is False

    eng = GfkbEngine(data_dir=str(tmp_path / "off"), dim=D, hash_dim=4096)
    assert not eng.store.int8_mirror and eng.store._codes == []


def test_engine_mirror_reaches_the_store_and_survives_restart(tmp_path):
    def sig(i):
        return "intent_tags:t%d | prompt_hint:case number %d | tools: | env_keys:" % (i % 5, i)

    eng = GfkbEngine(data_dir=str(tmp_path), dim=D, hash_dim=4096, int8_mirror=True)
    assert eng.store.int8_mirror
    for i in range(30):
        eng.upsert_failure("T%d" % (i % 2), sig(i), {}, app_id="a")
    want_c, want_m = quantise_ref(eng.store.row_range(0, 30))
    codes, meta = eng.store.mirror_range(0, 30)
    assert torch.equal(codes, want_c) and torch.equal(meta, want_m)
    first = eng.match(sig(7))

    again = GfkbEngine(data_dir=str(tmp_path), dim=D, hash_dim=4096, int8_mirror=True)
    assert again.store.count == 30 and again.store.int8_mirror
    codes2, meta2 = again.store.mirror_range(0, 30)
    assert torch.equal(codes2, want_c) and torch.equal(meta2, want_m)
    assert [m.failure_id for m in again.match(sig(7))] == [m.failure_id for m in first]

    class NotAStore:
        def append(self, rows):
            return 0

    with pytest.raises(NotImplementedError, match="int8_mirror"):
        again.attach_store(NotAStore())
    swapped = EmbeddingStore(D, device="cpu")
    again.attach_store(swapped)
    assert swapped.int8_mirror and swapped.count == 30


def test_service_applies_the_config_flag(tmp_path):
    from kakveda_amd.services.gfkb_service import create_app

    class Config:
        def __init__(self, values):
            self.values = values

        def get(self, key, default=None):
            return self.values.get(key, default)

    off = GfkbEngine(data_dir=str(tmp_path / "a"), dim=D, hash_dim=4096)
    create_app(engine=off, config=Config({}))
    assert not off.store.int8_mirror
    on = GfkbEngine(data_dir=str(tmp_path / "b"), dim=D, hash_dim=4096)
    on.upsert_failure("T", "intent_tags:x | prompt_hint:one | tools: | env_keys:", {}, app_id="a")
    create_app(engine=on, config=Config({"gfkb.int8_mirror": True}))
    assert on.int8_mirror and on.store.int8_mirror
    want_c, _ = quantise_ref(on.store.row_range(0, 1))
    assert torch.equal(on.store.mirror_range(0, 1)[0], want_c)
