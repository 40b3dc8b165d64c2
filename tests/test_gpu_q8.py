"""GPU tests of the int8 row mirror: the quantiser kernel against the torch
reference (codes and scales bit-equal), and the two-stage exact search
``ops.cosine_topk_q8`` (int8 scan + bf16 rescore) under the tie-aware float64
checker of tests/topk_adversarial.py.

Shapes are the smallest at which each loop can go wrong: N = 65,536 / 65,573
(the smallest corpus of the small-batch plan; a tail that is not a multiple
of a wave's 8 rows), D = 128 / 384 / 768 (1, 3 and 6 int8 segments: the
kernel's group of 2 and its remainder both run), B = 1 / 3 / 8, k = 2 / 5 / 8,
valid_n below the row count with poison beyond it. The planted input of
tests/q8_cases.py is the case a search without the error margin, or
without the rescore, fails.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_adversarial as ta  # noqa: E402
import q8_cases as qc  # noqa: E402

from kakveda_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_TAIL = 65_573
N_FLAT = 65_536
DIMS = (128, 384, 768)
_BASES = {}


def base_for(d):
    """65,700 unit rows per D, shared by the module and never modified."""
    if d not in _BASES:
        _BASES[d] = ta.rand_unit(ta.N_BASE, d, seed=1).to(DEV)
    return _BASES[d]


def mirror_of(c):
    codes, meta = ops.new_q8_mirror(c.shape[0], c.shape[1], c.device)
    ops.quantize_rows_q8(c, codes, meta, 0)
    return codes, meta


def search_q8(q, c, case, b0=0):
    codes, meta = mirror_of(c)
    if case.labels is None:
        return ops.cosine_topk_q8(q, c, codes, meta, case.k, valid_n=case.n)
    labels, want = ta._labels_want(case, c.shape[0], b0, q.shape[0])
    return ops.cosine_topk_q8(q, c, codes, meta, case.k, valid_n=case.n,
                              labels=labels.to(c.device), want=want.to(c.device))


# ---------------------------------------------------------------------------
# quantiser
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", DIMS)
def test_quantize_rows_matches_ref(d):
    for n in (1, 7, 8, 33, 4099):
        rows = qc.quantiser_rows(d, n, 20 + n)
        for first in (0, 5):
            codes, meta = ops.new_q8_mirror(n + first + 3, d, DEV)
            ops.quantize_rows_q8(rows.to(DEV), codes, meta, first)
            torch.cuda.synchronize()
            codes, meta = codes.cpu(), meta.cpu()
            want_c, want_m = qc.quantise_ref(rows)
            got_c, got_m = codes[first : first + n], meta[first : first + n]
            assert torch.equal(got_c, want_c), (d, n, first)
            assert torch.equal(got_m[:, 0], want_m[:, 0]), (d, n, first)
            qc.check_quantised(rows, got_c, got_m)
            # nothing outside [first, first + n) is written
            assert int(codes[:first].abs().sum()) == 0 and int(codes[first + n :].abs().sum()) == 0
            assert float(meta[:first].abs().sum()) == 0 and float(meta[first + n :].abs().sum()) == 0


# ---------------------------------------------------------------------------
# the search, shape by shape
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", DIMS)
def test_q8_search_shapes(d):
    base = base_for(d)
    poison = ta.poison_case(d, N_TAIL, 8, 8, 30 + d)
    c = ta.materialise(poison, base)  # N_TAIL live rows, 300 poisoned ones behind
    codes, meta = mirror_of(c)
    q8 = poison.q.to(DEV)
    sims_all = q8.double() @ c[:N_TAIL].double().t()
    E = ta.tolerance(d)
    for n in (N_FLAT, N_TAIL):
        sims = sims_all[:, :n]
        for B in (1, 3, 8):
            for k in (2, 5, 8):
                case = ta.Case(name="q8shape[D=%d,N=%d,B=%d,k=%d]" % (d, n, B, k),
                               q=poison.q[:B], n=n, k=k, idx_below=n)
                s, i = ops.cosine_topk_q8(q8[:B], c, codes, meta, k, valid_n=n)
                s0, i0 = ops.cosine_topk(q8[:B], c, k, valid_n=n)
                torch.cuda.synchronize()
                ta.judge(case, s, i, sims[:B])
                ta.judge(case, s0, i0, sims[:B])
                top = torch.topk(sims[:B], k + 1, dim=1).values
                clear = (top[:, k - 1] - top[:, k]) > E
                same = i.sort(dim=1).values == i0.sort(dim=1).values
                assert bool(same[clear].all()), case.name
                # stage 2 repeats the streaming kernel's arithmetic: measured
                # bit-equal at every shape here (profiles/q8_mirror.md)
                assert torch.equal(s, s0), case.name


def test_q8_planted_input():
    case = qc.planted_q8_case()
    ta.run_case(case, base_for(qc.D), search_q8)


def test_q8_adversarial_families():
    d = 384
    base, pc, n = base_for(d), ta.plan_constants(), ta.N_BASE
    u, neg = ta.negative_corpus(d, n, seed=40)
    cases = [
        ta.dup_case(d, n, 8, 5, 9, "scattered", pc, 1010),
        ta.dup_case(d, n, 1, 8, 24, "contig", pc, 1011),
        ta.dup_case(d, n, 3, 8, 8, "scattered", pc, 1012),
        ta.dup_case(d, n, 4, 8, 14, "scattered", pc, 1013, filtered_half=True),
        ta.neardup_case(d, n, 4, pc, 1014),
        ta.negative_case(u, neg.to(DEV), n, 4, 5, 1016),
    ]
    before = ops.q8_overflow_fallbacks
    for case in cases:
        ta.run_case(case, base, search_q8)
    assert ops.q8_overflow_fallbacks == before
    # an all-zero query scores 0 against every row and its floor is 0: every
    # row is a candidate under either scan, so this batch is a fallback
    ta.run_case(ta.zero_query_case(d, n, 4, 8, 1015), base, search_q8)
    assert ops.q8_overflow_fallbacks == before + 1


def test_q8_flooded_corpus_falls_back():
    d = 128
    before = ops.q8_overflow_fallbacks
    ta.run_case(ta.flooded_case(d, ta.N_BASE, 4, 8, 1020), base_for(d), search_q8)
    assert ops.q8_overflow_fallbacks == before + 1
    filt = ta.flooded_case(d, ta.N_BASE, 2, 5, 1021)
    filt.labels = torch.zeros(ta.N_BASE, dtype=torch.int32)
    filt.want = torch.tensor([0, -1], dtype=torch.int32)
    ta.run_case(filt, base_for(d), search_q8)
    assert ops.q8_overflow_fallbacks == before + 2


def test_q8_filtered():
    d, n, k = 384, N_TAIL, 5
    c = base_for(d)[:n]
    codes, meta = mirror_of(c)
    r = torch.arange(n)
    labels = (r % 2).to(torch.int32)  # 0 and 1: 50% each
    labels[r % 100 == 0] = 2  # 1%
    labels[torch.tensor([5, 40_000, n - 1])] = 4  # fewer than k rows; nobody carries 3
    want = torch.tensor([0, 2, 3, -1, 1, 4, -1, 2], dtype=torch.int32)
    q = ta.rand_unit(8, d, 1030)
    q[1] = c[300].cpu()  # a label-2 row's own query
    q[4] = c[300].cpu()  # the same row is ineligible for label 1
    case = ta.Case(name="q8filtered", q=q, n=n, k=k, labels=labels, want=want)
    lab_d, want_d, q_d = labels.to(DEV), want.to(DEV), q.to(DEV)
    s, i = ops.cosine_topk_q8(q_d, c, codes, meta, k, valid_n=n, labels=lab_d, want=want_d)
    s0, i0 = ops.cosine_topk_filtered(q_d, c, lab_d, want_d, k, valid_n=n)
    torch.cuda.synchronize()
    ta.judge(case, s, i, q_d.double() @ c.double().t(), ta.eligibility(case, DEV))
    assert i[1, 0].item() == 300 and 300 not in i[4].tolist()
    assert bool((i[2] == -1).all()) and int((i[5] >= 0).sum()) == 3
    assert torch.equal(i < 0, i0 < 0) and torch.equal(s[i < 0], s0[i0 < 0])
    # B = 1, filtered k = 1: the filtered table keeps k = 1 on the streaming kernel
    s1, i1 = ops.cosine_topk_q8(q_d[1:2], c, codes, meta, 1, valid_n=n, labels=lab_d,
                                want=want_d[1:2])
    assert i1.tolist() == [[300]]


def test_q8_out_of_plan_is_the_bf16_search():
    d = 128
    c = base_for(d)
    codes, meta = mirror_of(c)
    q = ta.rand_unit(9, d, 1040).to(DEV)
    for qq, n, k in ((q, ta.N_BASE, 5), (q[:4], 4096, 5), (q[:4], ta.N_BASE, 1)):
        got = ops.cosine_topk_q8(qq, c, codes, meta, k, valid_n=n)
        ref = ops.cosine_topk(qq, c, k, valid_n=n)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (qq.shape[0], n, k)
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.cosine_topk_q8(q[:, :64].contiguous(), c[:, :64].contiguous(), codes, meta, 5)


def test_q8_store_two_segments():
    from kakveda_amd.gfkb.engine import EmbeddingStore

    d, seg_rows = 128, 65_792
    rows = torch.cat([base_for(d), ta.rand_unit(seg_rows, d, seed=2).to(DEV)])[: 2 * seg_rows - 100]
    store = EmbeddingStore(d, device="cuda", capacity=seg_rows, segment_rows=seg_rows, int8_mirror=True)
    plain = EmbeddingStore(d, device="cuda", capacity=8, segment_rows=seg_rows)
    q = ta.rand_unit(4, d, 1050)
    q_d = q.to(DEV)
    k = 5

    def check(count, name):
        s, i = store.search(q_d, k)
        torch.cuda.synchronize()
        sims = q_d.double() @ store.row_range(0, count).double().t()
        ta.judge(ta.Case(name=name, q=q, n=count, k=k), s.float(), i, sims)
        return i

    done = 0
    for n in (seg_rows + 10, 30_000, rows.shape[0] - seg_rows - 30_010):
        store.append(rows[done : done + n])
        done += n
        check(done, "q8store[count=%d]" % done)
    assert store.n_segments == 2 and store.count == rows.shape[0]
    codes, meta = store.mirror_range(seg_rows - 5, seg_rows + 5)
    want_c, want_m = qc.quantise_ref(store.row_range(seg_rows - 5, seg_rows + 5).cpu())
    assert torch.equal(codes.cpu(), want_c) and torch.equal(meta.cpu()[:, 0], want_m[:, 0])
    assert plain._codes == []
    # a near-duplicate of query 2, appended now, is the next search's best match
    near = ta.near_rows(q[2:3], torch.Generator().manual_seed(1051), [0.99])[0].to(DEV)
    first = store.append(near)
    i = check(store.count, "q8store[after the near-duplicate]")
    assert i[2, 0].item() == first
