"""CPU side of the wide top-k (8 < k <= 64): the op's reference path, the
``top_k`` field of /failures/match, and the batcher's two-call split."""

import threading

import pytest
import torch

from kakveda_amd import ops
from kakveda_amd.gfkb.engine import EmbeddingStore, GfkbEngine
from kakveda_amd.services.gfkb_service import MatchBatcher

import topk_adversarial as ta


def test_kwide_max_exported():
    assert ops.KWIDE_MAX == 64 and ops.KMAX == 8
    assert ops.wide_overflow_fallbacks >= 0


@pytest.mark.parametrize("k", [9, 20, 64, 70])
def test_cosine_topk_wide_cpu_is_the_reference(k):
    d, n = 64, 300
    c = ta.rand_unit(n, d, 1)
    q = ta.rand_unit(5, d, 2)
    s, i = ops.cosine_topk_wide(q, c, k)
    rs, ri = ops.cosine_topk_ref(q, c, k, n)
    assert s.shape == (5, k) and i.dtype == torch.int64 and s.dtype == torch.float32
    assert torch.equal(i, ri) and torch.equal(s, rs)
    ta.check_topk(s, i, q.double() @ c.double().t(), k, d, what="cpu wide k=%d" % k)


def test_cosine_topk_wide_cpu_pads_and_valid_n():
    d = 64
    c = ta.rand_unit(100, d, 3)
    q = ta.rand_unit(3, d, 4)
    s, i = ops.cosine_topk_wide(q, c, 64, valid_n=40)
    assert bool((i[:, :40] >= 0).all()) and bool((i[:, :40] < 40).all())
    assert bool((i[:, 40:] == -1).all()) and bool((s[:, 40:] == float("-inf")).all())
    ta.check_topk(s, i, q.double() @ c[:40].double().t(), 64, d, what="cpu wide valid_n")
    s0, i0 = ops.cosine_topk_wide(q, c, 20, valid_n=0)
    assert s0.shape == (3, 20) and bool((i0 == -1).all())


def test_cosine_topk_wide_cpu_filtered():
    d, n, k = 64, 400, 33
    c = ta.rand_unit(n, d, 5)
    q = ta.rand_unit(4, d, 6)
    labels = (torch.arange(n) % 10).to(torch.int32)
    labels[:30] = 77  # a label with 30 rows only
    want = torch.tensor([3, 77, -1, 12345], dtype=torch.int32)
    s, i = ops.cosine_topk_wide(q, c, k, labels=labels, want=want)
    rs, ri = ops.cosine_topk_filtered_ref(q, c, labels, want, k, n)
    assert torch.equal(i, ri) and torch.equal(s, rs)
    elig = (want[:, None].long() < 0) | (labels[None, :].long() == want[:, None].long())
    ta.check_topk(s, i, q.double() @ c.double().t(), k, d, eligible=elig, what="cpu wide filtered")
    assert int((i[1] >= 0).sum()) == 30 and int((i[3] >= 0).sum()) == 0
    with pytest.raises(ValueError):
        ops.cosine_topk_wide(q, c, k, labels=labels)


def test_store_search_wide_cpu_two_segments_and_no_raise():
    d = 64
    rows = ta.rand_unit(700, d, 7)
    q = ta.rand_unit(3, d, 8)
    store = EmbeddingStore(dim=d, device="cpu", capacity=512, segment_rows=512)
    store.append(rows[:500])
    store.append(rows[500:])
    s, i = store.search(q, 20)
    ta.check_topk(s, i, q.double() @ rows.double().t(), 20, d, what="cpu store wide")
    # an nprobe without an index raises at k <= 8; the wide search ignores it
    with pytest.raises(ValueError):
        store.search(q, 5, nprobe=4)
    s2, i2 = store.search(q, 20, nprobe=4)
    assert torch.equal(i2, i)


def _sig(i):
    return "intent_tags:intent:t%d | prompt_hint:probe number %d of the wide test | tools: | env_keys:e2e" % (i % 7, i)


def _engine(tmp_path, n=30):
    eng = GfkbEngine(data_dir=str(tmp_path), device="cpu", dim=256, hash_dim=4096)
    for i in range(n):
        eng.upsert_failure("TIMEOUT" if i % 3 == 0 else "HALLUCINATION_CITATION", _sig(i), {"i": i},
                           app_id="app-%d" % (i % 3))
    return eng


@pytest.mark.parametrize("batcher", ["1", "0"])
def test_failures_match_top_k_field(tmp_path, monkeypatch, batcher):
    from fastapi.testclient import TestClient

    from kakveda_amd.services.gfkb_service import create_app

    monkeypatch.setenv("KAKVEDA_MATCH_BATCHER", batcher)
    eng = _engine(tmp_path)
    app = create_app(engine=eng)
    assert (app.state.batcher is not None) == (batcher == "1")
    with TestClient(app) as client:
        r = client.post("/failures/match", json={"signature_text": _sig(3), "top_k": 12})
        assert r.status_code == 200
        got = r.json()["matches"]
        assert len(got) == 12
        want = eng.match(_sig(3), top_k=12)
        assert [m["failure_id"] for m in got] == [m.failure_id for m in want]
        scores = [m["score"] for m in got]
        assert scores == sorted(scores, reverse=True)
        # without the field: today's five
        r = client.post("/failures/match", json={"signature_text": _sig(3)})
        assert r.status_code == 200 and len(r.json()["matches"]) == 5
        assert [m["failure_id"] for m in r.json()["matches"]] == [m.failure_id for m in want[:5]]
        # filter-first with top_k: every failure of the type (10 TIMEOUTs of 30)
        r = client.post("/failures/match", json={
            "signature_text": _sig(3), "top_k": 20, "failure_type": "TIMEOUT", "filter_first": True})
        assert r.status_code == 200
        got = r.json()["matches"]
        assert len(got) == 10 and all(m["failure_type"] == "TIMEOUT" for m in got)
        # the reference's order without filter_first: cut to top_k, then the type
        r = client.post("/failures/match", json={
            "signature_text": _sig(3), "top_k": 12, "failure_type": "TIMEOUT"})
        assert [m["failure_id"] for m in r.json()["matches"]] == [
            m.failure_id for m in want if m.failure_type == "TIMEOUT"]
        for bad in (0, 65, -1):
            r = client.post("/failures/match", json={"signature_text": _sig(3), "top_k": bad})
            assert r.status_code == 422, (bad, r.status_code)


class _Match:
    def __init__(self, text, rank, failure_type):
        self.text, self.rank, self.failure_type = text, rank, failure_type

    def __eq__(self, other):
        return (self.text, self.rank, self.failure_type) == (other.text, other.rank, other.failure_type)

    def __repr__(self):
        return "M(%s,%d,%s)" % (self.text, self.rank, self.failure_type)


class _RecordingEngine:
    """Records every match_batch call; answers top_k (default 5) matches per
    text with alternating types, restricted to a type when one is given
    together with filter_first."""

    def __init__(self):
        self.calls = []
        self.gate = threading.Event()
        self.entered = threading.Event()

    def match_batch(self, texts, failure_types=None, **kw):
        self.calls.append({"texts": list(texts), "types": list(failure_types), "kw": dict(kw)})
        if len(self.calls) == 1:
            # hold the first call until the test has queued the mixed batch
            self.entered.set()
            assert self.gate.wait(timeout=30)
        k = kw.get("top_k") or 5
        first = kw.get("filter_first") or [False] * len(texts)
        out = []
        for t, ft, f in zip(texts, failure_types, first):
            if f and ft:
                out.append([_Match(t, j, ft) for j in range(k)])
            else:
                out.append([_Match(t, j, "A" if j % 2 == 0 else "B") for j in range(k)])
        return out


def test_batcher_two_call_split_and_per_request_cut():
    eng = _RecordingEngine()
    batcher = MatchBatcher(eng)
    reqs = [
        dict(signature_text="plain-0"),
        dict(signature_text="wide-20", top_k=20),
        dict(signature_text="plain-typed", failure_type="B"),
        dict(signature_text="wide-3", top_k=3),
        dict(signature_text="wide-7-typed", top_k=7, failure_type="A"),
        dict(signature_text="wide-6-first", top_k=6, failure_type="B", filter_first=True),
    ]
    results = {}

    def call(name, kw):
        results[name] = batcher.match(**kw)

    opener = threading.Thread(target=call, args=("opener", dict(signature_text="opener")))
    opener.start()
    assert eng.entered.wait(timeout=30)
    # the collector thread is inside the first call: everything queued now
    # forms the next batch
    threads = []
    for r in reqs:
        t = threading.Thread(target=call, args=(r["signature_text"], r))
        t.start()
        threads.append(t)
    for _ in range(3000):
        if batcher._q.qsize() == len(reqs):
            break
        threading.Event().wait(0.001)
    assert batcher._q.qsize() == len(reqs)
    eng.gate.set()
    opener.join(timeout=30)
    for t in threads:
        t.join(timeout=30)

    assert len(eng.calls) == 3  # the opener, then at most two for the mixed batch
    plain, wide = eng.calls[1], eng.calls[2]
    # requests without top_k: exactly the call made before the field existed
    assert sorted(plain["texts"]) == ["plain-0", "plain-typed"]
    assert plain["kw"] == {}
    assert plain["types"][plain["texts"].index("plain-typed")] == "B"
    # requests with it: one call at their largest top_k
    assert sorted(wide["texts"]) == ["wide-20", "wide-3", "wide-6-first", "wide-7-typed"]
    assert wide["kw"]["top_k"] == 20
    # only the filter-first request hands its type to the engine
    assert wide["types"][wide["texts"].index("wide-7-typed")] is None
    assert wide["types"][wide["texts"].index("wide-6-first")] == "B"
    assert wide["kw"]["filter_first"][wide["texts"].index("wide-6-first")] is True

    assert len(results["plain-0"]) == 5
    assert [m.rank for m in results["wide-20"]] == list(range(20))
    assert [m.rank for m in results["wide-3"]] == [0, 1, 2]
    # cut to 7 first (ranks 0..6), then drop the other type: the even ranks
    assert [m.rank for m in results["wide-7-typed"]] == [0, 2, 4, 6]
    assert all(m.failure_type == "A" for m in results["wide-7-typed"])
    assert [m.rank for m in results["wide-6-first"]] == list(range(6))
    assert all(m.failure_type == "B" for m in results["wide-6-first"])
    assert batcher.requests == 7 and batcher.batches == 3
