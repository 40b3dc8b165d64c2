"""Routed (IVF) matching above the store: GfkbEngine on CPU, the GFKB
service's ``gfkb.routed`` config block, the ``exact`` wire field, and the
stores that refuse."""

import httpx
import pytest
import torch
import yaml

from kakveda_amd.core.config import DEFAULT_CONFIG, ConfigStore
from kakveda_amd.gfkb.engine import GfkbEngine

TOPICS = [
    "summarize the quarterly sales report with references",
    "translate the onboarding manual into french",
    "plan a database migration with rollback steps",
    "debug a failing kubernetes deployment",
    "draft an incident postmortem for the outage",
    "classify support tickets by urgency",
]


def _sig(hint):
    return f"intent_tags:intent:citations_required | prompt_hint:{hint} | tools: | env_keys:e2e"


def _engine(path, **kw):
    return GfkbEngine(data_dir=str(path), device="cpu", dim=256, hash_dim=4096, **kw)


def _populate(eng, per_topic=12):
    for t, topic in enumerate(TOPICS):
        for i in range(per_topic):
            eng.upsert_failure(f"TYPE_{t % 3}", _sig(f"{topic} v{i}"), {}, app_id="a")


QUERIES = [_sig(f"{t} again") for t in TOPICS]


def _flat(results):
    return [[(m.failure_id, m.failure_type) for m in r] for r in results]


def _config(tmp_path, routed):
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump({"gfkb": {"routed": routed}}))
    return ConfigStore(str(path))


def test_defaults_keep_routing_off():
    assert DEFAULT_CONFIG["gfkb"]["routed"] == {
        "enabled": False,
        "n_lists": None,
        "nprobe": 32,
        "min_rows": 65536,
    }


# -- engine -----------------------------------------------------------------

def test_engine_routed_equals_exact_at_all_lists(tmp_path):
    eng = _engine(tmp_path)
    _populate(eng)
    exact = eng.match_batch(QUERIES)
    assert eng.store.index is None
    with pytest.raises(ValueError, match="index"):
        eng.match(QUERIES[0], nprobe=4)
    idx = eng.build_index(n_lists=8)
    assert eng.store.index is idx and idx.n_indexed == eng.store.count
    # building an index changes nothing until nprobe is asked for
    assert eng.match_batch(QUERIES) == exact
    routed = eng.match_batch(QUERIES, nprobe=8)
    assert _flat(routed) == _flat(exact)
    for r, e in zip(routed, exact):
        assert [m.score for m in r] == pytest.approx([m.score for m in e], abs=1e-5)
    assert _flat([eng.match(QUERIES[0], nprobe=8)]) == _flat(exact[:1])
    # a narrow probe still finds each topic's own cluster
    narrow = eng.match_batch(QUERIES, nprobe=2)
    assert [r[0].failure_id for r in narrow] == [e[0].failure_id for e in exact]
    # the post-filter on failure_type is applied to routed results too
    typed = eng.match_batch(QUERIES, failure_types=["TYPE_0"] * len(QUERIES), nprobe=8)
    assert all(m.failure_type == "TYPE_0" for r in typed for m in r)


def test_engine_default_nprobe_and_tail(tmp_path):
    eng = _engine(tmp_path, nprobe=1)
    _populate(eng)
    exact = eng.match_batch(QUERIES)  # no index yet: the default is ignored
    eng.build_index(n_lists=8)
    assert _flat(eng.match_batch(QUERIES, nprobe=0)) == _flat(exact)
    # an upsert after the build is matched on the very next (routed) search
    new = _sig("an entirely unrelated cooking recipe for pancakes")
    rec, created = eng.upsert_failure("NEW", new, {}, app_id="z")
    assert created and eng.store.count == eng.store.index.n_indexed + 1
    got = eng.match(new)  # engine default nprobe=1
    assert got[0].failure_id == rec["failure_id"] and got[0].score > 0.99


def test_engine_filter_first_batch_runs_exact_filtered(tmp_path, monkeypatch):
    from kakveda_amd import ops

    eng = _engine(tmp_path)
    _populate(eng)
    want = eng.match_batch(QUERIES, failure_types=["TYPE_1"] * 6, filter_first=True)
    eng.build_index(n_lists=8)

    def boom(*a, **kw):
        raise AssertionError("a filter-first batch must not be routed")

    monkeypatch.setattr(ops, "ivf_search", boom)
    got = eng.match_batch(
        QUERIES, failure_types=["TYPE_1"] * 6, filter_first=True, nprobe=1
    )
    assert got == want


# -- service ----------------------------------------------------------------

async def _post(client, **body):
    r = await client.post("/failures/match", json=body)
    assert r.status_code == 200
    return [(m["failure_id"], m["failure_type"]) for m in r.json()["matches"]]


@pytest.mark.parametrize("batcher", ["1", "0"])
async def test_service_config_off_changes_nothing(tmp_path, monkeypatch, batcher):
    from kakveda_amd.services.gfkb_service import create_app

    monkeypatch.setenv("KAKVEDA_MATCH_BATCHER", batcher)
    eng = _engine(tmp_path)
    _populate(eng)
    before = _flat(eng.match_batch(QUERIES))
    app = create_app(engine=eng, config=_config(tmp_path, {"enabled": False, "min_rows": 1}))
    assert eng.store.index is None and eng.nprobe is None
    calls = []
    real = eng.match_batch

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(eng, "match_batch", spy)
    client = httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://gfkb")
    for q, want in zip(QUERIES, before):
        assert await _post(client, signature_text=q) == want
    # the additive wire field is accepted and harmless without an index
    assert await _post(client, signature_text=QUERIES[0], exact=True) == before[0]
    await client.aclose()
    # routing off, nothing asks for exact: precisely the call of before
    assert all(kw.get("nprobe") is None for kw in calls[: len(QUERIES)])
    # default app (no config given) is off as well
    create_app(engine=eng)
    assert eng.store.index is None


@pytest.mark.parametrize("batcher", ["1", "0"])
async def test_service_config_on_equals_exact(tmp_path, monkeypatch, batcher):
    from kakveda_amd import ops
    from kakveda_amd.services.gfkb_service import create_app

    monkeypatch.setenv("KAKVEDA_MATCH_BATCHER", batcher)
    eng = _engine(tmp_path)
    _populate(eng)
    before = _flat(eng.match_batch(QUERIES))
    cfg = _config(tmp_path, {"enabled": True, "n_lists": 8, "nprobe": 8, "min_rows": 16})
    app = create_app(engine=eng, config=cfg)
    assert eng.store.index is not None and eng.store.index.n_lists == 8
    assert eng.nprobe == 8
    routed_calls = []
    real = ops.ivf_search

    def spy(*a, **kw):
        routed_calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "ivf_search", spy)
    client = httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://gfkb")
    for q, want in zip(QUERIES, before):
        assert await _post(client, signature_text=q) == want
    assert len(routed_calls) == len(QUERIES)
    # exact: true opts this request out of routing
    assert await _post(client, signature_text=QUERIES[0], exact=True) == before[0]
    assert len(routed_calls) == len(QUERIES)
    await client.aclose()


def test_service_below_min_rows_serves_exact(tmp_path):
    from kakveda_amd.services.gfkb_service import create_app

    eng = _engine(tmp_path)
    _populate(eng, per_topic=2)
    create_app(engine=eng, config=_config(tmp_path, {"enabled": True, "min_rows": 1000}))
    assert eng.store.index is None and eng.nprobe is None


def test_one_exact_request_makes_the_batch_exact(tmp_path, monkeypatch):
    from kakveda_amd.services.gfkb_service import MatchBatcher

    eng = _engine(tmp_path, nprobe=2)
    _populate(eng)
    eng.build_index(n_lists=8)
    calls = []
    real = eng.match_batch

    def spy(texts, types, **kw):
        calls.append((len(texts), kw))
        return real(texts, types, **kw)

    monkeypatch.setattr(eng, "match_batch", spy)
    batcher = MatchBatcher(eng)
    # drive one collected batch directly: three requests, one asks for exact
    import threading

    items = [
        {"text": q, "ftype": None, "first": False, "exact": e,
         "ev": threading.Event(), "res": None, "err": None}
        for q, e in zip(QUERIES[:3], (False, True, False))
    ]
    for it in items:
        batcher._q.put(it)
    batcher._ensure_thread()
    for it in items:
        assert it["ev"].wait(timeout=30.0)
        assert it["err"] is None and len(it["res"]) == 5
    exact_kw = [kw for n, kw in calls if kw.get("nprobe") == 0]
    # whichever way the collector cut the queue, the batch holding the
    # exact request ran exact as a whole
    assert exact_kw, calls
    assert sum(n for n, _ in calls) == 3
    # and a batch without one keeps the engine default (no nprobe passed)
    assert batcher.match(QUERIES[0])
    assert "nprobe" not in calls[-1][1]


# -- stores that refuse -----------------------------------------------------

def test_sharded_and_distributed_stores_refuse_nprobe(tmp_path):
    from kakveda_amd.gfkb.dist_server import DistGfkbCoordinator, _CoordinatorStore
    from kakveda_amd.parallel.sharded import ShardedStore

    g = torch.Generator().manual_seed(0)
    rows = torch.nn.functional.normalize(torch.randn(8, 16, generator=g), dim=1)
    sharded = ShardedStore(16, device="cpu")
    sharded.append(rows)
    with pytest.raises(NotImplementedError, match="routed"):
        sharded.search(rows[:1], 3, nprobe=2)
    assert sharded.search(rows[:1], 3)[1].shape == (1, 3)

    eng = _engine(tmp_path)
    _populate(eng, per_topic=2)
    coord_store = _CoordinatorStore(DistGfkbCoordinator(dim=256, capacity=64))
    with pytest.raises(NotImplementedError, match="routed"):
        coord_store.search(torch.zeros(1, 256), 3, nprobe=2)
    eng.attach_store(coord_store)
    assert len(eng.match(QUERIES[0])) == 5
    with pytest.raises(NotImplementedError, match="nprobe"):
        eng.match(QUERIES[0], nprobe=2)
    with pytest.raises(NotImplementedError, match="routed"):
        eng.build_index()
