"""Label-filtered routed search on the CPU: the reference ops, the store's
opt-in routing with its exact fill and per-label row counts, the engine's
``route_filtered`` and the service's ``gfkb.routed.filtered`` flag."""

import httpx
import pytest
import torch
import yaml

from kakveda_amd import ops
from kakveda_amd.core.config import ConfigStore
from kakveda_amd.gfkb.engine import EmbeddingStore, GfkbEngine
from kakveda_amd.gfkb.ivf import IvfIndex

NEG_INF = float("-inf")


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _spy(monkeypatch, name):
    """Record the calls of ops.<name> and pass them through."""
    calls = []
    real = getattr(ops, name)

    def spy(*a, **kw):
        calls.append((a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(ops, name, spy)
    return calls


# -- reference ops ------------------------------------------------------------

@pytest.fixture(scope="module")
def random_index():
    """500 unit rows in 8 random lists with labels r % 5; never modified."""
    g = torch.Generator().manual_seed(0)
    n, d, L = 500, 32, 8
    rows = _unit(torch.randn(n, d, generator=g))
    q = _unit(torch.randn(12, d, generator=g))
    cen = _unit(torch.randn(L, d, generator=g))
    assign = torch.randint(0, L, (n,), generator=g)
    ids = torch.sort(assign, stable=True).indices.to(torch.int32)
    off = torch.zeros(L + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(assign, minlength=L), 0)
    labels = (torch.arange(n) % 5).to(torch.int32)
    return rows, q, cen, off, ids, labels


def test_ref_all_lists_probed_is_the_exact_filtered_search(random_index):
    rows, q, cen, off, ids, labels = random_index
    n = rows.shape[0]
    want = (torch.arange(12) % 6 - 1).to(torch.int32)  # -1, 0 .. 4
    s, i = ops.ivf_search_filtered_ref(q, rows, labels, want, cen, off, ids, 8, 5, n, n)
    es, ei = ops.cosine_topk_filtered_ref(q, rows, labels, want, 5)
    assert torch.allclose(s, es, atol=1e-6)
    sims = q @ rows.t()
    for b in range(12):
        if set(i[b].tolist()) != set(ei[b].tolist()):  # ties at the k-th score only
            for j in set(i[b].tolist()) ^ set(ei[b].tolist()):
                assert abs(float(sims[b, j]) - float(es[b, -1])) <= 1e-6
    # the public op on the CPU is the reference; labels as one tensor per segment too
    s2, i2 = ops.ivf_search_filtered(
        q, [rows[:200], rows[200:350], rows[350:]],
        [labels[:200], labels[200:350], labels[350:]], want, cen, off, ids, 8, 5, n, n,
    )
    assert torch.equal(i2, i) and torch.allclose(s2, s, atol=1e-6)


def test_ref_unfiltered_wants_equal_the_unfiltered_ref(random_index):
    rows, q, cen, off, ids, labels = random_index
    n = rows.shape[0]
    want = torch.full((12,), -1, dtype=torch.int32)
    for nprobe in (1, 3, 8):
        s, i = ops.ivf_search_filtered_ref(
            q, rows, labels, want, cen, off, ids, nprobe, 5, n - 20, n - 40
        )
        rs, ri = ops.ivf_search_ref(q, rows, cen, off, ids, nprobe, 5, n - 20, n - 40)
        assert torch.equal(s, rs) and torch.equal(i, ri)
    probes = torch.tensor([[0, 3, -1]] * 12)
    a = ops.ivf_scan_topk_filtered(q, rows, labels, want, off, ids, probes, 5, n, n, n)
    b = ops.ivf_scan_topk_ref(q, rows, off, ids, probes, 5, n, n, n)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_ref_label_no_row_has_pads_fully(random_index):
    rows, q, cen, off, ids, labels = random_index
    n = rows.shape[0]
    want = torch.tensor([9, -1] * 6, dtype=torch.int32)
    s, i = ops.ivf_search_filtered_ref(q, rows, labels, want, cen, off, ids, 8, 5, n, n)
    assert (i[0::2] == -1).all() and (s[0::2] == NEG_INF).all()
    assert (i[1::2] >= 0).all()
    # every returned id carries the wanted label
    want = torch.full((12,), 3, dtype=torch.int32)
    s, i = ops.ivf_search_filtered_ref(q, rows, labels, want, cen, off, ids, 2, 5, n, n)
    assert (labels[i[i >= 0]] == 3).all()


# -- store --------------------------------------------------------------------

D = 16
K = 5
COMMON, RARE_FAR, RARE_NEAR = 0, 1, 2


def _hand_store():
    """Four well-separated clusters of 10 rows around e0..e3, one inverted
    list per cluster. Label RARE_FAR sits on 6 rows of cluster 2 only, label
    RARE_NEAR on 2 rows of cluster 0 only; everything else is COMMON. A query
    near e0 probes list 0 alone at nprobe=1."""
    g = torch.Generator().manual_seed(1)
    eye = torch.eye(D)[:4]
    cluster = torch.arange(40) // 10
    rows = _unit(eye[cluster] + 0.05 * torch.randn(40, D, generator=g))
    labels = torch.full((40,), COMMON, dtype=torch.int32)
    labels[20:26] = RARE_FAR
    labels[3:5] = RARE_NEAR
    st = EmbeddingStore(D, device="cpu", capacity=64)
    st.append(rows, labels)
    st.index = IvfIndex(
        centroids=eye.clone(), offsets=torch.arange(0, 41, 10, dtype=torch.int64),
        ids=torch.arange(40, dtype=torch.int32), n_indexed=40, n_lists=4, max_list_len=10,
    )
    st.index.validate()
    q = _unit(eye[:1] + 0.05 * torch.randn(3, D, generator=g))
    return st, q


def test_store_routes_a_filtered_batch_only_when_asked(monkeypatch):
    st, q = _hand_store()
    want = torch.tensor([COMMON, -1, COMMON], dtype=torch.int32)
    routed = _spy(monkeypatch, "ivf_search_filtered")
    unfiltered = _spy(monkeypatch, "ivf_search")
    exact = _spy(monkeypatch, "cosine_topk_filtered")
    # the default is unchanged: exact filtered, whatever nprobe says
    es, ei = st.search(q, K, want=want, nprobe=1)
    assert len(exact) == 1 and not routed
    s, i = st.search(q, K, want=want, nprobe=1, route_filtered=True)
    assert len(routed) == 1 and len(exact) == 1 and not unfiltered
    # list 0 holds 8 COMMON rows: enough, and they are the exact answer
    assert torch.equal(i, ei) and torch.allclose(s, es, atol=1e-6)
    assert (i < 10).all() and st.exact_fills == 0
    # without nprobe the flag does nothing; without an index nprobe still raises
    st.search(q, K, want=want, route_filtered=True)
    assert len(routed) == 1 and len(exact) == 2
    st.index = None
    with pytest.raises(ValueError, match="index"):
        st.search(q, K, want=want, nprobe=1, route_filtered=True)


def test_store_exact_fill(monkeypatch):
    st, q = _hand_store()
    want = torch.tensor([RARE_FAR, RARE_NEAR, -1], dtype=torch.int32)
    es, ei = st.search(q, K, want=want)  # the exact filtered answer
    assert (ei[0] >= 20).all() and (ei[0] < 26).all()
    exact = _spy(monkeypatch, "cosine_topk_filtered")

    # fill off: the label's 6 rows all sit in list 2, which q does not probe
    s, i = st.search(q, K, want=want, nprobe=1, route_filtered=True, fill_exact=False)
    assert (i[0] == -1).all() and (s[0] == NEG_INF).all()
    assert not exact

    # fill on (the default): the short query alone is run again, exactly
    s, i = st.search(q, K, want=want, nprobe=1, route_filtered=True)
    assert torch.equal(i, ei) and torch.allclose(s, es, atol=1e-6)
    assert len(exact) == 1 and st.exact_fills == 1
    (fq, _seg, _lab, fw, fk), fkw = exact[0]
    assert fq.shape == (1, D) and torch.equal(fq, q[:1])
    assert fw.tolist() == [RARE_FAR] and fk == K
    # the 2-row label, both rows found in the probed list: no re-run for it
    assert sorted(i[1, :2].tolist()) == [3, 4] and (i[1, 2:] == -1).all()
    # the unfiltered query rode along: list 0's rows
    assert (i[2] >= 0).all() and (i[2] < 10).all()

    # every list probed needs no fill at all
    del exact[:]
    s, i = st.search(q, K, want=want, nprobe=4, route_filtered=True)
    assert not exact and torch.equal(i, ei)


def test_store_keeps_a_sparse_all_filtered_batch_on_the_per_query_scan(monkeypatch):
    st, q = _hand_store()
    # RARE_FAR has 6 of 40 rows, RARE_NEAR 2, COMMON 32: call 15% sparse here
    monkeypatch.setattr(ops, "IVF_FILTERED_SPARSE_SHARE", 0.15)
    routed = _spy(monkeypatch, "ivf_search_filtered")

    def chosen(want, **kw):
        del routed[:]
        st.search(q, K, want=torch.tensor(want, dtype=torch.int32), nprobe=1,
                  route_filtered=True, **kw)
        return routed[0][1]["batched"]

    assert chosen([RARE_FAR, RARE_NEAR, RARE_FAR]) is False
    # one unfiltered query, or one dense label, and the batch size decides again
    assert chosen([RARE_FAR, -1, RARE_FAR]) is None
    assert chosen([RARE_FAR, COMMON, RARE_NEAR]) is None
    # the caller's choice is never overridden
    assert chosen([RARE_FAR, RARE_NEAR, RARE_FAR], batched=True) is True
    # from IVF_FILTERED_SPARSE_MIN_B queries on the list-major scan wins again
    monkeypatch.setattr(ops, "IVF_FILTERED_SPARSE_MIN_B", 3)
    assert chosen([RARE_FAR, RARE_NEAR, RARE_FAR]) is None
    assert 0 < ops.IVF_FILTERED_SPARSE_SHARE < 1


def test_store_fill_ignores_a_stale_count():
    # rows appended after the valid_n snapshot inflate the count: that can only
    # ask for an exact re-run, whose answer is the same
    st, q = _hand_store()
    want = torch.tensor([RARE_NEAR], dtype=torch.int32)
    snap = st.count
    st.append(_unit(torch.ones(1, D)), torch.tensor([RARE_NEAR], dtype=torch.int32))
    s, i = st.search(q[:1], K, valid_n=snap, want=want, nprobe=1, route_filtered=True)
    assert sorted(i[0, :2].tolist()) == [3, 4] and (i[0, 2:] == -1).all()
    assert st.exact_fills == 1


def test_label_counts_follow_append_and_adopt():
    st = EmbeddingStore(4, device="cpu", capacity=4, segment_rows=8)
    g = torch.Generator().manual_seed(2)
    rows = _unit(torch.randn(21, 4, generator=g))
    labels = (torch.arange(21) % 3).to(torch.int32)
    st.append(rows[:6], labels[:6])      # grows the first segment
    st.append(rows[6:19], labels[6:19])  # crosses into later segments
    st.append(rows[19:])                 # unlabelled
    assert st.n_segments > 1 and st.count == 21
    assert [st.label_rows(v) for v in (0, 1, 2)] == [7, 6, 6]
    assert st.label_rows(-1) == 2 and st.label_rows(5) == 0
    stored = st.label_range(0, 21)
    for v in (-1, 0, 1, 2):
        assert st.label_rows(v) == int((stored == v).sum())
    st.adopt(rows[:10].clone(), torch.tensor([4] * 7 + [9] * 3))
    assert st.label_rows(4) == 7 and st.label_rows(9) == 3 and st.label_rows(0) == 0
    st.adopt(rows[:5].clone())
    assert st.label_rows(-1) == 5 and st.label_rows(4) == 0


# -- engine -------------------------------------------------------------------

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


QUERIES = [_sig(f"{t} again") for t in TOPICS]


def _engine(path, **kw):
    eng = GfkbEngine(data_dir=str(path), device="cpu", dim=256, hash_dim=4096, **kw)
    for t, topic in enumerate(TOPICS):
        for i in range(12):
            eng.upsert_failure(f"TYPE_{t % 3}", _sig(f"{topic} v{i}"), {}, app_id="a")
    return eng


def _flat(results):
    return [[(m.failure_id, m.failure_type) for m in r] for r in results]


def test_engine_routed_filter_first_equals_exact(tmp_path, monkeypatch):
    eng = _engine(tmp_path)
    types = ["TYPE_1"] * 6
    exact = eng.match_batch(QUERIES, failure_types=types, filter_first=True)
    eng.build_index(n_lists=8)
    routed = _spy(monkeypatch, "ivf_search_filtered")
    got = eng.match_batch(
        QUERIES, failure_types=types, filter_first=True, nprobe=8, route_filtered=True
    )
    assert len(routed) == 1
    assert _flat(got) == _flat(exact)
    assert all(m.failure_type == "TYPE_1" for r in got for m in r)
    for r, e in zip(got, exact):
        assert [m.score for m in r] == pytest.approx([m.score for m in e], abs=1e-5)
    one = eng.match(QUERIES[0], "TYPE_1", filter_first=True, nprobe=8, route_filtered=True)
    assert _flat([one]) == _flat(exact[:1]) and len(routed) == 2
    # a narrow probe with the exact fill still returns top_k of the type
    narrow = eng.match_batch(
        QUERIES, failure_types=types, filter_first=True, nprobe=1, route_filtered=True
    )
    assert all(len(r) == 5 and all(m.failure_type == "TYPE_1" for m in r) for r in narrow)


def test_engine_mixed_batch_routes_once(tmp_path, monkeypatch):
    eng = _engine(tmp_path, nprobe=8, route_filtered=True)
    assert eng.route_filtered is True
    types = ["TYPE_0", None, "TYPE_2", "TYPE_1", None, "NEVER_SEEN"]
    first = [True, False, True, False, False, True]
    exact = eng.match_batch(QUERIES, failure_types=types, filter_first=first)
    eng.build_index(n_lists=8)
    routed = _spy(monkeypatch, "ivf_search_filtered")
    unfiltered = _spy(monkeypatch, "ivf_search")
    exact_f = _spy(monkeypatch, "cosine_topk_filtered")
    got = eng.match_batch(QUERIES, failure_types=types, filter_first=first)
    assert len(routed) == 1 and not unfiltered and not exact_f
    # one search for the five known queries; the unfiltered ones ride with -1
    (a, kw) = routed[0]
    assert a[0].shape[0] == 5
    assert a[3].tolist() == [eng._type_id["TYPE_0"], -1, eng._type_id["TYPE_2"], -1, -1]
    assert _flat(got) == _flat(exact)
    assert got[5] == []  # an unknown type still matches nothing
    assert eng.match(QUERIES[0], "NEVER_SEEN", filter_first=True) == []
    # nprobe=0 forces exact, as does an explicit route_filtered=False
    del routed[:]
    assert _flat(eng.match_batch(QUERIES, types, filter_first=first, nprobe=0)) == _flat(exact)
    assert _flat(
        eng.match_batch(QUERIES, types, filter_first=first, route_filtered=False)
    ) == _flat(exact)
    assert not routed and len(exact_f) == 2


def test_engine_unset_leaves_the_routed_filtered_op_uncalled(tmp_path, monkeypatch):
    eng = _engine(tmp_path, nprobe=2)
    assert eng.route_filtered is False
    eng.build_index(n_lists=8)
    routed = _spy(monkeypatch, "ivf_search_filtered")
    got = eng.match_batch(QUERIES, failure_types=["TYPE_1"] * 6, filter_first=True)
    assert not routed and all(len(r) == 5 for r in got)
    # and with no index the flag changes nothing either
    eng.store.index = None
    eng.route_filtered = True
    eng.match_batch(QUERIES, failure_types=["TYPE_1"] * 6, filter_first=True)
    assert not routed


def test_engine_refuses_on_stores_without_labels(tmp_path):
    from kakveda_amd.gfkb.dist_server import DistGfkbCoordinator, _CoordinatorStore

    eng = _engine(tmp_path)
    eng.attach_store(_CoordinatorStore(DistGfkbCoordinator(dim=256, capacity=128)))
    with pytest.raises(NotImplementedError, match="filter_first"):
        eng.match(QUERIES[0], "TYPE_1", filter_first=True, route_filtered=True)
    with pytest.raises(NotImplementedError, match="nprobe"):
        eng.match(QUERIES[0], nprobe=2, route_filtered=True)


# -- service ------------------------------------------------------------------

def _config(tmp_path, routed):
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump({"gfkb": {"routed": routed}}))
    return ConfigStore(str(path))


async def _post(client, **body):
    r = await client.post("/failures/match", json=body)
    assert r.status_code == 200
    return [(m["failure_id"], m["failure_type"]) for m in r.json()["matches"]]


@pytest.mark.parametrize("batcher", ["1", "0"])
async def test_service_filtered_flag_keeps_filter_first_routed(tmp_path, monkeypatch, batcher):
    from kakveda_amd.services.gfkb_service import create_app

    monkeypatch.setenv("KAKVEDA_MATCH_BATCHER", batcher)
    eng = _engine(tmp_path)
    before = _flat(
        eng.match_batch(QUERIES, failure_types=["TYPE_1"] * 6, filter_first=True)
    )
    cfg = _config(
        tmp_path,
        {"enabled": True, "n_lists": 8, "nprobe": 8, "min_rows": 16, "filtered": True},
    )
    app = create_app(engine=eng, config=cfg)
    assert eng.store.index is not None and eng.nprobe == 8 and eng.route_filtered is True
    routed = _spy(monkeypatch, "ivf_search_filtered")
    client = httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://gfkb")
    for q, want in zip(QUERIES, before):
        got = await _post(client, signature_text=q, failure_type="TYPE_1", filter_first=True)
        assert got == want
    assert len(routed) == len(QUERIES)
    # exact: true opts the request out of routing
    got = await _post(
        client, signature_text=QUERIES[0], failure_type="TYPE_1", filter_first=True, exact=True
    )
    assert got == before[0] and len(routed) == len(QUERIES)
    await client.aclose()


async def test_service_filtered_flag_defaults_to_off(tmp_path, monkeypatch):
    from kakveda_amd.services.gfkb_service import create_app

    eng = _engine(tmp_path)
    cfg = _config(tmp_path, {"enabled": True, "n_lists": 8, "nprobe": 8, "min_rows": 16})
    app = create_app(engine=eng, config=cfg)
    assert eng.store.index is not None and eng.route_filtered is False
    routed = _spy(monkeypatch, "ivf_search_filtered")
    client = httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://gfkb")
    got = await _post(client, signature_text=QUERIES[0], failure_type="TYPE_1", filter_first=True)
    assert len(got) == 5 and not routed
    await client.aclose()
