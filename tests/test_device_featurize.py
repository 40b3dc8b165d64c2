"""The device featurizer's plumbing, without a GPU: packing, the reference
op and its status rules, the constants' mirror, the encoder's fallback rule
and the engine/config wiring. (The kernel itself: tests/test_gpu_featurize.py;
its serial C++ statement: tests/test_featurize_plan.py.)"""

import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featurize_cases as fc  # noqa: E402

from kakveda_amd import ops  # noqa: E402
from kakveda_amd.encoder.featurizer import featurize_batch, pack_texts  # noqa: E402
from kakveda_amd.encoder.model import TraceEncoder  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NON_ASCII = "caf\u00e9 \u212aelvin"  # U+212A KELVIN SIGN lower-cases to 'k'
OVER_LONG = "long " * 300  # 1500 bytes


def _mixed_batch(hash_dim, max_features):
    """Texts the device takes, plus one of each kind it hands back."""
    texts = [t for _n, t in fc.edge_texts()] + fc.random_texts(40)
    special = {
        3: NON_ASCII,
        10: OVER_LONG,
        17: fc.with_features(max_features + 1, hash_dim),
        25: " ".join(["ab", "cd"] * 70),  # 140 tokens: too many grams
    }
    for i, t in special.items():
        texts[i] = t
    return texts


def test_pack_texts_offsets_and_host_rows():
    texts = ["abc", "", NON_ASCII, "de", OVER_LONG, "x" * ops.FEATURIZE_MAX_BYTES, "f"]
    buf, offsets, host_rows = pack_texts(texts)
    assert buf.dtype == np.uint8 and offsets.dtype == np.int32
    assert host_rows == [2, 4]
    lens = [3, 0, 0, 2, 0, ops.FEATURIZE_MAX_BYTES, 1]
    assert offsets.tolist() == [0] + np.cumsum(lens).tolist()
    assert buf.tobytes() == ("abc" + "de" + "x" * ops.FEATURIZE_MAX_BYTES + "f").encode()
    # the caller's list is not touched
    assert texts[2] == NON_ASCII and texts[4] == OVER_LONG

    buf, offsets, host_rows = pack_texts([])
    assert buf.shape == (0,) and offsets.tolist() == [0] and host_rows == []
    buf, offsets, host_rows = pack_texts(("", ""))
    assert buf.shape == (0,) and offsets.tolist() == [0, 0, 0] and host_rows == []


def test_reference_op_equals_featurize_batch():
    texts = [t for _n, t in fc.edge_texts()] + fc.random_texts(64)
    buf, offsets = fc.pack(texts)
    for hash_dim, seed, mf in ((8, 0, 8), (64, 3, 64), (1000, 0, 128), (65536, 11, 64)):
        idx, w, status, flagged = ops.featurize_bytes(
            torch.from_numpy(buf), torch.from_numpy(offsets), hash_dim, seed, mf
        )
        assert idx.dtype == torch.int32 and w.dtype == torch.float32
        assert status.dtype == torch.int32 and flagged.shape == (1,)
        want_status = [fc.expected_status(t, hash_dim, seed, mf) for t in texts]
        assert status.tolist() == want_status
        assert int(flagged) == sum(s != 0 for s in want_status)
        ridx, rw = featurize_batch(texts, hash_dim=hash_dim, seed=seed, max_features=mf)
        for b, s in enumerate(want_status):
            if s == 0:
                assert np.array_equal(idx[b].numpy(), ridx[b]), (hash_dim, b)
                assert np.array_equal(w[b].numpy(), rw[b]), (hash_dim, b)
            else:  # a flagged row is all zeros
                assert not idx[b].any() and not w[b].any()


def test_status_rules():
    def status_of(text, hash_dim=65536, mf=64):
        buf, offsets = fc.pack([text])
        out = ops.featurize_bytes_ref(
            torch.from_numpy(buf), torch.from_numpy(offsets), hash_dim, 0, mf
        )
        return int(out[2][0]), int(out[3])

    assert status_of("") == (0, 0)
    assert status_of("x" * ops.FEATURIZE_MAX_BYTES) == (0, 0)
    assert status_of("x" * (ops.FEATURIZE_MAX_BYTES + 1)) == (1, 1)
    # 128 tokens are 255 grams and fit; 129 are 257 and do not, however
    # few of them are distinct
    assert status_of(" ".join(["r"] * 128)) == (0, 0)
    assert status_of(" ".join(["r"] * 129)) == (1, 1)
    # capacity is checked before the feature count
    assert status_of(" ".join("k%d" % i for i in range(129)), mf=8) == (1, 1)
    assert status_of(fc.with_features(64, 65536), mf=64) == (0, 0)
    assert status_of(fc.with_features(65, 65536), mf=64) == (2, 1)
    # bytes >= 0x80 separate tokens
    raw = np.frombuffer(bytearray(b"ab\xc3\xa9cd \xffx"), dtype=np.uint8)
    off = np.array([0, len(raw)], dtype=np.int32)
    idx, w, _s, _f = ops.featurize_bytes_ref(
        torch.from_numpy(raw), torch.from_numpy(off), 65536, 0, 64
    )
    ridx, rw = featurize_batch(["ab  cd  x"], hash_dim=65536, seed=0, max_features=64)
    assert np.array_equal(idx[0].numpy(), ridx[0]) and np.array_equal(w[0].numpy(), rw[0])


def test_constants_mirror_the_header():
    header = open(
        os.path.join(REPO, "kakveda_amd", "ops", "hip", "featurize_plan.h")
    ).read()

    def const(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, header).group(1))

    assert ops.FEATURIZE_MAX_BYTES == const("FEATURIZE_MAX_BYTES")
    assert ops.FEATURIZE_MAX_GRAMS == const("FEATURIZE_MAX_GRAMS")
    assert ops.FEATURIZE_OK == const("FEATURIZE_OK")
    assert ops.FEATURIZE_TOO_MANY_GRAMS == const("FEATURIZE_TOO_MANY_GRAMS")
    assert ops.FEATURIZE_TOO_MANY_FEATURES == const("FEATURIZE_TOO_MANY_FEATURES")
    assert const("FEATURIZE_MAX_FEATURES") == 128  # embedding_bag's L limit


def test_encoder_flag_is_bit_identical_on_cpu():
    hash_dim, mf = 4096, 32
    texts = _mixed_batch(hash_dim, mf)
    off = TraceEncoder(dim=64, hash_dim=hash_dim, device="cpu", max_features=mf)
    on = TraceEncoder(
        dim=64, hash_dim=hash_dim, device="cpu", max_features=mf, device_featurize=True
    )
    assert off.device_featurize is False and off.host_fallbacks == 0
    want = off.encode_texts(texts)
    got = on.encode_texts(texts)
    assert torch.equal(got, want)
    # exactly the rows the device cannot take went back to the host
    expect = sum(
        (not t.isascii())
        or len(t) > ops.FEATURIZE_MAX_BYTES
        or fc.expected_status(t, hash_dim, 0, mf) != 0
        for t in texts
    )
    assert expect >= 4
    assert on.host_fallbacks == expect and off.host_fallbacks == 0

    # a clean batch falls back nowhere; a second call keeps counting
    clean = fc.signature_texts(32)
    on2 = TraceEncoder(dim=64, hash_dim=65536, device="cpu", device_featurize=True)
    off2 = TraceEncoder(dim=64, hash_dim=65536, device="cpu")
    assert torch.equal(on2.encode_texts(clean), off2.encode_texts(clean))
    assert on2.host_fallbacks == 0
    assert torch.equal(on2.encode_texts([NON_ASCII]), off2.encode_texts([NON_ASCII]))
    assert on2.host_fallbacks == 1
    assert torch.equal(on2.encode_text("one text"), off2.encode_text("one text"))
    assert on2.encode_texts([]).shape == (0, 64)


def test_engine_and_config_reach_the_encoder(tmp_path):
    from kakveda_amd.core.config import DEFAULT_CONFIG, ConfigStore
    from kakveda_amd.gfkb.engine import GfkbEngine
    from kakveda_amd.services.gfkb_service import create_app

    assert DEFAULT_CONFIG["gfkb"]["device_featurize"] is False
    shipped = ConfigStore(os.path.join(REPO, "config", "config.yaml"))
    assert shipped.get("gfkb.device_featurize") is False

    eng = GfkbEngine(data_dir=str(tmp_path / "a"), device="cpu", dim=64)
    assert eng.encoder.device_featurize is False
    eng_on = GfkbEngine(data_dir=str(tmp_path / "b"), device="cpu", dim=64,
                        device_featurize=True)
    assert eng_on.encoder.device_featurize is True

    # the two engines store and match alike
    sigs = fc.signature_texts(24)
    for e in (eng, eng_on):
        for i, s in enumerate(sigs):
            e.upsert_failure("T%d" % (i % 3), s, {}, app_id="app")
    for q in sigs[:6]:
        a, b = eng.match(q), eng_on.match(q)
        assert [m.failure_id for m in a] == [m.failure_id for m in b]
        assert [m.score for m in a] == [m.score for m in b]

    # the service turns it on from the config file, and leaves it off otherwise
    path = tmp_path / "config.yaml"
    path.write_text("gfkb:\n  device_featurize: true\n")
    create_app(engine=eng, config=ConfigStore(str(path)))
    assert eng.encoder.device_featurize is True
    eng2 = GfkbEngine(data_dir=str(tmp_path / "c"), device="cpu", dim=64)
    path.write_text("gfkb:\n  device_featurize: false\n")
    create_app(engine=eng2, config=ConfigStore(str(path)))
    assert eng2.encoder.device_featurize is False
