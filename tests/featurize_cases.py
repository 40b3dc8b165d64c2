"""Texts for the device featurizer's tests (CPU and GPU share them): the
edge list a wave-parallel tokeniser goes wrong on, seeded random texts and
realistic signatures, plus the status rules computed on the CPU."""

import random

import numpy as np

from kakveda_amd import ops
from kakveda_amd.core.signature import signature_text
from kakveda_amd.encoder.featurizer import featurize, tokenize

MAX_BYTES = ops.FEATURIZE_MAX_BYTES
MAX_GRAMS = ops.FEATURIZE_MAX_GRAMS

#: three exactly-zero buckets at hash_dim=64, two at hash_dim=8
ZERO_BUCKET_64 = "Explain THE sky_with-refs: v1.2 [1] (Doe, 2020)"
ZERO_BUCKET_8 = "w8 w36 w4 w16 w7 w31"


def of_length(n: int) -> str:
    """A text of exactly n bytes: words of varying length, single spaces."""
    words, i = [], 0
    while sum(len(x) + 1 for x in words) < n + 8:
        words.append("w%d" % (i * 7919 % 1000) + "x" * (i % 5))
        i += 1
    return " ".join(words)[:n]


def edge_texts():
    """(name, text) pairs; every text is ASCII and at most MAX_BYTES long."""
    out = [
        ("empty", ""),
        ("separators", " \t!?()[]  ,;"),
        ("one_token", "alpha"),
        ("repeat", "a a a a"),
        ("upper", "Hello WORLD MiXeD hello world mixed"),
        ("punct_in_tokens", "a_b c:d e.f g-h _:.- x_:.-y"),
        ("high_bytes", "caf\x7f na\x00ive a\x1fb"),
        ("zero64", ZERO_BUCKET_64),
        ("zero8", ZERO_BUCKET_8),
        # a token that ends exactly at the text's end / exactly on a step
        ("ends_in_token", "lead trail"),
        ("token_to_step_end", "x" * 60 + " abc" + " tail"),  # 'abc' ends at byte 64
        ("token_from_step_start", " " * 64 + "abc def"),  # 'abc' starts at byte 64
        ("straddle", "y" * 50 + " " + "straddlingtokenacrossstep" + " end"),
        ("long_token", "pre " + "z" * 150 + " post"),
        ("long_token_only", "q" * 64),
        ("full_token", "t" * MAX_BYTES),
    ]
    for n in (1, 63, 64, 65, 127, 128, 129, MAX_BYTES - 1, MAX_BYTES):
        out.append(("len%d" % n, of_length(n)))
    # more than MAX_GRAMS grams, few distinct: 129 tokens -> 257 grams
    out.append(("many_grams_few_distinct", " ".join(["ab", "cd"] * 65)[: 129 * 3 - 1]))
    # exactly MAX_GRAMS - 1 grams (128 tokens): the largest text that fits
    out.append(("max_tokens", " ".join("k%d" % i for i in range(128))))
    out.append(("max_tokens_repeat", " ".join(["r"] * 128)))
    return out


def n_features(text: str, hash_dim: int, seed: int = 0) -> int:
    return len(featurize(text, hash_dim=hash_dim, seed=seed)[0])


def with_features(target: int, hash_dim: int, seed: int = 0) -> str:
    """A text with exactly ``target`` features: distinct words are added one
    at a time (each adds up to two grams) until the count is met; a word
    that would jump over the target is skipped."""
    words, i = [], 0
    while True:
        have = n_features(" ".join(words), hash_dim, seed)
        if have == target:
            return " ".join(words)
        assert have < target and i < 100000
        cand = words + ["f%d" % i]
        i += 1
        if n_features(" ".join(cand), hash_dim, seed) <= target:
            words = cand


def expected_status(text: str, hash_dim: int, seed: int, max_features: int) -> int:
    """The status rules, on the CPU."""
    n_tok = len(tokenize(text))
    if len(text.encode("utf-8")) > MAX_BYTES or 2 * n_tok - 1 > MAX_GRAMS:
        return 1
    if n_features(text, hash_dim, seed) > max_features:
        return 2
    return 0


def random_texts(n: int = 512, seed: int = 20240607):
    """Seeded random texts, lengths 0 to 300, over token bytes, separators
    and capitals."""
    rng = random.Random(seed)
    alphabet = "abcdeXYZ019_:.-" + "  \t,;()!" + "abAB"
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 300))) for _ in range(n)]


_WORDS = (
    "summarize explain describe the report include references citations sources "
    "please provide a short summary of this document with bibliography even if "
    "none translate code review quarterly results customer email draft policy"
).split()[:30]
_TOOLS = ("search", "calculator", "browser", "code_interpreter", "retriever")


def signature_texts(n: int = 2048, seed: int = 7):
    """Realistic signatures: prompts of 5 to 30 words from a fixed 30-word
    list, 0 to 3 tools, two env keys."""
    assert len(_WORDS) == 30
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        prompt = " ".join(rng.choice(_WORDS) for _ in range(rng.randint(5, 30)))
        tools = rng.sample(_TOOLS, rng.randint(0, 3))
        env = {"region_%d" % rng.randint(0, 9): 1, "tier_%d" % rng.randint(0, 3): 1}
        out.append(signature_text(prompt, tools, env))
    return out


def pack(texts):
    """Bytes back to back and int32 offsets, with no host rows taken out."""
    raw = [t.encode("ascii") for t in texts]
    offsets = np.zeros(len(raw) + 1, dtype=np.int32)
    np.cumsum([len(r) for r in raw], out=offsets[1:])
    return np.frombuffer(bytearray(b"".join(raw)), dtype=np.uint8), offsets
