"""The trace-encoder model: hashed features -> 768-d unit embedding.

MI355X-native analogue of the reference's similarity space (SURVEY.md
section 2.5 row 'failure_classifier.on_trace'): a random-init embedding
table (the hashed-feature projection) followed by a small GEMM stack whose
weight is orthogonal, so cosine structure of the sparse feature space is
preserved exactly — required to keep the reference's >=0.8 match-threshold
semantics (config/config.yaml:2) meaningful after encoding.

GPU path: fused embedding-bag HIP kernel (ops.embedding_bag) + hipBLASLt
GEMM via torch.matmul for the projection + fused L2-normalise. CPU path:
the same math in plain torch (deterministic, used by BASELINE config 1).
"""

from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from kakveda_amd.encoder.featurizer import featurize_batch, pack_texts

#: batch size from which ``device_featurize=True`` hashes on a CUDA device
#: (None would mean never: the flag inert). Measured,
#: profiles/device_featurize.md: the smallest B from which the device arm of
#: encode_texts beats the host arm by more than the spread between rounds is
#: the smallest measured, 1 (0.139 against 0.151 ms, both arms within 0.9%;
#: 24x at 64 texts, 370x at 2,048)
DEVICE_FEATURIZE_MIN_B: Optional[int] = 1


class TraceEncoder:
    def __init__(
        self,
        dim: int = 768,
        hash_dim: int = 1 << 16,
        seed: int = 1234,
        device: str = "cpu",
        depth: int = 2,
        max_features: int = 64,
        device_featurize: bool = False,
    ):
        self.dim = dim
        self.hash_dim = hash_dim
        self.seed = seed
        self.max_features = max_features
        self.device = torch.device(device)
        #: hash the texts with ops.featurize_bytes instead of featurize_batch
        #: (off by default). On a CUDA device that is the HIP kernel, from
        #: DEVICE_FEATURIZE_MIN_B texts on; on a CPU device the reference op.
        self.device_featurize = device_featurize
        #: rows the device featurizer handed back to featurize_batch so far
        self.host_fallbacks = 0

        gen = torch.Generator(device="cpu").manual_seed(seed)
        # Hashed-feature embedding table, scaled so bag outputs are O(1).
        table = torch.randn(hash_dim, dim, generator=gen, dtype=torch.float32) / (dim**0.5)
        # GEMM stack: product of `depth` orthogonal matrices (exact isometry).
        w = torch.eye(dim, dtype=torch.float32)
        for _ in range(depth):
            q, r = torch.linalg.qr(torch.randn(dim, dim, generator=gen, dtype=torch.float32))
            q = q * torch.sign(torch.diagonal(r)).unsqueeze(0)  # fix QR sign ambiguity
            w = w @ q
        self._table = table.to(self.device)
        self._proj = w.to(self.device)
        if self.device.type == "cuda":
            # bf16 resident copies for the GPU hot path
            self._table_bf16 = self._table.to(torch.bfloat16)
            self._proj_bf16 = self._proj.to(torch.bfloat16)

    @torch.no_grad()
    def encode_texts(self, texts: Sequence[str]) -> torch.Tensor:
        """Encode signature texts -> [B, dim] unit-norm float32 embeddings."""
        if self._featurize_on_device(len(texts)):
            return self.encode_features(*self._featurize_device(texts))
        idx, w = featurize_batch(
            texts, hash_dim=self.hash_dim, seed=0, max_features=self.max_features
        )
        return self.encode_features(
            torch.from_numpy(idx).to(self.device),
            torch.from_numpy(w).to(self.device),
        )

    def _featurize_on_device(self, n_texts: int) -> bool:
        if not self.device_featurize or n_texts == 0 or self.max_features > 128:
            return False
        if self.device.type != "cuda":
            return True  # the reference op: the same plumbing without a GPU
        return DEVICE_FEATURIZE_MIN_B is not None and n_texts >= DEVICE_FEATURIZE_MIN_B

    def _featurize_device(self, texts: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        """``featurize_batch`` through ``ops.featurize_bytes``: pack, upload,
        hash on the device, then redo on the host the rows the device could
        not take (``pack_texts``'s host rows and the rows it flagged). One
        integer comes back from the device when nothing was flagged."""
        from kakveda_amd import ops

        buf, offsets, host_rows = pack_texts(texts)
        idx, w, status, flagged = ops.featurize_bytes(
            torch.from_numpy(buf).to(self.device),
            torch.from_numpy(offsets).to(self.device),
            self.hash_dim,
            0,
            self.max_features,
        )
        redo = list(host_rows)
        if int(flagged.item()) > 0:
            # host rows were packed empty (status 0): no row is listed twice
            redo += torch.nonzero(status).flatten().tolist()
        if redo:
            hidx, hw = featurize_batch(
                [texts[i] for i in redo],
                hash_dim=self.hash_dim,
                seed=0,
                max_features=self.max_features,
            )
            rows = torch.tensor(redo, dtype=torch.int64, device=self.device)
            idx[rows] = torch.from_numpy(hidx).to(self.device)
            w[rows] = torch.from_numpy(hw).to(self.device)
            self.host_fallbacks += len(redo)
        return idx, w

    @torch.no_grad()
    def encode_features(self, idx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """Encode pre-hashed padded features [B, L] -> [B, dim] unit fp32."""
        if self.device.type == "cuda":
            from kakveda_amd import ops

            bag = ops.embedding_bag(self._table_bf16, idx, w)  # [B, dim] f32
            out = (bag.to(torch.bfloat16) @ self._proj_bf16).float()
        else:
            flat = self._table[idx.reshape(-1).long()].reshape(*idx.shape, self.dim)
            bag = (flat * w.unsqueeze(-1)).sum(dim=1)
            out = bag @ self._proj
        norm = out.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        return out / norm

    @torch.no_grad()
    def encode_text(self, text: str) -> torch.Tensor:
        return self.encode_texts([text])[0]
