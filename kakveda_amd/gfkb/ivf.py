"""Cluster-routed (IVF) index over an ``EmbeddingStore``.

The optional approximate search mode: the store's rows stay where they are
and an ``IvfIndex`` beside them holds L unit centroids plus a CSR inverted
list of row ids. A routed search scores the queries against the centroids,
scans the ``nprobe`` best lists per query and every row appended since the
index was built (the tail), and returns the exact top-k of that candidate
set (``ops.ivf_search``). With ``nprobe == n_lists`` that is the exact
search's result; below it, recall depends on how well the data clusters.

Building is offline work: Lloyd iterations on a sample through
``StreamingKMeans`` (above 512 lists ``ops.kmeans_update`` takes its eager
path), one chunked assignment pass over all rows, one stable sort. The
index is immutable; a rebuild makes a new one and swaps it in.
"""

from __future__ import annotations

import math
import time
from dataclasses import dataclass, field
from typing import Any, Dict, Optional

import torch

from kakveda_amd import ops
from kakveda_amd.patterns.kmeans import StreamingKMeans

#: rows per ``ops.kmeans_assign`` call of the assignment pass
ASSIGN_CHUNK = 1 << 20
#: sample rows per list for the Lloyd iterations when ``sample`` is unset
SAMPLE_PER_LIST = 256


def default_n_lists(n: int) -> int:
    """~sqrt(N), a multiple of 8, within [16, 16384]."""
    l = int(round(math.sqrt(max(n, 1)) / 8.0)) * 8
    return max(16, min(16384, l))


@dataclass(frozen=True)
class IvfIndex:
    centroids: torch.Tensor  # [L, D], store dtype, unit rows
    offsets: torch.Tensor  # int64 [L + 1]
    ids: torch.Tensor  # int32 [n_indexed], global row ids
    n_indexed: int
    n_lists: int
    max_list_len: int
    stats: Dict[str, Any] = field(default_factory=dict)

    @classmethod
    def build(
        cls,
        store,
        n_lists: Optional[int] = None,
        iters: int = 8,
        sample: Optional[int] = None,
        seed: int = 0,
    ) -> "IvfIndex":
        t0 = time.perf_counter()
        n = int(store.count)
        if n < 1:
            raise ValueError("cannot build a routed index over an empty store")
        L = default_n_lists(n) if n_lists is None else int(n_lists)
        if L < 1:
            raise ValueError("n_lists must be >= 1")
        L = min(L, n)
        dev = store.device
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        n_sample = min(n, int(sample) if sample else max(L * SAMPLE_PER_LIST, 1 << 16))
        pick = torch.randperm(n, generator=gen)[:n_sample].sort().values
        pts = ops._gather_rows(
            [seg[:valid] for seg, valid, _base in store._live_segments(n)], pick.to(dev)
        )
        km = StreamingKMeans(L, store.dim, device=str(dev), seed=int(seed))
        # start from data rows: random directions leave lists empty
        km.centroids = pts[torch.randperm(n_sample, generator=gen)[:L].to(dev)].float()
        if iters > 0:
            km.fit(pts, iters=int(iters))
        centroids = km.centroids.to(store.dtype).contiguous()
        del pts

        assign = torch.empty(n, dtype=torch.int64, device=dev)
        for lo in range(0, n, ASSIGN_CHUNK):
            hi = min(lo + ASSIGN_CHUNK, n)
            assign[lo:hi] = ops.kmeans_assign(store.row_range(lo, hi), centroids)
        ids = torch.sort(assign, stable=True).indices.to(torch.int32)
        counts = torch.bincount(assign, minlength=L)
        offsets = torch.zeros(L + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts, 0)
        c = counts.cpu()
        stats = {
            "n_lists": L,
            "n_indexed": n,
            "list_min": int(c.min()),
            "list_median": int(c.median()),
            "list_max": int(c.max()),
            "empty_lists": int((c == 0).sum()),
            "sample_rows": n_sample,
            "iters": int(iters),
        }
        idx = cls(
            centroids=centroids,
            offsets=offsets.contiguous(),
            ids=ids.contiguous(),
            n_indexed=n,
            n_lists=L,
            max_list_len=int(c.max()),
            stats=stats,
        )
        idx.validate()
        stats["build_seconds"] = time.perf_counter() - t0
        return idx

    def validate(self) -> None:
        """CPU-side check of the id table before it reaches a kernel."""
        off = self.offsets.cpu().long()
        ids = self.ids.cpu().long()
        if off.shape[0] != self.n_lists + 1 or self.centroids.shape[0] != self.n_lists:
            raise ValueError("routed index: offsets/centroids do not match n_lists")
        if int(off[0]) != 0 or int(off[-1]) != self.n_indexed:
            raise ValueError("routed index: offsets must run from 0 to n_indexed")
        if bool((off[1:] < off[:-1]).any()):
            raise ValueError("routed index: offsets are not monotone")
        if ids.shape[0] != self.n_indexed:
            raise ValueError("routed index: ids must have n_indexed entries")
        if self.n_indexed and not torch.equal(
            ids.sort().values, torch.arange(self.n_indexed, dtype=torch.int64)
        ):
            raise ValueError("routed index: ids are not a permutation of [0, n_indexed)")
        if int((off[1:] - off[:-1]).max()) != self.max_list_len:
            raise ValueError("routed index: max_list_len does not match offsets")
