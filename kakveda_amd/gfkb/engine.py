"""The GFKB engine: durable JSONL log + device-resident embedding store.

Service-level parity with the reference GFKB
(/root/reference/services/gfkb/app.py:74-198): versioned append-only
failure upserts keyed by (failure_type, signature_text), F-%04d /
FP-%04d id numbering over total row count, top-5-then-type-filter match
ordering, latest-per-id pattern listing, name-identity pattern upserts.

MI355X-first redesign: instead of re-reading the
JSONL and refitting TF-IDF per request, the engine keeps one embedding row
per failure *identity* in a preallocated device tensor (bf16 in HBM3E on
GPU, fp32 on CPU) and matches with the fused cosine-topk kernel. Deliberate
divergence from the reference: the reference scores every *version* row, so
its top-5 can be five copies of one failure; this engine searches one row
per identity and reports the latest version — strictly more informative,
same wire shapes.

Opt-in divergence: ``filter_first`` applies the ``failure_type`` of a match
inside the search (each store row carries its type as an int32 label and
the kernels skip other rows), so the answer is the top-k of that type
instead of whatever of that type survived the global top-k cut.
"""

from __future__ import annotations

import json
import logging
import threading
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

from kakveda_amd import ops
from kakveda_amd.core.schemas import (
    CanonicalFailureRecord,
    FailureMatch,
    PatternEntity,
    Severity,
    utcnow,
)
from kakveda_amd.core.store import JsonlLog
from kakveda_amd.encoder.model import TraceEncoder

logger = logging.getLogger(__name__)

#: tail rows / indexed rows past which a routed store asks for a rebuild
STALE_WARN_FRACTION = 0.10

#: rows per quantiser call when a filled store builds its int8 mirror
MIRROR_CHUNK_ROWS = 1 << 20


class EmbeddingStore:
    """A growable, segmented [N, D] row store on a device; rows are unit
    vectors. On GPU the rows are bf16 in HBM3E; queries arrive fp32 and
    are cast.

    Growth never needs 2x memory at scale: the
    store is a list of segments. The first segment doubles in place only
    while it is small (< ``segment_rows``); past that, growth allocates a
    fresh fixed-size segment and leaves existing rows where they are, so a
    154 GB-resident store can keep accepting live inserts without a 308 GB
    transient. Searches run the fused kernel once per live segment (each
    >= millions of rows, so launch overhead is amortised) and merge the
    per-segment (score, global-row) candidates with one tiny topk.

    Insertion appends rows at the live prefix; the search kernel only scans
    the first ``count`` rows (valid_n), so inserts while serving are safe
    under the engine lock.

    Every row also carries an int32 label (-1 = unlabelled; 4 B beside a
    1536-B bf16 row), one label tensor per segment, growing and splitting
    with the rows. ``search(..., want=...)`` restricts each query to the
    rows of one label inside the scan (``ops.cosine_topk_filtered``).

    Optional int8 mirror (``int8_mirror=True`` or ``enable_mirror()``): per
    segment an int8 copy of the rows with one (scale, error bound) pair per
    row, created, grown, split and adopted with the rows as the labels are.
    Exact searches of up to ``ops.Q8_MAX_B`` queries scan it instead of the
    bf16 rows and rescore the survivors from them (``ops.cosine_topk_q8``):
    the same answer from about half the bytes. Unfiltered batches of at least
    ``ops.Q8_BATCH_MIN_B`` queries are screened with it on the int8 matrix
    cores and rescored the same way: the same answer from about half the
    matrix-core cycles. The routed scans stay bf16.

    Optional routed search: ``build_index()`` attaches an ``IvfIndex``
    (gfkb/ivf.py) and ``search(..., nprobe=n)`` then scans only the n best
    inverted lists per query plus the tail of rows appended since the build.
    It is approximate and strictly opt-in: ``nprobe=None`` is the exact
    search, whether an index is attached or not. A label-filtered batch is
    routed only with ``route_filtered=True`` (``ops.ivf_search_filtered``);
    the per-label row counts kept at insertion then let the store re-run,
    exactly, the queries whose label's rows sat in unprobed lists.
    """

    def __init__(
        self,
        dim: int,
        device: str = "cpu",
        capacity: int = 1024,
        segment_rows: Optional[int] = None,
        int8_mirror: bool = False,
    ):
        self.dim = dim
        self.device = torch.device(device)
        self.dtype = torch.bfloat16 if self.device.type == "cuda" else torch.float32
        self.segment_rows = int(
            segment_rows
            if segment_rows is not None
            else ((4 << 20) if self.device.type == "cuda" else (1 << 16))
        )
        self._segments: List[torch.Tensor] = [
            torch.zeros(capacity, dim, dtype=self.dtype, device=self.device)
        ]
        self._labels: List[torch.Tensor] = [self._new_labels(capacity)]
        #: rows per label, kept on the host by append/adopt (the insert
        #: path) for the exact fill of a routed filtered search
        self._label_counts: Dict[int, int] = {}
        self.count = 0
        #: the routed-search index (None: exact search only)
        self.index = None
        self._stale_warned = False
        #: filtered queries a routed filtered search handed to the exact fill
        self.exact_fills = 0
        #: the optional int8 mirror (ops.quantize_rows_q8): one codes and one
        #: meta tensor per segment, empty lists while it is off
        self.int8_mirror = False
        self._codes: List[torch.Tensor] = []
        self._meta: List[torch.Tensor] = []
        #: per segment, at least the largest norm of its mirrored rows (fp32
        #: [1]; q8_plan.h cnorm), raised where the rows are quantised
        self._cnorm: List[torch.Tensor] = []
        if int8_mirror:
            self.enable_mirror()

    # -- int8 mirror ---------------------------------------------------------

    def _new_mirror(self, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return ops.new_q8_mirror(n, self.dim, self.device)

    def _quantize(self, seg_no: int, lo: int, hi: int) -> None:
        """Quantise rows [lo, hi) of segment ``seg_no`` into its mirror, in
        chunks of at most MIRROR_CHUNK_ROWS rows."""
        seg = self._segments[seg_no]
        for a in range(lo, hi, MIRROR_CHUNK_ROWS):
            b = min(a + MIRROR_CHUNK_ROWS, hi)
            ops.quantize_rows_q8(
                seg[a:b], self._codes[seg_no], self._meta[seg_no], a, self._cnorm[seg_no]
            )

    def enable_mirror(self) -> None:
        """Turn the int8 mirror on: allocate it beside every segment and
        quantise the live rows. From then on ``append`` keeps it current and
        exact small-batch searches read it (``ops.cosine_topk_q8``). It costs
        (D + 8) / (2 D) of the rows' memory on a GPU store."""
        if self.int8_mirror:
            return
        pairs = [self._new_mirror(int(seg.shape[0])) for seg in self._segments]
        self._codes = [c for c, _m in pairs]
        self._meta = [m for _c, m in pairs]
        self._cnorm = [ops.new_q8_cnorm(self.device) for _ in pairs]
        for i, (_seg, valid, _base) in enumerate(self._live_segments()):
            self._quantize(i, 0, valid)
        self.int8_mirror = True

    def mirror_range(self, start: int, end: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(codes, meta) of rows [start, end), each as one tensor."""
        if not self.int8_mirror:
            raise RuntimeError("the store has no int8 mirror: call enable_mirror()")
        end = min(end, self.count)
        cs, ms = [], []
        for i, (_seg, valid, base) in enumerate(self._live_segments()):
            lo, hi = max(start - base, 0), min(end - base, valid)
            if lo < hi:
                cs.append(self._codes[i][lo:hi])
                ms.append(self._meta[i][lo:hi])
        if not cs:
            return self._codes[0][:0], self._meta[0][:0]
        return torch.cat(cs, dim=0), torch.cat(ms, dim=0)

    def _new_labels(self, n: int) -> torch.Tensor:
        return torch.full((n,), -1, dtype=torch.int32, device=self.device)

    def _count_labels(self, labels: Optional[torch.Tensor], n: int) -> None:
        """Add ``n`` new rows to the per-label row counts (None: all -1)."""
        if labels is None:
            if n:
                self._label_counts[-1] = self._label_counts.get(-1, 0) + n
            return
        values, counts = torch.unique(labels, return_counts=True)
        for v, c in zip(values.tolist(), counts.tolist()):
            self._label_counts[int(v)] = self._label_counts.get(int(v), 0) + int(c)

    def label_rows(self, label: int) -> int:
        """Rows that carry ``label`` (counted at insertion, on the host)."""
        return self._label_counts.get(int(label), 0)

    @property
    def capacity(self) -> int:
        return sum(int(s.shape[0]) for s in self._segments)

    @property
    def n_segments(self) -> int:
        return len(self._segments)

    def _grow_to(self, needed: int) -> None:
        while self.capacity < needed:
            if len(self._segments) == 1 and self._segments[0].shape[0] < self.segment_rows:
                # small store: double the single segment in place (cheap,
                # bounded by segment_rows) so tiny corpora stay contiguous
                cap = int(self._segments[0].shape[0])
                while cap < min(needed, self.segment_rows):
                    cap *= 2
                fresh = torch.zeros(cap, self.dim, dtype=self.dtype, device=self.device)
                fresh[: self.count] = self._segments[0][: self.count]
                self._segments[0] = fresh
                labels = self._new_labels(cap)
                labels[: self.count] = self._labels[0][: self.count]
                self._labels[0] = labels
                if self.int8_mirror:
                    codes, meta = self._new_mirror(cap)
                    codes[: self.count] = self._codes[0][: self.count]
                    meta[: self.count] = self._meta[0][: self.count]
                    self._codes[0], self._meta[0] = codes, meta
            else:
                # at scale: copy-free growth by a fixed segment quantum
                self._segments.append(
                    torch.zeros(
                        self.segment_rows, self.dim, dtype=self.dtype, device=self.device
                    )
                )
                self._labels.append(self._new_labels(self.segment_rows))
                if self.int8_mirror:
                    codes, meta = self._new_mirror(self.segment_rows)
                    self._codes.append(codes)
                    self._meta.append(meta)
                    self._cnorm.append(ops.new_q8_cnorm(self.device))

    def adopt(self, data: torch.Tensor, labels: Optional[torch.Tensor] = None) -> None:
        """Take ownership of a pre-built [n, D] row tensor (zero copy) —
        used by benches/restore paths where the rows already live on the
        device in the right dtype. Later appends grow segment-wise.
        ``labels`` ([n] ints) default to all unlabelled."""
        assert data.dtype == self.dtype and data.shape[1] == self.dim
        n = int(data.shape[0])
        if labels is None:
            lab = self._new_labels(n)
        else:
            assert labels.shape == (n,)
            lab = labels.to(device=self.device, dtype=torch.int32).contiguous()
        self._segments = [data]
        self._labels = [lab]
        self.count = n
        self._label_counts = {}
        self._count_labels(labels, n)
        self.index = None  # it described the rows just replaced
        if self.int8_mirror:
            codes, meta = self._new_mirror(n)
            self._codes, self._meta = [codes], [meta]
            self._cnorm = [ops.new_q8_cnorm(self.device)]
            self._quantize(0, 0, n)

    def append(self, rows: torch.Tensor, labels: Optional[torch.Tensor] = None) -> int:
        """Append [n, D] rows (splitting across segments); returns the
        first new row index. ``labels`` ([n] ints) default to unlabelled."""
        n = rows.shape[0]
        if labels is not None:
            assert labels.shape == (n,)
        # counted where the caller's labels live (host tensors from the
        # engine): no device read on the insert path
        self._count_labels(labels, n)
        if labels is not None:
            labels = labels.to(device=self.device, dtype=torch.int32)
        self._grow_to(self.count + n)
        first = self.count
        written = 0
        base = 0
        for seg_no, (seg, lab) in enumerate(zip(self._segments, self._labels)):
            seg_rows = int(seg.shape[0])
            if self.count + written < base + seg_rows and written < n:
                off = self.count + written - base
                take = min(seg_rows - off, n - written)
                seg[off : off + take] = rows[written : written + take].to(self.dtype)
                # the mirror of exactly these rows, before count is bumped:
                # rows below count are immutable in both copies
                if self.int8_mirror:
                    self._quantize(seg_no, off, off + take)
                # slots past the live prefix are -1 already (never reused)
                if labels is not None:
                    lab[off : off + take] = labels[written : written + take]
                written += take
            base += seg_rows
        assert written == n
        self.count += n
        return first

    def _live_segments(
        self, count: Optional[int] = None
    ) -> List[Tuple[torch.Tensor, int, int]]:
        """(tensor, valid_rows, global_base) for every non-empty segment."""
        out = []
        base = 0
        total = self.count if count is None else count
        for seg in self._segments:
            seg_rows = int(seg.shape[0])
            valid = min(total - base, seg_rows)
            if valid <= 0:
                break
            out.append((seg, valid, base))
            base += seg_rows
        return out

    # -- routed (IVF) search ------------------------------------------------

    def build_index(self, **kw):
        """Build an ``IvfIndex`` over the live rows and attach it (replacing
        any earlier one). Keyword arguments go to ``IvfIndex.build``.
        Callers that serve concurrently swap it in under their own lock
        (``GfkbEngine.build_index``)."""
        from kakveda_amd.gfkb.ivf import IvfIndex

        index = IvfIndex.build(self, **kw)
        self.index = index
        self._stale_warned = False
        return index

    @property
    def stale_fraction(self) -> float:
        """Rows appended since the index was built, as a fraction of the
        rows it covers (0.0 without an index). These tail rows are scanned
        by every routed search, so the figure is the routed mode's growing
        fixed cost, not a loss of recall."""
        index = self.index
        if index is None or index.n_indexed <= 0:
            return 0.0
        return max(self.count - index.n_indexed, 0) / float(index.n_indexed)

    def _warn_stale(self, index) -> None:
        tail = self.count - index.n_indexed
        if not self._stale_warned and tail > STALE_WARN_FRACTION * index.n_indexed:
            self._stale_warned = True
            logger.warning(
                "routed index is stale: %d rows appended since it was built over "
                "%d (%.0f%%); every routed search scans them all - rebuild with "
                "build_index()",
                tail,
                index.n_indexed,
                100.0 * tail / max(index.n_indexed, 1),
            )

    def _search_routed(
        self, q: torch.Tensor, k: int, count: int, nprobe: int, index,
        batched: Optional[bool] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        self._warn_stale(index)
        # a snapshot older than the index is safe: the scan drops listed ids
        # >= count and the tail is then empty
        return ops.ivf_search(
            q,
            [seg for seg, _v, _b in self._live_segments(count)],
            index.centroids,
            index.offsets,
            index.ids,
            min(nprobe, index.n_lists),
            k,
            count,
            index.n_indexed,
            index.max_list_len,
            batched=batched,
        )

    def _search_routed_filtered(
        self, q: torch.Tensor, k: int, count: int, want: torch.Tensor,
        nprobe: int, index, batched: Optional[bool], fill_exact: bool,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The routed search with the label predicate inside the scan, then
        the exact fill: a filtered query that holds fewer live results than
        ``min(k, rows of its label)`` had rows of its label in lists it did
        not probe, and is answered again by the exact filtered search."""
        self._warn_stale(index)
        segs = self._live_segments(count)
        w = want.to(device=self.device, dtype=torch.int32)
        nprobe = min(nprobe, index.n_lists)
        want_h = want.tolist()
        if (
            batched is None
            and len(want_h) < ops.IVF_FILTERED_SPARSE_MIN_B
            and all(wb >= 0 for wb in want_h)
            and max(self.label_rows(wb) for wb in want_h)
            <= ops.IVF_FILTERED_SPARSE_SHARE * count
        ):
            # every query wants a rare label: the per-query scan skips
            # nearly every row and stays ahead up to that many queries
            batched = False
        scores, idx = ops.ivf_search_filtered(
            q,
            [seg for seg, _v, _b in segs],
            self._labels[: len(segs)],  # the live segments are a prefix
            w,
            index.centroids,
            index.offsets,
            index.ids,
            nprobe,
            k,
            count,
            index.n_indexed,
            index.max_list_len,
            batched=batched,
        )
        if not fill_exact or nprobe >= index.n_lists:
            return scores, idx
        # the counts may include rows appended after the ``count`` snapshot:
        # that can only ask for an exact re-run that was not needed
        found = (idx >= 0).sum(dim=1).tolist()
        short = [
            b
            for b, wb in enumerate(want_h)
            if wb >= 0 and found[b] < min(k, self.label_rows(wb))
        ]
        self.exact_fills += len(short)
        if short:
            sel = torch.tensor(short, dtype=torch.int64, device=self.device)
            fill_s, fill_i = self.search(q[sel], k, valid_n=count, want=w[sel])
            scores[sel] = fill_s
            idx[sel] = fill_i
        return scores, idx

    def search(
        self,
        queries: torch.Tensor,
        k: int,
        valid_n: Optional[int] = None,
        want: Optional[torch.Tensor] = None,
        nprobe: Optional[int] = None,
        index=None,
        batched: Optional[bool] = None,
        route_filtered: bool = False,
        fill_exact: bool = True,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Top-k over the first ``valid_n`` rows (default: the live count).
        Passing a snapshot of ``count`` makes the search safe to run
        outside the engine lock while appends continue: rows below the
        snapshot are immutable once written.

        ``want`` ([B] ints) restricts query b to the rows labelled
        ``want[b]`` (negative: no restriction for that query); rows short
        of k such rows are padded with (-inf, -1). ``want=None`` is the
        unfiltered search.

        ``nprobe`` > 0 asks for the routed (approximate) search over the
        attached index: the ``nprobe`` best lists per query (clamped to the
        list count) plus every row appended since the build. It raises
        without an index. A label-filtered batch (``want`` set) is answered
        by the exact filtered search whatever ``nprobe`` says: exact is
        never worse, and a filtered query is not silently routed - unless
        ``route_filtered`` is set: then the batch runs the routed search
        with the label predicate inside the scan
        (``ops.ivf_search_filtered``; queries with a negative ``want`` ride
        along unfiltered). With ``fill_exact`` (the default) every filtered
        query that then holds fewer than ``min(k, rows of its label)`` live
        results is run again through the exact filtered search, so a label
        with at least k rows never comes back short because its rows sat in
        unprobed lists; ``fill_exact=False`` returns the routed answer as it
        is. With ``batched=None`` a batch whose every query wants a label
        that at most ``ops.IVF_FILTERED_SPARSE_SHARE`` of the rows carry
        stays on the per-query scan below ``ops.IVF_FILTERED_SPARSE_MIN_B``
        queries (measured: it skips nearly every row there). ``index``
        is the index to route through (default: the attached one), for
        callers that snapshot it together with ``valid_n``. ``batched``
        picks the routed scan kernel (``ops.ivf_scan_topk``: None chooses by
        batch size); it changes no result beyond fp32 summation order.

        ``k > ops.KMAX`` (up to ``ops.KWIDE_MAX`` = 64 on a GPU; more comes
        back padded) is the wide search, ``ops.cosine_topk_wide`` per segment:
        always exact and always over the bf16 rows. ``nprobe``, the index and
        the int8 mirror do not apply to it and it never raises over them; a
        filtered batch of more than 8 queries is scanned in groups of 8."""
        q = queries.to(self.dtype)
        count = self.count if valid_n is None else min(int(valid_n), self.count)
        if k > ops.KMAX:
            return self._search_wide(q, int(k), count, want)
        if nprobe is not None and int(nprobe) < 0:
            raise ValueError("nprobe must be >= 0")
        if nprobe:
            index = self.index if index is None else index
            if index is None:
                raise ValueError(
                    "nprobe was given but the store has no routed index: "
                    "call build_index() first"
                )
            if want is None and count > 0:
                return self._search_routed(q, k, count, int(nprobe), index, batched)
            if route_filtered and count > 0:
                return self._search_routed_filtered(
                    q, k, count, want, int(nprobe), index, batched, fill_exact
                )
        segs = self._live_segments(count)
        w = None if want is None else want.to(device=self.device, dtype=torch.int32)

        # exact from here on. With the int8 mirror on, small batches scan it
        # (ops.Q8_MAX_B) and unfiltered batches from ops.Q8_BATCH_MIN_B
        # queries on are screened with it; both rescore from the bf16 rows.
        q8 = self.int8_mirror and (
            q.shape[0] <= ops.Q8_MAX_B
            or (want is None and q.shape[0] >= ops.Q8_BATCH_MIN_B)
        )

        def topk(seg_no: int, n: int):
            seg, labels = self._segments[seg_no], self._labels[seg_no]
            if q8:
                return ops.cosine_topk_q8(
                    q, seg, self._codes[seg_no], self._meta[seg_no], k, valid_n=n,
                    labels=None if w is None else labels, want=w,
                    cnorm=self._cnorm[seg_no],
                )
            if w is None:
                return ops.cosine_topk(q, seg, k, valid_n=n)
            return ops.cosine_topk_filtered(q, seg, labels, w, k, valid_n=n)

        if len(segs) <= 1:
            return topk(0, count)
        parts_s, parts_i = [], []
        # the live segments are a prefix of _segments, so labels line up
        for seg_no, (seg, valid, base) in enumerate(segs):
            s, i = topk(seg_no, valid)
            parts_i.append(torch.where(i < 0, i, i + base))
            parts_s.append(s)
        all_s = torch.cat(parts_s, dim=1)
        all_i = torch.cat(parts_i, dim=1)
        top_s, sel = torch.topk(all_s, min(k, all_s.shape[1]), dim=1)
        return top_s, all_i.gather(1, sel)

    def _search_wide(
        self, q: torch.Tensor, k: int, count: int, want: Optional[torch.Tensor]
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``search`` for k > ops.KMAX: ``ops.cosine_topk_wide`` per live
        segment and the cross-segment merge of ``search``."""
        segs = self._live_segments(count)
        w = None if want is None else want.to(device=self.device, dtype=torch.int32)

        def topk(seg_no: int, n: int):
            return ops.cosine_topk_wide(
                q, self._segments[seg_no], k, valid_n=n,
                labels=None if w is None else self._labels[seg_no], want=w,
            )

        if len(segs) <= 1:
            return topk(0, count)
        parts_s, parts_i = [], []
        for seg_no, (seg, valid, base) in enumerate(segs):
            s, i = topk(seg_no, valid)
            parts_i.append(torch.where(i < 0, i, i + base))
            parts_s.append(s)
        all_s = torch.cat(parts_s, dim=1)
        all_i = torch.cat(parts_i, dim=1)
        top_s, sel = torch.topk(all_s, min(k, all_s.shape[1]), dim=1)
        return top_s, all_i.gather(1, sel)

    def label_range(self, start: int, end: int) -> torch.Tensor:
        """Labels of rows [start, end) as one int32 tensor."""
        end = min(end, self.count)
        pieces = []
        base = 0
        for lab in self._labels:
            lo, hi = max(start - base, 0), min(end - base, int(lab.shape[0]))
            if lo < hi:
                pieces.append(lab[lo:hi])
            base += int(lab.shape[0])
        if not pieces:
            return self._labels[0][:0]
        return pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=0)

    def row_range(self, start: int, end: int) -> torch.Tensor:
        """Rows [start, end) as one tensor (a view when they sit in a
        single segment, a copy when they span a boundary)."""
        end = min(end, self.count)
        pieces = []
        for seg, valid, base in self._live_segments():
            lo, hi = max(start - base, 0), min(end - base, valid)
            if lo < hi:
                pieces.append(seg[lo:hi])
        if not pieces:
            return self._segments[0][:0]
        return pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=0)

    @property
    def data(self) -> torch.Tensor:
        """Contiguous view of the live rows. Only valid while the store
        occupies a single segment (benches adopt one tensor); segmented
        stores must use ``row_range``."""
        if len(self._segments) != 1:
            raise RuntimeError(
                "EmbeddingStore.data is single-segment only; use row_range()"
            )
        return self._segments[0]


class EmbeddingSidecar:
    """Packed embedding snapshot beside the JSONL log (SURVEY.md 5.4,
    VERDICT round 1 weak #4): row i is the embedding of identity i in
    engine insertion order, stored raw (bf16 on GPU engines, fp32 on CPU)
    with a tiny JSON meta file. On restart the engine memory-maps this
    file and uploads it H2D in chunks instead of re-encoding every
    identity — an mmap+upload instead of minutes-to-hours of encode at
    10M+ identities. A count/dtype mismatch (hand-edited JSONL, dtype
    change) falls back to re-encode and rewrites the sidecar."""

    VERSION = 1

    def __init__(self, path: Path, dim: int, dtype: torch.dtype):
        self.path = Path(path)
        self.meta_path = self.path.with_suffix(".meta.json")
        self.dim = dim
        self.dtype = dtype
        self._dtype_name = "bfloat16" if dtype == torch.bfloat16 else "float32"
        self._np_dtype = "uint16" if dtype == torch.bfloat16 else "float32"
        self.row_bytes = dim * (2 if dtype == torch.bfloat16 else 4)

    def _meta_ok(self) -> bool:
        try:
            meta = json.loads(self.meta_path.read_text())
            return (
                meta.get("version") == self.VERSION
                and meta.get("dim") == self.dim
                and meta.get("dtype") == self._dtype_name
            )
        except (OSError, ValueError):
            return False

    def count(self) -> int:
        """Rows on disk, or 0 when absent/invalid."""
        if not self.path.exists() or not self._meta_ok():
            return 0
        return self.path.stat().st_size // self.row_bytes

    def _write_meta(self) -> None:
        self.meta_path.write_text(
            json.dumps({"version": self.VERSION, "dim": self.dim, "dtype": self._dtype_name})
        )

    def _to_bytes(self, rows: torch.Tensor) -> bytes:
        t = rows.to(self.dtype).contiguous().cpu()
        if self.dtype == torch.bfloat16:
            t = t.view(torch.uint16)
        return t.numpy().tobytes()

    def append(self, rows: torch.Tensor) -> None:
        if not self.path.exists() or not self._meta_ok():
            # first write (or invalid leftovers): start a fresh file
            self.path.write_bytes(b"")
            self._write_meta()
        with open(self.path, "ab") as f:
            f.write(self._to_bytes(rows))

    def rewrite(self, rows: torch.Tensor) -> None:
        with open(self.path, "wb") as f:
            f.write(self._to_bytes(rows))
        self._write_meta()

    def load_chunks(self, chunk_rows: int = 1 << 18):
        """Yield CPU tensors of up to chunk_rows rows (mmap-backed read)."""
        import numpy as np

        n = self.count()
        if n == 0:
            return
        mm = np.memmap(self.path, dtype=self._np_dtype, mode="r", shape=(n, self.dim))
        for s in range(0, n, chunk_rows):
            chunk = torch.from_numpy(np.array(mm[s : min(s + chunk_rows, n)]))
            if self.dtype == torch.bfloat16:
                chunk = chunk.view(torch.bfloat16)
            yield chunk


class GfkbEngine:
    def __init__(
        self,
        data_dir: str,
        device: str = "cpu",
        dim: int = 768,
        hash_dim: int = 1 << 16,
        encoder_seed: int = 1234,
        top_k: int = 5,
        nprobe: Optional[int] = None,
        route_filtered: bool = False,
        device_featurize: bool = False,
        int8_mirror: bool = False,
    ):
        self.data_dir = Path(data_dir)
        self.data_dir.mkdir(parents=True, exist_ok=True)
        self.failures = JsonlLog(self.data_dir / "failures.jsonl")
        self.patterns = JsonlLog(self.data_dir / "patterns.jsonl")
        self.top_k = top_k
        #: default routed-search width of match()/match_batch(); None or 0
        #: is the exact search. Only takes effect once an index is built.
        self.nprobe = nprobe
        #: whether a batch with a filter-first query stays on the routed
        #: search (label predicate in the scan, exact fill) when ``nprobe``
        #: and an index are in effect; False: such a batch runs exact
        self.route_filtered = route_filtered
        self._lock = threading.RLock()

        # device_featurize: hash signature texts with the device featurizer
        # (TraceEncoder.device_featurize); off by default
        self.encoder = TraceEncoder(
            dim=dim,
            hash_dim=hash_dim,
            seed=encoder_seed,
            device=device,
            device_featurize=device_featurize,
        )
        #: keep an int8 mirror of the rows for exact small-batch searches
        #: (EmbeddingStore.enable_mirror); rebuilt from the rows on restart,
        #: never persisted
        self.int8_mirror = int8_mirror
        self.store = EmbeddingStore(
            dim, device=device, capacity=1024, int8_mirror=int8_mirror
        )
        self.sidecar = EmbeddingSidecar(
            self.data_dir / "embeddings.bin", dim, self.store.dtype
        )

        # identity (failure_type, signature_text) -> latest record dict
        self._latest: Dict[Tuple[str, str], Dict[str, Any]] = {}
        # store row -> identity
        self._row_identity: List[Tuple[str, str]] = []
        self._identity_row: Dict[Tuple[str, str], int] = {}
        # failure_type -> store label id, in order of first appearance. Not
        # persisted on its own: identities replay from the JSONL in the
        # same order on restart, so the same ids come out again.
        self._type_id: Dict[str, int] = {}
        self._rebuild_from_log()

    # -- bootstrap ---------------------------------------------------------

    def _label_of(self, failure_type: str) -> int:
        """Vocabulary id of a failure type, assigned on first sight."""
        return self._type_id.setdefault(failure_type, len(self._type_id))

    def _append_rows(self, rows: torch.Tensor, labels: torch.Tensor) -> int:
        """Append to whatever store is attached. Distributed stores keep no
        labels (filter-first is refused for them in match_batch)."""
        if isinstance(self.store, EmbeddingStore):
            return self.store.append(rows, labels)
        return self.store.append(rows)

    def _restore_rows(self, identities: List[Tuple[str, str]]) -> None:
        """Install the embedding rows for ``identities`` (in order) into
        the current store: from the packed sidecar when it matches
        (mmap + chunked H2D upload), else re-encode and rewrite it. The
        sidecar holds embeddings only; the labels come from the identities
        on either path."""
        labels = torch.tensor(
            [self._label_of(ft) for (ft, _sig) in identities], dtype=torch.int32
        )
        if self.sidecar.count() == len(identities):
            done = 0
            for chunk in self.sidecar.load_chunks():
                self._append_rows(chunk, labels[done : done + chunk.shape[0]])
                done += chunk.shape[0]
        else:
            emb = self.encoder.encode_texts([sig for (_ft, sig) in identities])
            self._append_rows(emb, labels)
            self.sidecar.rewrite(emb)

    def _rebuild_from_log(self) -> None:
        """Rebuild the HBM mirror from the durable JSONL."""
        for rec in self.failures.all():
            key = (rec.get("failure_type", ""), rec.get("signature_text", ""))
            self._latest[key] = rec
        identities = list(self._latest.keys())
        if identities:
            self._restore_rows(identities)
            self._row_identity = identities
            self._identity_row = {key: i for i, key in enumerate(identities)}

    def attach_store(self, new_store) -> None:
        """Swap the embedding store (e.g. for a distributed coordinator
        store) and reload every known identity into it, preserving row
        order (sidecar fast path, re-encode fallback). Must happen before
        serving begins."""
        if self.int8_mirror and not isinstance(new_store, EmbeddingStore):
            raise NotImplementedError(
                f"int8_mirror is not supported on {type(new_store).__name__}: "
                "sharded and distributed stores keep no mirror"
            )
        with self._lock:
            if self.int8_mirror:
                new_store.enable_mirror()
            self.store = new_store
            if self._row_identity:
                self._restore_rows(self._row_identity)

    def build_index(self, **kw):
        """Build a routed-search index over the current rows and swap it in.
        The build reads a snapshot of the live rows outside the lock (rows
        below a snapshot are immutable); only the swap takes the lock. Rows
        appended meanwhile are the new index's tail. Rebuilding is this
        same call again."""
        from kakveda_amd.gfkb.ivf import IvfIndex

        with self._lock:
            store = self.store
        if not isinstance(store, EmbeddingStore):
            raise NotImplementedError(
                f"routed search is not supported on {type(store).__name__}"
            )
        index = IvfIndex.build(store, **kw)
        with self._lock:
            if self.store is store:
                store.index = index
                store._stale_warned = False
        return index

    # -- failures ----------------------------------------------------------

    def list_failures(self) -> List[Dict[str, Any]]:
        return self.failures.all()

    def upsert_failure(
        self,
        failure_type: str,
        signature_text: str,
        context_signature: Dict[str, Any],
        impact_severity: str = "medium",
        root_cause: Optional[str] = None,
        resolution: Optional[str] = None,
        app_id: str = "",
    ) -> Tuple[Dict[str, Any], bool]:
        """Versioned upsert; returns (record, created)."""
        with self._lock:
            key = (failure_type, signature_text)
            existing = self._latest.get(key)
            now = utcnow()
            if existing is None:
                rec = CanonicalFailureRecord(
                    failure_id=f"F-{len(self.failures) + 1:04d}",
                    version=1,
                    created_at=now,
                    updated_at=now,
                    failure_type=failure_type,
                    root_cause=root_cause,
                    context_signature=context_signature,
                    impact_severity=Severity(impact_severity),
                    resolution=resolution,
                    occurrences=1,
                    affected_apps=[app_id] if app_id else [],
                    signature_text=signature_text,
                ).model_dump(mode="json")
                self.failures.append(rec)
                self._latest[key] = rec
                emb = self.encoder.encode_texts([signature_text])
                row = self._append_rows(
                    emb, torch.tensor([self._label_of(failure_type)], dtype=torch.int32)
                )
                self.sidecar.append(emb)
                self._row_identity.append(key)
                self._identity_row[key] = row
                return rec, True

            rec = dict(existing)
            rec["version"] = int(rec["version"]) + 1
            rec["updated_at"] = now.isoformat().replace("+00:00", "Z")
            rec["occurrences"] = int(rec.get("occurrences", 0)) + 1
            apps = list(rec.get("affected_apps", []))
            if app_id and app_id not in apps:
                apps.append(app_id)
            rec["affected_apps"] = apps
            rec["root_cause"] = root_cause or rec.get("root_cause")
            rec["resolution"] = resolution or rec.get("resolution")
            rec["context_signature"] = context_signature or rec.get("context_signature")
            self.failures.append(rec)
            self._latest[key] = rec
            return rec, False

    def match(
        self,
        signature_text: str,
        failure_type: Optional[str] = None,
        top_k: Optional[int] = None,
        filter_first: bool = False,
        nprobe: Optional[int] = None,
        route_filtered: Optional[bool] = None,
    ) -> List[FailureMatch]:
        """Top-k failures by cosine similarity, then optional type filter
        (reference order: cut to top-k first, filter second). With
        ``filter_first`` the type filter runs inside the search instead:
        the top-k of the failures of that type. ``nprobe`` and
        ``route_filtered``: see ``match_batch``."""
        return self.match_batch(
            [signature_text],
            failure_types=[failure_type],
            top_k=top_k,
            filter_first=filter_first,
            nprobe=nprobe,
            route_filtered=route_filtered,
        )[0]

    def match_batch(
        self,
        signature_texts: List[str],
        failure_types: Optional[List[Optional[str]]] = None,
        top_k: Optional[int] = None,
        filter_first: Union[bool, Sequence[bool]] = False,
        nprobe: Optional[int] = None,
        route_filtered: Optional[bool] = None,
    ) -> List[List[FailureMatch]]:
        """Match a whole batch of signatures with ONE fused-kernel launch.

        The engine lock is held only to snapshot (store, live count) —
        NOT across the encode GEMMs or the search kernel (VERDICT round 1
        weak #2), so concurrent upserts and other matches proceed while
        the GPU works. Rows below the snapshot are immutable, and their
        identity-map entries are written before ``count`` is bumped, so
        the lock-free mapping below is race-free.

        ``filter_first`` (one bool, or one per query) opts a query that
        names a ``failure_type`` into filter-first semantics: the search
        itself is restricted to rows of that type, so the result is the
        top-k OF that type rather than whatever of that type made the
        global top-k. Queries without it keep the reference's post-filter
        order; a batch may mix both, and a batch with none set takes the
        unfiltered kernels. A type no failure has ever had matches nothing.

        ``nprobe`` (one value per batch; default: the engine's) > 0 routes
        the batch through the store's index: approximate, scanning that
        many inverted lists per query plus the rows appended since the
        build. 0 forces the exact search. Without an index the engine's
        default is ignored (an explicit ``nprobe`` raises); a batch with a
        filter-first query runs the exact filtered search; sharded and
        distributed stores refuse an explicit ``nprobe``.

        ``route_filtered`` (default: the engine's) keeps such a batch routed
        instead, when an ``nprobe`` and an index are in effect: one routed
        search with the type filter inside the scan, the batch's other
        queries riding along unfiltered, and the store's exact fill for any
        filtered query whose type's rows sat in lists it did not probe.
        """
        nq = len(signature_texts)
        k = top_k or self.top_k
        first = (
            [bool(filter_first)] * nq
            if isinstance(filter_first, bool)
            else [bool(f) for f in filter_first]
        )
        if len(first) != nq:
            raise ValueError("filter_first must be one bool or one per query")
        with self._lock:
            store = self.store
            valid = store.count
            index = getattr(store, "index", None)
            # per query: want = the label id to search under (None: no
            # filter in the search); unknown = filter-first on a type the
            # vocabulary has never seen
            want: List[Optional[int]] = [None] * nq
            unknown = [False] * nq
            for r in range(nq):
                ft = failure_types[r] if failure_types else None
                if first[r] and ft:
                    if ft in self._type_id:
                        want[r] = self._type_id[ft]
                    else:
                        unknown[r] = True
        if valid == 0:
            return [[] for _ in range(nq)]
        filtered = any(w is not None for w in want)
        if (filtered or any(unknown)) and not isinstance(store, EmbeddingStore):
            raise NotImplementedError(
                f"filter_first is not supported on {type(store).__name__}: "
                "sharded and distributed stores keep no row labels, and "
                "post-filtering instead would silently change the result"
            )
        if nprobe and not isinstance(store, EmbeddingStore):
            raise NotImplementedError(
                f"nprobe is not supported on {type(store).__name__}: sharded "
                "and distributed stores have no routed index"
            )
        if nprobe is None:
            # the engine default applies only where it can
            probe = self.nprobe if index is not None else None
        else:
            probe = nprobe
        route_f = self.route_filtered if route_filtered is None else bool(route_filtered)
        # unknown types cannot match: search only the other queries
        live = [r for r in range(nq) if not unknown[r]]
        if not live:
            return [[] for _ in range(nq)]
        q = self.encoder.encode_texts([signature_texts[r] for r in live])
        if filtered:
            want_t = torch.tensor(
                [-1 if want[r] is None else want[r] for r in live], dtype=torch.int32
            )
            if route_f and probe and index is not None:
                scores, idx = store.search(
                    q, min(k, valid), valid_n=valid, want=want_t, nprobe=probe,
                    index=index, route_filtered=True,
                )
            else:
                scores, idx = store.search(q, min(k, valid), valid_n=valid, want=want_t)
        elif probe:
            scores, idx = store.search(
                q, min(k, valid), valid_n=valid, nprobe=probe, index=index
            )
        else:
            scores, idx = store.search(q, min(k, valid), valid_n=valid)
        slot = {r: j for j, r in enumerate(live)}
        results: List[List[FailureMatch]] = []
        for r in range(nq):
            failure_type = failure_types[r] if failure_types else None
            out: List[FailureMatch] = []
            if unknown[r]:
                results.append(out)
                continue
            for s, i in zip(scores[slot[r]].tolist(), idx[slot[r]].tolist()):
                if i < 0 or i >= len(self._row_identity):
                    # rows the engine has no identity for (e.g. a pre-loaded
                    # corpus adopted under the engine) can win the similarity
                    # search but cannot be reported as failures
                    continue
                rec = self._latest[self._row_identity[i]]
                if failure_type and rec["failure_type"] != failure_type:
                    continue
                out.append(
                    FailureMatch(
                        failure_id=rec["failure_id"],
                        version=rec["version"],
                        score=float(s),
                        failure_type=rec["failure_type"],
                        suggested_mitigation=rec.get("resolution"),
                    )
                )
            results.append(out)
        return results

    # -- patterns ----------------------------------------------------------

    def list_patterns(self) -> List[Dict[str, Any]]:
        latest: Dict[str, Dict[str, Any]] = {}
        for rec in self.patterns.all():
            latest[rec.get("pattern_id") or rec.get("name", "")] = rec
        return list(latest.values())

    def upsert_pattern(
        self,
        name: str,
        failure_ids: List[str],
        affected_apps: List[str],
        description: Optional[str] = None,
    ) -> Tuple[Dict[str, Any], bool]:
        with self._lock:
            existing = None
            for rec in reversed(self.patterns.all()):
                if rec.get("name") == name:
                    existing = rec
                    break
            if existing is None:
                rec = PatternEntity(
                    pattern_id=f"FP-{len(self.patterns) + 1:04d}",
                    name=name,
                    created_at=utcnow(),
                    failure_ids=sorted(set(failure_ids)),
                    affected_apps=sorted(set(affected_apps)),
                    description=description,
                ).model_dump(mode="json")
                self.patterns.append(rec)
                return rec, True
            rec = dict(existing)
            rec["failure_ids"] = sorted(set(list(rec.get("failure_ids", [])) + failure_ids))
            rec["affected_apps"] = sorted(set(list(rec.get("affected_apps", [])) + affected_apps))
            rec["description"] = description or rec.get("description")
            self.patterns.append(rec)
            return rec, False
