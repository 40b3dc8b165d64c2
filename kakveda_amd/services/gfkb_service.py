"""GFKB HTTP service fronting the GfkbEngine.

Endpoint parity with /root/reference/services/gfkb/app.py:74-198:
GET /failures, POST /failures/match, POST /failures/upsert,
GET /patterns, POST /patterns/upsert. The engine behind them is the
HBM-resident embedding store + fused cosine-topk kernel (gfkb/engine.py)
instead of a per-request TF-IDF refit.
"""

from __future__ import annotations

import logging
import os
import queue
import threading
from typing import Any, Dict, List, Optional

from fastapi import FastAPI
from pydantic import BaseModel, Field

from kakveda_amd.core.schemas import (
    FailureMatchRequest,
    FailureMatchResponse,
    Severity,
)
from kakveda_amd.gfkb.engine import GfkbEngine

logger = logging.getLogger(__name__)


class MatchBatcher:
    """Coalesces concurrent /failures/match requests into one fused-kernel
    launch (serving concurrency).

    Adaptive batching with zero added idle latency: the collector thread
    blocks for the first request, then drains whatever else is queued at
    that instant (requests naturally accumulate while the previous
    batch's kernel is in flight) — a single client sees one thread-hop,
    N concurrent clients share one engine.match_batch launch instead of
    serialising N kernel launches behind the engine lock.
    """

    def __init__(self, engine: GfkbEngine, max_batch: int = 256):
        self.engine = engine
        self.max_batch = max_batch
        self._q: "queue.SimpleQueue" = queue.SimpleQueue()
        self._thread: Optional[threading.Thread] = None
        self._start_lock = threading.Lock()
        self.batches = 0  # observability: launches issued
        self.requests = 0  # requests served through the batcher

    def _ensure_thread(self) -> None:
        if self._thread is None or not self._thread.is_alive():
            with self._start_lock:
                if self._thread is None or not self._thread.is_alive():
                    self._thread = threading.Thread(
                        target=self._loop, name="gfkb-match-batcher", daemon=True
                    )
                    self._thread.start()

    def match(
        self,
        signature_text: str,
        failure_type: Optional[str] = None,
        filter_first: bool = False,
        exact: bool = False,
        top_k: Optional[int] = None,
    ):
        self._ensure_thread()
        item: Dict[str, Any] = {
            "text": signature_text,
            "ftype": failure_type,
            "first": filter_first,
            "exact": exact,
            "top_k": top_k,
            "ev": threading.Event(),
            "res": None,
            "err": None,
        }
        self._q.put(item)
        if not item["ev"].wait(timeout=120.0):
            raise TimeoutError("match batcher timed out")
        if item["err"] is not None:
            raise item["err"]
        return item["res"]

    def _loop(self) -> None:
        while True:
            batch = [self._q.get()]
            while len(batch) < self.max_batch:
                try:
                    batch.append(self._q.get_nowait())
                except queue.Empty:
                    break
            # At most two engine calls per batch: the requests without a
            # top_k go in exactly the call made before the field existed,
            # those with one in a second call at their largest top_k.
            plain = [b for b in batch if b.get("top_k") is None]
            asked = [b for b in batch if b.get("top_k") is not None]
            for group, run in ((plain, self._run_plain), (asked, self._run_top_k)):
                if not group:
                    continue
                try:
                    run(group)
                except Exception as exc:  # surfaced to every waiting request
                    for b in group:
                        b["err"] = exc
                self.batches += 1
            self.requests += len(batch)
            for b in batch:
                b["ev"].set()

    def _extra(self, batch) -> Dict[str, Any]:
        first = [b["first"] for b in batch]
        # an all-unset batch makes the call it always made
        extra: Dict[str, Any] = {"filter_first": first} if any(first) else {}
        # one request asking for exact makes its whole batch exact.
        # A routed batch needs no cap on its size: from
        # ops.IVF_BATCHED_MIN_B queries on the store takes the
        # list-major scan, which gathers a probed list once per 16
        # queries and stays below the exact search's time
        if any(b["exact"] for b in batch):
            extra["nprobe"] = 0
        return extra

    def _run_plain(self, batch) -> None:
        results = self.engine.match_batch(
            [b["text"] for b in batch], [b["ftype"] for b in batch], **self._extra(batch)
        )
        for b, r in zip(batch, results):
            b["res"] = r

    def _run_top_k(self, batch) -> None:
        """One call at the largest top_k of the group; each result is cut to
        its own. The reference's order holds per request: cut to top_k first,
        then drop other types. So only a filter-first request hands its type
        to the engine (the type is then applied inside the search, and the
        best top_k of that type are a prefix of the best of the call); every
        other request is searched untyped and filtered here, after its cut."""
        k = max(int(b["top_k"]) for b in batch)
        types = [b["ftype"] if b["first"] else None for b in batch]
        results = self.engine.match_batch(
            [b["text"] for b in batch], types, top_k=k, **self._extra(batch)
        )
        for b, r in zip(batch, results):
            r = r[: int(b["top_k"])]
            if b["ftype"] and not b["first"]:
                r = [m for m in r if m.failure_type == b["ftype"]]
            b["res"] = r


class UpsertFailureRequest(BaseModel):
    failure_type: str
    root_cause: Optional[str] = None
    context_signature: Dict[str, Any] = Field(default_factory=dict)
    impact_severity: Severity = Severity.medium
    resolution: Optional[str] = None
    signature_text: str
    app_id: str


class UpsertPatternRequest(BaseModel):
    name: str
    failure_ids: List[str]
    affected_apps: List[str]
    description: Optional[str] = None


def _setup_routed(engine: GfkbEngine, config: Optional[Any]) -> None:
    """Apply the ``gfkb.routed`` config block: when enabled, build the routed
    index at start-up if the store is big enough, make its ``nprobe`` the
    engine default and its ``filtered`` flag the engine's ``route_filtered``.
    Disabled (the default) touches nothing."""
    if config is None:
        from kakveda_amd.core.config import ConfigStore

        config = ConfigStore()
    routed = config.get("gfkb.routed", {}) or {}
    if not routed.get("enabled", False):
        return
    rows = engine.store.count
    min_rows = int(routed.get("min_rows", 65536) or 0)
    if rows < max(min_rows, 1):
        logger.info(
            "routed search enabled but the store has %d rows (< min_rows=%d): "
            "serving exact search",
            rows,
            min_rows,
        )
        return
    index = engine.build_index(n_lists=routed.get("n_lists"))
    engine.nprobe = int(routed.get("nprobe", 32))
    # filter_first requests stay routed too (with the store's exact fill);
    # off, a batch with one of them runs the exact filtered search
    engine.route_filtered = bool(routed.get("filtered", False))
    logger.info(
        "routed search on: nprobe=%d, filtered=%s, index %s",
        engine.nprobe,
        engine.route_filtered,
        index.stats,
    )


def _setup_featurize(engine: GfkbEngine, config: Optional[Any]) -> None:
    """Apply ``gfkb.device_featurize``: true turns the engine's encoder over
    to the device featurizer. False (the default) touches nothing, so an
    engine built with the flag keeps it."""
    if config is None:
        from kakveda_amd.core.config import ConfigStore

        config = ConfigStore()
    if bool(config.get("gfkb.device_featurize", False)):
        engine.encoder.device_featurize = True
        logger.info("device featurizer on")
    # gfkb.int8_mirror, likewise: true builds the mirror of the rows the
    # engine holds and keeps it on across store swaps; false touches nothing
    if bool(config.get("gfkb.int8_mirror", False)):
        from kakveda_amd.gfkb.engine import EmbeddingStore

        if not isinstance(engine.store, EmbeddingStore):
            raise NotImplementedError(
                f"gfkb.int8_mirror is not supported on {type(engine.store).__name__}"
            )
        engine.int8_mirror = True
        engine.store.enable_mirror()
        logger.info("int8 mirror on")


def create_app(
    data_dir: Optional[str] = None,
    device: Optional[str] = None,
    engine: Optional[GfkbEngine] = None,
    config: Optional[Any] = None,
) -> FastAPI:
    """``config`` is a ``ConfigStore`` (or anything with its ``get``); its
    ``gfkb.routed`` block opts the service into routed search, its
    ``gfkb.device_featurize`` flag into hashing texts on the device, its
    ``gfkb.int8_mirror`` flag into the int8 row mirror."""
    app = FastAPI(title="Kakveda-AMD GFKB")
    if engine is None:
        import torch

        dev = device or ("cuda" if torch.cuda.is_available() else "cpu")
        engine = GfkbEngine(
            data_dir=data_dir or os.environ.get("DATA_DIR", "/app/data"), device=dev
        )
    app.state.engine = engine
    _setup_routed(engine, config)
    _setup_featurize(engine, config)
    # micro-batcher on by default; KAKVEDA_MATCH_BATCHER=0 opts out
    batcher = (
        MatchBatcher(engine)
        if os.environ.get("KAKVEDA_MATCH_BATCHER", "1") == "1"
        else None
    )
    app.state.batcher = batcher

    # handlers are plain `def` so FastAPI runs them in its threadpool: the
    # engine is synchronous (GPU kernels, file appends) and must not block
    # the event loop — a slow match would stall every concurrent request
    # including /healthz (matches the reference's sync-handler behaviour)

    # anyio's default 40-token thread limiter caps how many requests can
    # be parked inside `match` waiting on the batcher, which caps the
    # micro-batch size and hence service throughput. Raise it so the
    # batcher, not the threadpool, sets the batch size. (The front-door
    # warn app registers the same hook: ASGITransport composition never
    # runs THIS app's lifespan.)
    @app.on_event("startup")
    async def _raise_threadpool():
        from kakveda_amd.services.wiring import raise_thread_limiter

        raise_thread_limiter()

    @app.get("/failures")
    def list_failures():
        return {"failures": engine.list_failures()}

    @app.post("/failures/match", response_model=FailureMatchResponse)
    def match(req: FailureMatchRequest):
        from kakveda_amd.core.metrics import observe_gfkb

        if batcher is not None:
            matches = batcher.match(
                req.signature_text,
                failure_type=req.failure_type,
                filter_first=req.filter_first,
                exact=req.exact,
                **({} if req.top_k is None else {"top_k": req.top_k}),
            )
        else:
            extra = {"nprobe": 0} if req.exact else {}
            if req.top_k is not None:
                extra["top_k"] = req.top_k
            matches = engine.match(
                req.signature_text,
                failure_type=req.failure_type,
                filter_first=req.filter_first,
                **extra,
            )
        observe_gfkb(engine.store.count, len(engine.failures))
        return FailureMatchResponse(matches=matches)

    @app.post("/failures/upsert")
    def upsert(req: UpsertFailureRequest):
        rec, created = engine.upsert_failure(
            failure_type=req.failure_type,
            signature_text=req.signature_text,
            context_signature=req.context_signature,
            impact_severity=req.impact_severity.value,
            root_cause=req.root_cause,
            resolution=req.resolution,
            app_id=req.app_id,
        )
        return {"ok": True, "created": created, "failure": rec}

    @app.get("/patterns")
    def list_patterns():
        return {"patterns": engine.list_patterns()}

    @app.post("/patterns/upsert")
    def upsert_pattern(req: UpsertPatternRequest):
        rec, created = engine.upsert_pattern(
            name=req.name,
            failure_ids=req.failure_ids,
            affected_apps=req.affected_apps,
            description=req.description,
        )
        return {"ok": True, "created": created, "pattern": rec}

    @app.get("/healthz")
    def healthz():
        from kakveda_amd.core.metrics import observe_gfkb

        observe_gfkb(engine.store.count, len(engine.failures))
        return {"ok": True, "failures": len(engine.failures), "rows": engine.store.count}

    return app
