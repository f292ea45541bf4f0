"""MI355XRetriever: drop-in replacement of QdrantRetriever (src/audio_rag/retrieval/qdrant.py).

Same constructor (config, embedding_dim), same methods and semantics:
  add(chunks, embeddings, collection_name)                      qdrant.py:140-225
  search(query_embedding, top_k, collection_name, filter_metadata, search_type)  qdrant.py:227-352
  delete_collection / count / collection_exists / is_hybrid_collection         qdrant.py:134-138, 354-381
The ranking arithmetic runs on the GPU through libarmi (dense cosine, sparse dot, RRF); nothing
falls back to the CPU. search_batch() is the batched device API the pipeline and bench use.
"""

from __future__ import annotations

import hashlib
import json
import logging
import threading
from dataclasses import dataclass

import numpy as np
import torch

from audio_rag_amd.config.schema import RetrievalConfig
from audio_rag_amd.core.base import (AudioChunk, BaseRetriever, EmbeddingResult, RetrievalResult,
                                     SparseVector)
from audio_rag_amd.core.exceptions import RetrievalError
from audio_rag_amd.retrieval.base import RetrievalRegistry
from audio_rag_amd.retrieval.collection import ChunkCollection
from audio_rag_amd.retrieval.device import ConcurrentHybrid, TopK
from audio_rag_amd.utils.decorators import timed

logger = logging.getLogger(__name__)


@dataclass
class QueryBatch:
    """B queries on the device: dense fp16 [B, dim] and an optional sparse CSR."""

    dense: torch.Tensor
    sparse_indptr: torch.Tensor | None = None   # int32 [B+1]
    sparse_indices: torch.Tensor | None = None  # int32
    sparse_values: torch.Tensor | None = None   # float32

    @property
    def has_sparse(self) -> bool:
        return self.sparse_indptr is not None


def sparse_arrays(sv: SparseVector | None) -> tuple[np.ndarray, np.ndarray] | None:
    """SparseVector -> (ascending int32 indices, float32 values). Qdrant stores sparse vectors
    sorted by index; duplicate indices are rejected like Qdrant does."""
    if sv is None:
        return None
    idx = np.asarray(sv.indices, dtype=np.int64)
    val = np.asarray(sv.values, dtype=np.float32)
    if idx.shape != val.shape:
        raise ValueError("sparse vector indices and values differ in length")
    order = np.argsort(idx, kind="stable")
    idx, val = idx[order], val[order]
    if idx.size and (np.any(idx[1:] == idx[:-1]) or idx[0] < 0 or idx[-1] >= 2**31):
        raise ValueError("sparse vector indices must be unique non-negative int32")
    return idx.astype(np.int32), val


MAX_QUERY_TERMS = 256  # armi_sparse_topk's per-query term capacity (include/armi.h)


def query_sparse_arrays(sv: SparseVector | None) -> tuple[np.ndarray, np.ndarray] | None:
    """sparse_arrays for a query vector, refusing more terms than the device search scores (it
    would silently use only the first 256; Qdrant uses every term)."""
    arr = sparse_arrays(sv)
    if arr is not None and arr[0].size > MAX_QUERY_TERMS:
        raise ValueError(f"sparse query has {arr[0].size} terms; the MI355X sparse search takes at "
                         f"most {MAX_QUERY_TERMS}")
    return arr


def filter_key(f: dict | None):
    """The identity of a metadata filter (None for no filter): queries with equal keys share one
    search."""
    return None if not f else tuple(sorted((k, repr(v)) for k, v in f.items()))


@dataclass
class FilterGroup:
    """The queries of one search_batch call that carry one filter, and the planner's choice."""

    filter: dict | None
    queries: list
    matches: int = -1       # rows the filter matches (-1: not counted, the knob is off / no filter)
    rowlist: bool = False   # ranked from the matching rows (armi_*_rowlist_topk), else a masked scan
    qmask: bool = False     # its masked scan is shared with the other qmask groups of the call
    #                         (armi_dense_topk_qmask; sparse mode: armi_sparse_topk_qmask), else a
    #                         masked search of its own


QMASK_MODES = ("dense", "legacy_dense", "hybrid")
QMASK_MAX_QUERIES = 128  # queries of one armi_dense_topk_qmask call (sparse mode cuts alike)


def plan_filter_groups(filters: list, n_rows: int, knob: int, count_matches,
                       query_masks: bool = False, mode: str = "dense", tail_rows: int = 0,
                       qmask_supported=None, sparse_masks: bool = False,
                       tail_masks: bool = False) -> list[FilterGroup]:
    """Groups the queries of a batch by filter (in order of first appearance) and picks each
    group's path. A group of q queries whose filter matches m of the collection's n_rows rows is
    ranked from its row list iff the knob is on (filter_list_rows > 0), m <= knob and
    2 * q * m <= n_rows: byte parity, the list path reads at most 2 B per component, row and
    query (fp16 rows, once per query), the masked scan at least 1 B per component and row (the
    int8 image, once per pass of up to 64 queries), so a chosen list never reads more than the scan
    it replaces. An empty match list always qualifies (count 0). Queries without a filter, and
    every group the rule refuses, take the masked scan. count_matches(filter) -> m is asked only
    with the knob on. For a live collection m and n_rows count both segments.

    Then the groups left to the masked scan, the unfiltered one included, are marked `qmask`:
    their dense scans become one scan of the int8 image per 64 queries in which every query
    carries its own mask (DenseIndex.topk_masks). All of: query_masks (the filter_query_masks knob)
    on, at least two such groups (one group is one masked search already), mode dense /
    legacy_dense / hybrid, no tail rows unless tail_masks (the filter_query_masks_live knob: the
    live tail pass then takes the masks too, TailIndex.tail_topk_masks) and
    qmask_supported(queries of a call) -> bool (the dense index's answer for the leg's k: an int8
    image, k <= 64). Otherwise they stay one masked search per group.

    Mode sparse has its own rule: sparse_masks (the filter_query_masks_sparse knob) on, at least
    two such groups and no tail rows unless tail_masks (armi_sparse_tail_topk takes one mask,
    TailSparseIndex.tail_topk_masks one per query). The sparse form (SparseIndex.topk_masks) has no
    shape limit, so neither query_masks nor qmask_supported is consulted. tail_masks alone marks
    nothing."""
    groups: dict = {}
    for i, f in enumerate(filters):
        g = groups.get(filter_key(f))
        if g is None:
            g = groups[filter_key(f)] = FilterGroup(f or None, [])
        g.queries.append(i)
    for g in groups.values():
        if knob > 0 and g.filter:
            g.matches = int(count_matches(g.filter))
            g.rowlist = g.matches <= knob and 2 * len(g.queries) * g.matches <= n_rows
    rest = [g for g in groups.values() if not g.rowlist]
    no_tail = tail_rows == 0 or tail_masks
    if query_masks and len(rest) >= 2 and mode in QMASK_MODES and no_tail and \
            qmask_supported is not None:
        n = sum(len(g.queries) for g in rest)
        if qmask_supported(min(n, QMASK_MAX_QUERIES)):
            for g in rest:
                g.qmask = True
    if mode == "sparse" and sparse_masks and len(rest) >= 2 and no_tail:
        for g in rest:
            g.qmask = True
    return list(groups.values())


def qmask_calls(groups: list[FilterGroup], limit: int = QMASK_MAX_QUERIES) -> list[tuple]:
    """The topk_masks calls that serve the qmask groups of a plan: their queries in the groups'
    order, cut into calls of at most `limit`; per call (query indexes, filters, q_mask): the
    distinct filters of the call's queries in order of first appearance (the rows of the stacked
    mask tensor) and, per query, its filter's row or -1 for no filter. Queries that repeat a
    filter share its row."""
    pairs = [(i, g.filter) for g in groups if g.qmask for i in g.queries]
    calls = []
    for lo in range(0, len(pairs), limit):
        rows: dict = {}
        filters, q_mask = [], []
        for _, f in pairs[lo:lo + limit]:
            if not f:
                q_mask.append(-1)
                continue
            key = filter_key(f)
            if key not in rows:
                rows[key] = len(filters)
                filters.append(f)
            q_mask.append(rows[key])
        calls.append(([i for i, _ in pairs[lo:lo + limit]], filters, q_mask))
    return calls


def fp16_rows(vectors: list[list[float]] | np.ndarray, dim: int) -> np.ndarray:
    a = np.asarray(vectors, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError(f"dense vectors must have dimension {dim}, got shape {a.shape}")
    return a.astype(np.float16)


class _QueryGraph:
    """One unfiltered single-query search of a collection, captured as a HIP graph for one
    (branch, top_k): the query's dense fp16 vector and sparse terms (<= 256) are written into a
    pinned staging buffer and sent in one host->device copy, the graph replays every search
    kernel (dense scan / merge / second pass, the sparse chain on its side stream, RRF) plus the
    packing of (count, ids, scores) into one fp64 row, and one device->host copy brings that row
    back. The eager path launches the same kernels one Python call at a time, with a copy per
    input array and a packing step per result."""

    def __init__(self, ret: "MI355XRetriever", coll: ChunkCollection, mode: str, top_k: int):
        dev, dim = ret.device, coll.dim
        self.indexes = coll.segments()  # the graph's kernels read them
        self.mode, self.k, self.dim = mode, top_k, dim
        self.lock = threading.Lock()
        off_ptr = dim * 2
        off_idx = off_ptr + 16
        off_val = off_idx + 4 * MAX_QUERY_TERMS
        total = off_val + 4 * MAX_QUERY_TERMS
        self.host = torch.zeros(total, dtype=torch.uint8, pin_memory=True)
        self.stage = torch.zeros(total, dtype=torch.uint8, device=dev)
        h = self.host.numpy()
        self.h_dense = h[:off_ptr].view(np.float16)
        self.h_ptr = h[off_ptr:off_ptr + 8].view(np.int32)
        self.h_idx = h[off_idx:off_val].view(np.int32)
        self.h_val = h[off_val:].view(np.float32)
        d = self.stage
        batch = QueryBatch(dense=d[:off_ptr].view(torch.float16).view(1, dim))
        if mode in ("hybrid", "sparse"):
            batch = QueryBatch(dense=batch.dense, sparse_indptr=d[off_ptr:off_ptr + 8].view(torch.int32),
                               sparse_indices=d[off_idx:off_val].view(torch.int32),
                               sparse_values=d[off_val:].view(torch.float32))
        self.out_host = torch.zeros(1 + 2 * top_k, dtype=torch.float64, pin_memory=True)

        def run():
            out = ret._search_device(coll, batch, top_k, mode, None)
            sc = out.rank if mode == "hybrid" else out.scores
            return torch.cat([out.count[:1].double(), out.ids[0].double(), sc[0].double()])

        # captured under inference mode, as the reranker's graphs are (xlmr.py forward): the
        # CUDA generator's graph-state tensors are created by the first capture in a process and
        # updated in place by every later one, which torch refuses across the two modes. The
        # warm-up query is a one-hot vector with no sparse terms: the all-zero staging buffer
        # ties every row at cosine 0, whose top-k cannot be certified, and each warm-up call then
        # ran the collect pass over the whole shard (~0.16 s at 1M rows)
        batch.dense[0, 0] = 1.0
        with torch.inference_mode():
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):
                    run()
            torch.cuda.current_stream(dev).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.packed = run()

    def search(self, dense, sparse: tuple[np.ndarray, np.ndarray] | None) -> np.ndarray:
        """The packed result row (count, ids[k], scores[k]) of one query."""
        with self.lock:
            self.h_dense[:] = dense
            if sparse is not None:
                n = sparse[0].size
                self.h_ptr[0], self.h_ptr[1] = 0, n
                self.h_idx[:n] = sparse[0]
                self.h_val[:n] = sparse[1]
            stream = torch.cuda.current_stream(self.stage.device)
            self.stage.copy_(self.host, non_blocking=True)
            self.graph.replay()
            self.out_host.copy_(self.packed, non_blocking=True)
            stream.synchronize()
            return self.out_host.numpy().copy()


@RetrievalRegistry.register("mi355x")
class MI355XRetriever(BaseRetriever):
    """Dense (cosine), sparse (lexical) and hybrid (RRF) search on an MI355X chunk store."""

    def __init__(self, config: RetrievalConfig, embedding_dim: int = 1024):
        self.config = config
        self.embedding_dim = embedding_dim
        self.device = torch.device("cuda", config.device)
        self._collections: dict[str, ChunkCollection] = {}
        self._hybrid: ConcurrentHybrid | None = None
        self._graphs_ok = True  # cleared when a capture is refused (search() then runs eagerly)
        self.last_sharded = None  # the ShardedSearch of the last collective call (diagnostics)
        self.last_plan: list[FilterGroup] | None = None  # the last planned call's groups (same)
        self._enc_cache: dict = {}  # (filter, queries) -> (row lists, their encoding): one group
        # num_gpus > 1: the corpus is sharded by ordinal over the ranks of the default process
        # group (one process per GPU, launched by torchrun, torch.distributed initialised and
        # the process's GPU selected before the retriever is built): see _search_sharded
        self._rank, self._world = 0, 1
        if config.num_gpus > 1:
            import torch.distributed as dist

            if not dist.is_available() or not dist.is_initialized():
                raise RetrievalError("num_gpus > 1 needs torch.distributed initialised (one "
                                     "process per GPU, e.g. torchrun) before the retriever")
            if dist.get_world_size() != config.num_gpus:
                raise RetrievalError(f"num_gpus = {config.num_gpus} but the process group has "
                                     f"{dist.get_world_size()} ranks")
            self._rank, self._world = dist.get_rank(), dist.get_world_size()
            self.device = torch.device("cuda", torch.cuda.current_device())
        logger.info(f"MI355XRetriever initialized: collection={config.collection_name}, "
                    f"search_type={config.search_type}, device={self.device}")

    # ---------------------------------------------------------------------- collections

    def _resolve_collection(self, collection_name: str | None) -> str:
        return collection_name or self.config.collection_name

    def _ensure_collection(self, collection_name: str | None = None, hybrid: bool = False) -> str:
        """Creates a missing collection (hybrid = dense + sparse named vectors, else dense-only
        legacy schema), as qdrant.py:59-132 does."""
        resolved = self._resolve_collection(collection_name)
        coll = self._collections.get(resolved)
        if coll is not None:
            if hybrid and not coll.hybrid:
                logger.warning(f"Collection {resolved} exists but is not hybrid-enabled. "
                               "Re-index required for hybrid search.")
            return resolved
        try:
            coll = ChunkCollection(resolved, self.embedding_dim, hybrid, self.device)
            coll.shard = (self._rank, self._world)
            coll.live_tail_rows = self.config.live_tail_rows
            self._collections[resolved] = coll
            logger.info(f"Creating {'hybrid' if hybrid else 'dense'} collection: {resolved}")
            return resolved
        except Exception as e:
            raise RetrievalError(f"Failed to ensure collection '{resolved}': {e}")

    def is_hybrid_collection(self, collection_name: str | None = None) -> bool:
        resolved = self._ensure_collection(collection_name)
        return self._collections[resolved].hybrid

    def delete_collection(self, collection_name: str | None = None) -> None:
        resolved = self._resolve_collection(collection_name)
        try:
            coll = self._collections.pop(resolved, None)
            if coll is not None:
                coll.close()
            logger.info(f"Deleted collection: {resolved}")
        except Exception as e:
            raise RetrievalError(f"Failed to delete collection '{resolved}': {e}")

    def count(self, collection_name: str | None = None) -> int:
        resolved = self._ensure_collection(collection_name)
        return self._collections[resolved].count

    def collection_exists(self, collection_name: str | None = None) -> bool:
        return self._resolve_collection(collection_name) in self._collections

    def collection(self, collection_name: str | None = None) -> ChunkCollection:
        return self._collections[self._ensure_collection(collection_name)]

    # ------------------------------------------------------------------------------ add

    @timed
    def add(self, chunks: list[AudioChunk], embeddings: list[EmbeddingResult],
            collection_name: str | None = None) -> None:
        if not chunks:
            return
        if len(chunks) != len(embeddings):
            raise RetrievalError(f"Chunks/embeddings mismatch: {len(chunks)} chunks, "
                                 f"{len(embeddings)} embeddings")
        has_sparse = any(e.sparse is not None for e in embeddings)
        resolved = self._ensure_collection(collection_name, hybrid=has_sparse)
        try:
            coll = self._collections[resolved]
            dense = fp16_rows([e.dense for e in embeddings], self.embedding_dim)
            if coll.hybrid and not self.config.reproduce_sparse_drop:
                sparse = [sparse_arrays(e.sparse) for e in embeddings]
            else:
                # legacy collections keep dense only; with reproduce_sparse_drop the reference's
                # final dense-only batch upsert (qdrant.py:210-220) replaces every point, so the
                # stored points have no sparse vector
                sparse = [None] * len(embeddings)
            payloads = [{"text": c.text, "start": c.start, "end": c.end, "speaker": c.speaker,
                         "metadata": c.metadata or {}} for c in chunks]
            coll.upsert(dense, sparse, payloads)
            logger.info(f"Added {len(chunks)} chunks to {resolved} (hybrid={coll.hybrid})")
        except Exception as e:
            raise RetrievalError(f"Failed to add chunks to '{resolved}': {e}")

    def add_arrays(self, dense: np.ndarray, payloads: list[dict],
                   sparse: list[tuple[np.ndarray, np.ndarray] | None] | None = None,
                   collection_name: str | None = None) -> None:
        """Bulk upsert of pre-embedded chunks (fp16 [n, dim] + payload dicts), the fast ingest
        path for large corpora."""
        resolved = self._ensure_collection(collection_name, hybrid=sparse is not None)
        coll = self._collections[resolved]
        if sparse is None or not coll.hybrid:
            sparse = [None] * len(payloads)
        coll.upsert(np.ascontiguousarray(dense, dtype=np.float16), sparse, payloads)

    # ---------------------------------------------------------------------- persistence

    def save_collection(self, path, collection_name: str | None = None) -> None:
        """Persists a collection as an on-disk chunk store (retrieval/store.py), the durable
        form of the Qdrant collection qdrant.py:59-225 maintains."""
        resolved = self._resolve_collection(collection_name)
        if resolved not in self._collections:
            raise RetrievalError(f"Collection '{resolved}' does not exist")
        try:
            self._collections[resolved].save(path)
        except Exception as e:
            raise RetrievalError(f"Failed to save collection '{resolved}': {e}")

    def attach_collection(self, coll: ChunkCollection) -> None:
        """Registers a collection built elsewhere (ChunkCollection.from_indexes)."""
        old = self._collections.pop(coll.name, None)
        if old is not None and old is not coll:
            old.close()
        self._collections[coll.name] = coll

    def load_collection(self, path, collection_name: str | None = None) -> str:
        """Loads an on-disk chunk store as a collection (replacing one of the same name);
        returns the collection name."""
        try:
            from audio_rag_amd.retrieval.store import read_meta

            resolved = collection_name or read_meta(path)["name"]
            coll = ChunkCollection.load(path, self.device, resolved)
            coll.shard = (self._rank, self._world)
            coll.live_tail_rows = self.config.live_tail_rows
        except Exception as e:
            raise RetrievalError(f"Failed to load chunk store '{path}': {e}")
        old = self._collections.pop(resolved, None)
        if old is not None:
            old.close()
        self._collections[resolved] = coll
        logger.info(f"Loaded collection {resolved}: {coll.count} points (hybrid={coll.hybrid})")
        return resolved

    # --------------------------------------------------------------------------- search

    def _mode(self, coll: ChunkCollection, search_type: str, has_sparse: bool) -> str:
        if search_type == "hybrid" and coll.hybrid and has_sparse:
            return "hybrid"
        if search_type == "sparse" and coll.hybrid and has_sparse:
            return "sparse"
        return "dense" if coll.hybrid else "legacy_dense"

    def search_batch(self, queries: QueryBatch, top_k: int | None = None,
                     collection_name: str | None = None,
                     filter_metadata: dict | list | None = None,
                     search_type: str | None = None) -> tuple[TopK, str]:
        """Device top-k for B queries; returns (TopK, mode). Scores are cosine (dense),
        sparse dot (sparse) or the RRF score (hybrid), as Qdrant's hit.score. filter_metadata: one
        filter for every query, or a list of one `dict | None` per query (the reference's API
        takes one filter per request, api/v1/query.py:41). With config.filter_list_rows > 0 the
        queries are grouped by filter and selective groups are ranked from their matching rows
        (plan_filter_groups); with config.filter_query_masks the groups left to the masked scan
        share one dense scan per 64 queries, each query under its own mask, and with
        config.filter_query_masks_sparse one sparse search per call as well. The answers do not
        depend on the path, only TopK.flags tell (ARMI_FLAG_ROWLIST, ARMI_FLAG_QMASK). With
        num_gpus > 1 the knobs are ignored and the list form refused."""
        resolved = self._ensure_collection(collection_name)
        top_k = top_k or self.config.top_k
        search_type = search_type or self.config.search_type
        coll = self._collections[resolved]
        mode = self._mode(coll, search_type, queries.has_sparse)
        per_query = isinstance(filter_metadata, (list, tuple))
        if self._world > 1:
            if per_query:
                raise RetrievalError("one filter per query needs num_gpus = 1: the collective "
                                     "search of a sharded corpus agrees on one filter per call")
            mask = coll.filter_mask(filter_metadata)
            return self._search_sharded(coll, queries, top_k, mode, mask, filter_metadata), mode
        b = int(queries.dense.shape[0])
        if per_query and len(filter_metadata) != b:
            raise RetrievalError(f"{len(filter_metadata)} filters for {b} queries")
        if not per_query and (self.config.filter_list_rows == 0 or not filter_metadata):
            return self._search_device(coll, queries, top_k, mode,
                                       coll.segment_masks(filter_metadata)), mode
        filters = list(filter_metadata) if per_query else [filter_metadata] * b
        return self._search_planned(coll, queries, top_k, mode, filters), mode

    def _search_planned(self, coll: ChunkCollection, queries: QueryBatch, top_k: int, mode: str,
                        filters: list) -> TopK:
        """search_batch with one filter per query: the planner's groups (plan_filter_groups), all
        row-list groups in one dense and one sparse launch per segment, the qmask groups in one
        dense scan per 64 queries (_search_qmask), every other group by the masked search, one
        call per group; the results scattered back in query order with their flags
        (ARMI_FLAG_ROWLIST on the row-list queries, ARMI_FLAG_QMASK from the kernel)."""
        from audio_rag_amd._armi import ARMI_FLAG_ROWLIST

        seg = coll.segments()
        b = int(queries.dense.shape[0])
        knob = self.config.filter_list_rows
        tail_rows = seg.tail.n_rows if seg.tail is not None else 0
        n_rows = seg.dense.n_rows + tail_rows
        leg_k = 2 * top_k if mode == "hybrid" else top_k
        groups = plan_filter_groups(filters, n_rows, knob,
                                    lambda f: coll.segment_row_lists(f, knob)[2],
                                    query_masks=self.config.filter_query_masks, mode=mode,
                                    tail_rows=tail_rows,
                                    qmask_supported=lambda n: seg.dense.qmask_supported(n, leg_k),
                                    sparse_masks=self.config.filter_query_masks_sparse,
                                    tail_masks=self.config.filter_query_masks_live)
        self.last_plan = groups
        if len(groups) == 1 and not groups[0].rowlist:  # one masked search, as without a plan
            return self._search_device(coll, queries, top_k, mode,
                                       coll.segment_masks(groups[0].filter))
        parts = []  # (query indexes, their TopK, flag bits to add)
        listed = [g for g in groups if g.rowlist]
        if listed:
            idx = [i for g in listed for i in g.queries]
            out = self._search_rowlists(seg, self._select(queries, idx), top_k, mode,
                                        *self._encode_rowlists(coll, listed))
            parts.append((idx, out, ARMI_FLAG_ROWLIST))
        for idx, flt, q_mask in qmask_calls(groups):
            out = self._search_qmask(coll, seg, self._select(queries, idx), top_k, mode, flt, q_mask)
            parts.append((idx, out, 0))
        for g in groups:
            if not g.rowlist and not g.qmask:
                out = self._search_device(coll, self._select(queries, g.queries), top_k, mode,
                                          coll.segment_masks(g.filter))
                parts.append((g.queries, out, 0))
        return self._scatter(parts, b)

    def _select(self, queries: QueryBatch, idx: list) -> QueryBatch:
        """The queries idx of a batch as a batch of their own, built on the device without reading
        anything back: the term arrays keep the whole batch's length (an upper bound), filled up to
        the new indptr's end."""
        if idx == list(range(int(queries.dense.shape[0]))):
            return queries
        dev = queries.dense.device
        it = torch.tensor(idx, dtype=torch.int64, device=dev)
        dense = queries.dense.index_select(0, it)
        if not queries.has_sparse:
            return QueryBatch(dense=dense)
        ptr = queries.sparse_indptr.to(torch.int64)
        starts = ptr[:-1][it]
        new_ptr = torch.zeros(len(idx) + 1, dtype=torch.int64, device=dev)
        torch.cumsum(ptr[1:][it] - starts, 0, out=new_ptr[1:])
        cap = int(queries.sparse_indices.numel())
        indices, values = queries.sparse_indices, queries.sparse_values
        if cap and idx:
            pos = torch.arange(cap, dtype=torch.int64, device=dev)
            j = (torch.searchsorted(new_ptr, pos, right=True) - 1).clamp_(0, len(idx) - 1)
            src = (starts[j] + (pos - new_ptr[j])).clamp_(0, cap - 1)
            indices, values = indices[src], values[src]
        return QueryBatch(dense=dense, sparse_indptr=new_ptr.to(torch.int32),
                          sparse_indices=indices, sparse_values=values)

    def _encode_rowlists(self, coll: ChunkCollection, groups: list[FilterGroup]):
        """The row lists of the groups' filters in the kernels' encoding, per segment: (main, tail),
        each (list_ptr, list_rows, q_list, longest list) on the device with one list per group and
        the queries in the groups' order; tail None when the collection has no tail rows."""
        dev = self.device
        lists = [coll.segment_row_lists(g.filter, self.config.filter_list_rows) for g in groups]
        # one group (search(), a batch under one filter): the encoding is kept with the lists it
        # was made from, so a repeated filter uploads nothing
        one = (self._enc_cache.get((filter_key(groups[0].filter), len(groups[0].queries)))
               if len(groups) == 1 else None)
        if one is not None and one[0] is lists[0]:
            return one[1]
        q_list = torch.from_numpy(np.repeat(np.arange(len(groups), dtype=np.int32),
                                            [len(g.queries) for g in groups])).to(dev)

        def encode(which: int):
            rows = [ls[which] for ls in lists]
            if any(r is None for r in rows):
                return None
            ptr = np.zeros(len(rows) + 1, dtype=np.int64)
            np.cumsum([r.numel() for r in rows], out=ptr[1:])
            return (torch.from_numpy(ptr).to(dev), torch.cat(rows), q_list,
                    max(r.numel() for r in rows))

        enc = encode(0), encode(1)
        if len(groups) == 1:
            if len(self._enc_cache) >= 1024:
                self._enc_cache.clear()
            key = (filter_key(groups[0].filter), len(groups[0].queries))
            self._enc_cache[key] = (lists[0], enc)
        return enc

    def _search_rowlists(self, seg, queries: QueryBatch, top_k: int, mode: str, main: tuple,
                         tail: tuple | None) -> TopK:
        """The row-list groups of a planned call (_encode_rowlists' lists, the queries in the same
        order): one dense and one sparse launch per segment, the segments' lists merged exactly
        (merge_shards: rank = the exact key), hybrid through the same RRF.
        Device work only (graph-capturable)."""
        from audio_rag_amd.retrieval.device import merge_shards

        live = tail is not None and tail[3] > 0  # no tail match: the main lists are the answer
        sq = (queries.sparse_indptr, queries.sparse_indices, queries.sparse_values)

        def merged(a: TopK, t: TopK, k: int) -> TopK:
            m = merge_shards(torch.stack([a.rank, t.rank]), torch.stack([a.scores, t.scores]),
                             torch.stack([a.ids, t.ids]), torch.stack([a.count, t.count]), k)
            m.flags = a.flags
            return m

        def dense(k: int) -> TopK:
            d = seg.dense.topk_rows(queries.dense, k, *main)
            return merged(d, seg.tail.topk_rows(queries.dense, k, *tail), k) if live else d

        def sparse(k: int) -> TopK:
            s = seg.sparse.topk_rows(*sq, k, *main)
            return merged(s, seg.tail_sparse.topk_rows(*sq, k, *tail), k) if live else s

        if mode == "hybrid":
            if self._hybrid is None:
                self._hybrid = ConcurrentHybrid(self.device)
            extra = main[:3] + (tail[:3] if live else ())
            return self._hybrid(lambda: dense(2 * top_k), lambda: sparse(2 * top_k), sq + extra,
                                top_k, rrf_k=self.config.rrf_k)
        if mode == "sparse":
            return sparse(top_k)
        return dense(top_k)

    def _search_qmask(self, coll: ChunkCollection, seg, queries: QueryBatch, top_k: int, mode: str,
                      filters: list, q_mask: list) -> TopK:
        """One qmask_calls call (<= 128 queries, in that call's order): the dense leg is one
        DenseIndex.topk_masks over the stacked masks of `filters`, mode sparse one
        SparseIndex.topk_masks over them. Hybrid's sparse leg is that call too with
        config.filter_query_masks_sparse, else one masked SparseIndex.topk per distinct filter,
        scattered into the call's order; one RRF fuses the two legs for the whole call (RRF is per
        query). A collection with tail rows (the planner lets it in with
        config.filter_query_masks_live) follows every main list with the fused tail pass over the
        stacked tail masks (TailIndex / TailSparseIndex.tail_topk_masks), the per-filter sparse
        searches with tail_topk under the filter's tail mask; an empty tail launches nothing."""
        dev = self.device
        live = seg.tail is not None and seg.tail.n_rows > 0
        masks = [coll.segment_masks(f) for f in filters]  # (main, tail; tail None when not live)

        def stack(which: int, n_rows: int) -> torch.Tensor:
            if masks:
                return torch.stack([m[which] for m in masks])
            return torch.empty((0, max((n_rows + 63) // 64, 1)), dtype=torch.int64, device=dev)

        stacked = stack(0, seg.dense.n_rows)
        tstacked = stack(1, seg.tail.n_rows) if live else None
        qm = torch.tensor(q_mask, dtype=torch.int32, device=dev)

        def dense(k: int) -> TopK:
            d = seg.dense.topk_masks(queries.dense, k, stacked, qm)
            return seg.tail.tail_topk_masks(queries.dense, k, d, tstacked, qm) if live else d

        sq = (queries.sparse_indptr, queries.sparse_indices, queries.sparse_values)

        def sparse_masks(k: int) -> TopK:
            s = seg.sparse.topk_masks(*sq, k, stacked, qm)
            return seg.tail_sparse.tail_topk_masks(*sq, k, s, tstacked, qm) if live else s

        if mode == "sparse":
            return sparse_masks(top_k)
        if mode != "hybrid":
            return dense(top_k)
        if self._hybrid is None:
            self._hybrid = ConcurrentHybrid(self.device)
        stacks = (stacked, qm) + ((tstacked,) if live else ())
        if self.config.filter_query_masks_sparse:
            return self._hybrid(lambda: dense(2 * top_k), lambda: sparse_masks(2 * top_k),
                                sq + stacks, top_k, rrf_k=self.config.rrf_k)
        by_mask: dict = {}
        for i, m in enumerate(q_mask):
            by_mask.setdefault(m, []).append(i)

        def sparse(k: int) -> TopK:
            parts = []
            for m, idx in by_mask.items():
                sub = self._select(queries, idx)
                sub_q = (sub.sparse_indptr, sub.sparse_indices, sub.sparse_values)
                mask, tmask = (None, None) if m < 0 else masks[m]
                s = seg.sparse.topk(*sub_q, k, row_mask=mask)
                if live:
                    s = seg.tail_sparse.tail_topk(*sub_q, k, s, row_mask=tmask)
                parts.append((idx, s, 0))
            return self._scatter(parts, len(q_mask))

        each = tuple(t for m in masks for t in m if t is not None)
        return self._hybrid(lambda: dense(2 * top_k), lambda: sparse(2 * top_k),
                            sq + each + stacks, top_k, rrf_k=self.config.rrf_k)

    def _scatter(self, parts: list, b: int) -> TopK:
        """One TopK in query order from the groups' results: parts = (query indexes, TopK, flag
        bits the group adds). Only the tensors every part holds are copied (the others convert on
        access, TopK); flags are always present."""
        dev = self.device
        if len(parts) == 1 and parts[0][0] == list(range(b)):  # one group: nothing to reorder
            _, out, bits = parts[0]
            if out.flags is None:
                out.flags = torch.full((b,), bits, dtype=torch.int32, device=dev)
            elif bits:
                out.flags |= bits
            return out
        names = [n for n in ("_scores", "ids", "_rank", "count")
                 if all(getattr(p, n) is not None for _, p, _ in parts)]
        first = parts[0][1]
        out = TopK(flags=torch.zeros(b, dtype=torch.int32, device=dev))
        for n in names:
            t = getattr(first, n)
            setattr(out, n, torch.empty((b,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev))
        for idx, p, bits in parts:
            it = torch.tensor(idx, dtype=torch.int64, device=dev)
            for n in names:
                getattr(out, n).index_copy_(0, it, getattr(p, n))
            flags = p.flags | bits if p.flags is not None else torch.full(
                (len(idx),), bits, dtype=torch.int32, device=dev)
            out.flags.index_copy_(0, it, flags.to(torch.int32))
        return out

    def _search_sharded(self, coll: ChunkCollection, queries: QueryBatch, top_k: int, mode: str,
                        mask: torch.Tensor | None, mask_spec: dict | None = None) -> TopK:
        """search_batch over the corpus sharded across the process group (num_gpus > 1), a
        COLLECTIVE call: every rank calls it with its own queries (any batch size, any branch)
        and the same top_k, collection and filter, and gets the global top-k of its own queries.
        retrieval/shards.ShardedSearch: one RCCL all-gather of all ranks' queries, the local
        kernels over this rank's shard for all of them, one all-gather of the per-shard lists,
        the merge of this rank's queries (armi_topk_merge_shards_packed), RRF after the merge
        for hybrid. Keys are exact and tie-broken by the global ordinal, so the answer equals
        the single-GPU one. Reranking stays local: each rank reranks its own queries' candidates
        (the query slice), with no further exchange."""
        from audio_rag_amd.retrieval.device import merge_shards, merge_shards_packed, rrf_fuse
        from audio_rag_amd.retrieval.shards import ShardedSearch

        sh = ShardedSearch(lambda q, k: coll.dense_index.topk(q, k, row_mask=mask), merge_shards,
                           local_sparse=(lambda c, k: coll.sparse_index.topk(*c, k, row_mask=mask))
                           if coll.hybrid else None,
                           rrf=lambda a, b, k: rrf_fuse(a, b, k, rrf_k=self.config.rrf_k),
                           merge_packed=merge_shards_packed)
        self.last_sharded = sh
        csr = (queries.sparse_indptr, queries.sparse_indices, queries.sparse_values)
        # the ranks agree on top_k and on collection + filter through the call's header (a
        # mismatch raises on every rank); batch sizes and branches may differ
        key = json.dumps([coll.name, coll.count, coll.hybrid, mask_spec or {}],
                         sort_keys=True, default=str)
        digest = int.from_bytes(hashlib.sha256(key.encode()).digest()[:8], "little")
        try:
            return sh.search(queries.dense, csr if queries.has_sparse else None, mode, top_k,
                             digest)
        except ValueError as e:
            raise RetrievalError(str(e))

    def _search_device(self, coll: ChunkCollection, queries: QueryBatch, top_k: int, mode: str,
                       masks: tuple | None) -> TopK:
        """The device work of search_batch for a resolved collection and branch. masks:
        ChunkCollection.segment_masks (main mask, tail mask) or None. Both segments of a live
        collection are searched, dense and sparse alike: the main top-k followed by the fused
        tail pass (TailIndex.tail_topk, TailSparseIndex.tail_topk); an empty tail adds no
        kernel."""
        seg = coll.segments()
        mask, tmask = masks if masks is not None else (None, None)
        live = seg.tail is not None and seg.tail.n_rows > 0
        sq = (queries.sparse_indptr, queries.sparse_indices, queries.sparse_values)

        def dense(k: int) -> TopK:
            d = seg.dense.topk(queries.dense, k, row_mask=mask)
            return seg.tail.tail_topk(queries.dense, k, d, row_mask=tmask) if live else d

        def sparse(k: int) -> TopK:
            s = seg.sparse.topk(*sq, k, row_mask=mask)
            return seg.tail_sparse.tail_topk(*sq, k, s, row_mask=tmask) if live else s

        if mode == "hybrid":
            if self._hybrid is None:
                self._hybrid = ConcurrentHybrid(self.device)
            extra = tuple(m for m in (mask, tmask) if m is not None)
            return self._hybrid(lambda: dense(2 * top_k), lambda: sparse(2 * top_k), sq + extra,
                                top_k, rrf_k=self.config.rrf_k)
        if mode == "sparse":
            return sparse(top_k)
        return dense(top_k)

    def to_query_batch(self, query_embeddings: list[EmbeddingResult]) -> QueryBatch:
        dense = torch.from_numpy(fp16_rows([q.dense for q in query_embeddings],
                                           self.embedding_dim)).to(self.device)
        if any(q.sparse is None for q in query_embeddings):
            return QueryBatch(dense=dense)
        parts = [query_sparse_arrays(q.sparse) for q in query_embeddings]
        indptr = np.zeros(len(parts) + 1, dtype=np.int32)
        np.cumsum([len(p[0]) for p in parts], out=indptr[1:])
        # one unused entry past indptr[-1] keeps the term arrays' device pointers non-null when
        # every query is an empty SparseVector (the C ABI refuses null arrays)
        idx = np.concatenate([p[0] for p in parts] + [np.zeros(1, np.int32)]).astype(np.int32)
        val = np.concatenate([p[1] for p in parts] + [np.zeros(1, np.float32)]).astype(np.float32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        return QueryBatch(dense=dense, sparse_indptr=t(indptr), sparse_indices=t(idx),
                          sparse_values=t(val))

    def materialize(self, out: TopK, mode: str, resolved: str, b: int = 0,
                    threshold: float | None = None) -> list[RetrievalResult]:
        """Row b of a device TopK -> fresh RetrievalResult objects from the payload table
        (qdrant.py:334-346)."""
        coll = self._collections[resolved]
        # one packed device-to-host copy (count, ids, scores as fp64: ordinals < 2^31 and fp32
        # scores convert exactly) instead of three synchronising copies
        sc = out.rank if mode == "hybrid" else out.scores
        packed = torch.cat([out.count[b:b + 1].double(), out.ids[b].double(),
                            sc[b].double()]).cpu().numpy()
        k = out.ids.shape[1]
        count = int(packed[0])
        ids = packed[1:1 + count].astype(np.int64).tolist()
        scores = packed[1 + k:1 + k + count].tolist()
        results = []
        for pid, score in zip(ids, scores):
            if threshold is not None and score < threshold:
                continue
            p = coll.payloads[pid]
            chunk = AudioChunk(text=p.get("text", ""), start=p.get("start", 0.0),
                               end=p.get("end", 0.0), speaker=p.get("speaker"),
                               metadata=p.get("metadata"))
            results.append(RetrievalResult(chunk=chunk, score=float(score), source=resolved))
        return results

    def materialize_batch(self, out: TopK, mode: str, resolved: str,
                          threshold: float | None = None) -> list[list[RetrievalResult]]:
        """Every row of a device TopK -> RetrievalResult lists, with one device-to-host copy per
        tensor for the whole batch (materialize() copies per row)."""
        coll = self._collections[resolved]
        counts = out.count.cpu().tolist()
        ids = out.ids.cpu().tolist()
        scores = (out.rank if mode == "hybrid" else out.scores).cpu().tolist()
        batch = []
        for c, row_ids, row_sc in zip(counts, ids, scores):
            results = []
            for pid, score in zip(row_ids[:c], row_sc[:c]):
                if threshold is not None and score < threshold:
                    continue
                p = coll.payloads[pid]
                chunk = AudioChunk(text=p.get("text", ""), start=p.get("start", 0.0),
                                   end=p.get("end", 0.0), speaker=p.get("speaker"),
                                   metadata=p.get("metadata"))
                results.append(RetrievalResult(chunk=chunk, score=float(score), source=resolved))
            batch.append(results)
        return batch

    def _graph_search(self, coll: ChunkCollection, query: EmbeddingResult, top_k: int,
                      search_type: str) -> tuple[np.ndarray, str] | None:
        """search() of one unfiltered query through the collection's captured graph for its
        branch (captured on first use); None when the path does not apply."""
        if not (self.config.query_graphs and self._graphs_ok) or coll.count == 0 or self._world > 1:
            return None
        mode = self._mode(coll, search_type, query.sparse is not None)
        sparse = query_sparse_arrays(query.sparse) if mode in ("hybrid", "sparse") else None
        dense = np.asarray(query.dense, dtype=np.float32)
        if dense.shape != (self.embedding_dim,):
            raise ValueError(f"dense vectors must have dimension {self.embedding_dim}, "
                             f"got shape {(1,) + dense.shape}")
        graphs = coll.query_graphs()
        key = (mode, top_k, self.config.rrf_k)
        g = graphs.get(key)
        if g is None:
            try:
                g = _QueryGraph(self, coll, mode, top_k)
            except RuntimeError as e:  # capture refused: the same kernels through search_batch
                logger.warning(f"query graph capture failed ({e}); searching without graphs")
                self._graphs_ok = False
                return None
            graphs[key] = g
        return g.search(dense, sparse), mode

    def _materialize_packed(self, packed: np.ndarray, resolved: str, k: int,
                            threshold: float | None) -> list[RetrievalResult]:
        coll = self._collections[resolved]
        count = int(packed[0])
        ids = packed[1:1 + count].astype(np.int64).tolist()
        scores = packed[1 + k:1 + k + count].tolist()
        results = []
        for pid, score in zip(ids, scores):
            if threshold is not None and score < threshold:
                continue
            p = coll.payloads[pid]
            chunk = AudioChunk(text=p.get("text", ""), start=p.get("start", 0.0),
                               end=p.get("end", 0.0), speaker=p.get("speaker"),
                               metadata=p.get("metadata"))
            results.append(RetrievalResult(chunk=chunk, score=float(score), source=resolved))
        return results

    @timed
    def search(self, query_embedding: EmbeddingResult, top_k: int | None = None,
               collection_name: str | None = None, filter_metadata: dict | None = None,
               search_type: str | None = None) -> list[RetrievalResult]:
        resolved = self._ensure_collection(collection_name)
        top_k = top_k or self.config.top_k
        search_type = search_type or self.config.search_type
        try:
            if not filter_metadata:
                coll = self._collections[resolved]
                got = self._graph_search(coll, query_embedding, top_k, search_type)
                if got is not None:
                    packed, mode = got
                    thr = None
                    if mode == "legacy_dense" and self.config.score_threshold > 0:
                        thr = self.config.score_threshold
                    results = self._materialize_packed(packed, resolved, top_k, thr)
                    logger.debug(f"Search returned {len(results)} results")
                    return results
            batch = self.to_query_batch([query_embedding])
            out, mode = self.search_batch(batch, top_k, resolved, filter_metadata, search_type)
            thr = None
            if mode == "legacy_dense" and self.config.score_threshold > 0:
                thr = self.config.score_threshold
            results = self.materialize(out, mode, resolved, 0, thr)
            logger.debug(f"Search returned {len(results)} results")
            return results
        except Exception as e:
            raise RetrievalError(f"Search failed in '{resolved}': {e}")


# The reference's own configs name the backend "qdrant" (configs/base.yaml:39,
# config/schema.py:60); in this package that key builds the MI355X chunk store, so a reference
# deployment's YAML runs unchanged (the qdrant_host / qdrant_port / qdrant_in_memory knobs are
# accepted and ignored).
RetrievalRegistry.register("qdrant")(MI355XRetriever)
