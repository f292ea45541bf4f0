"""A chunk collection: host staging of upserted points plus their device indexes.

Replaces one Qdrant collection as QdrantRetriever creates and fills it
(src/audio_rag/retrieval/qdrant.py:59-132 _ensure_collection, 140-225 add):
  * named dense vector "dense" (size = embedding_dim, COSINE)      -> DenseIndex (fp16 rows)
  * named sparse vector "sparse" (hybrid collections only)         -> SparseIndex (CSR)
  * payload {text, start, end, speaker, metadata}                  -> host list
Points get consecutive ordinals in upsert order (the reference's uuid4 ids are never surfaced:
RetrievalResult carries no id, core/base.py:56-61). The device indexes are rebuilt lazily on the
first search after an add; a built index is read-only, so concurrent searches are safe, and a
rebuild never frees an index a running search still holds (the old handles die with their last
reference).

Live ingest (live_tail_rows > 0): after the first build, later upserts are flushed into a small
growable segment, the tail (TailIndex: fp16 rows; TailSparseIndex: the rows' forward CSR, appended
to on the device, with no inverted index of its own), which every search covers together with the
main indexes by the fused tail passes; the main indexes are not touched by a flush, and a flush
uploads the new points only.
When a flush would pass the tail's capacity the tail is folded into new main indexes built from
device-side concatenations (compact()). A flush changes the tail in place on the current stream:
searches on other streams must not overlap an upsert's first search.
"""

from __future__ import annotations

import threading
import weakref
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np
import torch

from audio_rag_amd.retrieval.device import DenseIndex, SparseIndex, TailIndex, TailSparseIndex

BGE_M3_VOCAB = 250002


_NO_MATCH = object()

# The device segments of a collection: the main indexes over ordinals [base, base + main_rows)
# and, in a live collection, the tail over the ordinals behind them (tail None or tail.n_rows == 0:
# nothing to search there; tail_sparse, a TailSparseIndex holding the same rows' forward CSR, None in
# a dense-only collection).
Segments = namedtuple("Segments", "dense sparse tail tail_sparse main_rows")


def mask_words(ok: np.ndarray) -> np.ndarray:
    """bool [n] -> uint64 bitmask words (bit r of word r // 64 = ok[r]), at least one word."""
    words = np.zeros(max((len(ok) + 63) // 64, 1), dtype=np.uint64)
    idx = np.nonzero(ok)[0]
    np.bitwise_or.at(words, idx >> 6, np.left_shift(np.uint64(1), (idx & 63).astype(np.uint64)))
    return words


def split_mask_words(ok: np.ndarray, main_rows: int) -> tuple[np.ndarray, np.ndarray]:
    """The per-segment row masks of a live collection: (main, tail) bitmask words of ok[:main_rows]
    and ok[main_rows:]. Each segment's bit 0 is its own first row, so the tail's words are not a
    suffix of the whole mask's words unless main_rows is a multiple of 64."""
    return mask_words(ok[:main_rows]), mask_words(ok[main_rows:])


def _canon(x):
    """The equivalence class _match_value compares a scalar in: bools only equal bools,
    integral numbers compare by value, non-integral floats never match, strings by value.
    None when the value needs the general comparison."""
    if isinstance(x, bool):
        return ("bool", x)
    if isinstance(x, int):
        return ("num", x)
    if isinstance(x, float):
        return ("num", int(x)) if x.is_integer() else _NO_MATCH
    if isinstance(x, str):
        return ("str", x)
    return None


def _match_value(field_value, wanted) -> bool:
    """Qdrant MatchValue: equality on keyword / integer / bool payload values; an array field
    matches when any element does."""
    if isinstance(field_value, list):
        return any(_match_value(v, wanted) for v in field_value)
    if isinstance(field_value, bool) or isinstance(wanted, bool):
        return isinstance(field_value, bool) and isinstance(wanted, bool) and field_value == wanted
    if isinstance(field_value, float) and not field_value.is_integer():
        return False
    return field_value == wanted


@dataclass
class ChunkCollection:
    name: str
    dim: int
    hybrid: bool
    device: torch.device
    # host staging
    dense_rows: list[np.ndarray] = field(default_factory=list)        # fp16 [n_i, dim] blocks
    sparse_rows: list[tuple[np.ndarray, np.ndarray] | None] = field(default_factory=list)
    payloads: list[dict] = field(default_factory=list)
    # device state
    _dense: DenseIndex | None = None
    _sparse: SparseIndex | None = None
    _built_rows: int = -1
    _mask_cache: dict = field(default_factory=dict)
    _key_index: dict = field(default_factory=dict)   # metadata key -> (count, {canon: ordinals})
    _lock: threading.Lock = field(default_factory=threading.Lock)
    _frozen: bool = False
    _servers: weakref.WeakSet = field(default_factory=weakref.WeakSet)  # open StreamServers
    # captured single-query searches over the current indexes (MI355XRetriever._graph_search),
    # dropped whenever the indexes are rebuilt or closed
    _graphs: dict = field(default_factory=dict)
    # (rank, world): this process's shard of the corpus when it is spread over `world` GPUs
    # (RetrievalConfig.num_gpus): every rank stages every point on the host and builds device
    # indexes over its contiguous ordinal range only (retrieval/shards.shard_range)
    shard: tuple = (0, 1)
    # live ingest (RetrievalConfig.live_tail_rows; 0 = rebuild on every add)
    live_tail_rows: int = 0
    _tail: TailIndex | None = None
    _tail_sparse: TailSparseIndex | None = None
    _main_rows: int = 0      # points held by the main indexes
    _vmax: int = -1          # largest sparse term id upserted so far
    _seg_mask_cache: dict = field(default_factory=dict)
    _seg_rows_cache: dict = field(default_factory=dict)   # filter key -> segment_row_lists

    def shard_bounds(self, n: int | None = None) -> tuple[int, int]:
        """[lo, hi) ordinals of this rank's shard of n (default: every) points."""
        from audio_rag_amd.retrieval.shards import shard_range

        return shard_range(self.count if n is None else n, self.shard[0], self.shard[1])

    @property
    def count(self) -> int:
        return len(self.payloads)

    # ------------------------------------------------------------------------------ upsert

    def upsert(self, dense: np.ndarray, sparse: list[tuple[np.ndarray, np.ndarray] | None],
               payloads: list[dict]) -> None:
        """dense: float16 [n, dim]; sparse[i]: (indices int32 ascending, values float32) or
        None; payloads: one dict per point."""
        if dense.dtype != np.float16 or dense.ndim != 2 or dense.shape[1] != self.dim:
            raise ValueError(f"dense vectors must be float16 [n, {self.dim}]")
        if not (len(sparse) == len(payloads) == dense.shape[0]):
            raise ValueError("dense / sparse / payload counts differ")
        if self._frozen:
            raise ValueError(f"collection {self.name} is read-only (built from device indexes)")
        bits = dense.view(np.uint16)
        if ((bits >> 10) & 31).max(initial=0) > 15:
            raise ValueError("dense components must be finite with |x| < 2 (unit embeddings)")
        with self._lock:
            self.dense_rows.append(np.ascontiguousarray(dense))
            self.sparse_rows.extend(sparse)
            self.payloads.extend(payloads)
            self._mask_cache.clear()
            self._seg_mask_cache.clear()
            self._seg_rows_cache.clear()
            self._key_index.clear()
            self._vmax = max([self._vmax] + [int(s[0].max(initial=-1)) for s in sparse
                                             if s is not None])

    # ------------------------------------------------------------------------------- build

    @property
    def _live(self) -> bool:
        return self.live_tail_rows > 0 and self.shard[1] == 1 and not self._frozen

    def _ensure_built(self) -> None:
        if self._built_rows == self.count:
            return
        with self._lock:
            if self._built_rows == self.count:
                return
            if self._live and self._dense is not None and self._built_rows >= 0:
                self._flush_live()
                return
            rows = (np.concatenate(self.dense_rows) if self.dense_rows
                    else np.zeros((0, self.dim), dtype=np.float16))
            lo, hi = self.shard_bounds()
            old_dense, old_sparse = self._dense, self._sparse
            self._graphs = {}
            self._dense = DenseIndex(torch.from_numpy(np.ascontiguousarray(rows[lo:hi])).to(self.device),
                                     ordinal_base=lo)
            if self.hybrid:
                mine = self.sparse_rows[lo:hi]
                indptr = np.zeros(hi - lo + 1, dtype=np.int64)
                lens = [0 if s is None else len(s[0]) for s in mine]
                np.cumsum(lens, out=indptr[1:])
                idx = np.concatenate([s[0] for s in mine if s is not None] or
                                     [np.zeros(0, np.int32)]).astype(np.int32)
                val = np.concatenate([s[1] for s in mine if s is not None] or
                                     [np.zeros(0, np.float32)]).astype(np.float32)
                # the vocabulary of the whole corpus: every shard answers the same term ids
                vmax = max((int(s[0].max(initial=-1)) for s in self.sparse_rows if s is not None),
                           default=-1)
                vocab = max(BGE_M3_VOCAB, vmax + 1)
                t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
                self._sparse = SparseIndex(t(indptr), t(idx), t(val), vocab, ordinal_base=lo)
            self._built_rows = self._main_rows = self.count
            self._tail = self._tail_sparse = None
            # The superseded indexes are not closed here: a search that fetched them before
            # this rebuild may still be using them. Dropping the reference frees each one (its
            # __del__ closes it) once the last such search lets go of it.
            del old_dense, old_sparse

    # ------------------------------------------------------------------------- live ingest

    def _upload(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _host_csr(self, lo: int, hi: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(indptr int64, indices int32, values float32) of points [lo, hi)."""
        mine = self.sparse_rows[lo:hi]
        indptr = np.zeros(hi - lo + 1, dtype=np.int64)
        np.cumsum([0 if s is None else len(s[0]) for s in mine], out=indptr[1:])
        idx = np.concatenate([s[0] for s in mine if s is not None] or
                             [np.zeros(0, np.int32)]).astype(np.int32)
        val = np.concatenate([s[1] for s in mine if s is not None] or
                             [np.zeros(0, np.float32)]).astype(np.float32)
        return indptr, idx, val

    def _host_dense(self, lo: int, hi: int) -> np.ndarray:
        """fp16 rows of points [lo, hi) from the staged blocks (only the blocks they touch)."""
        out, at = [], 0
        for blk in self.dense_rows:
            n = blk.shape[0]
            if at + n > lo and at < hi:
                out.append(blk[max(lo - at, 0):hi - at])
            at += n
        return np.concatenate(out) if out else np.zeros((0, self.dim), dtype=np.float16)

    def _tail_capacity(self) -> int:
        # twice the nominal size: a batch that arrives at a nearly full tail still lands in it
        return 2 * self.live_tail_rows

    def _fold(self, dense_parts: list, csr_parts: list) -> None:
        """New main indexes over the main rows followed by the given device blocks (fp16 row
        blocks; (indptr, indices, values) CSRs with indptr starting at 0): device-side
        concatenations, nothing read from the host staging. The superseded objects die with
        their last reference."""
        old = (self._dense, self._sparse)
        rows = torch.cat([self._dense.rows, *dense_parts]) if dense_parts else self._dense.rows
        self._dense = DenseIndex(rows, ordinal_base=0)
        if self.hybrid:
            sp = old[1]
            indptr, idx, val = [sp.indptr], [sp.indices], [sp.values]
            end = sp.indptr[-1:]
            for p, i, v in csr_parts:
                indptr.append(p[1:] + end)
                end = indptr[-1][-1:] if p.numel() > 1 else end
                idx.append(i)
                val.append(v)
            self._sparse = SparseIndex(torch.cat(indptr), torch.cat(idx), torch.cat(val),
                                       max(BGE_M3_VOCAB, self._vmax + 1), ordinal_base=0)
        self._main_rows = int(rows.shape[0])
        self._seg_mask_cache.clear()
        self._seg_rows_cache.clear()
        del old

    def _flush_live(self) -> None:
        """Brings the points upserted since the last build into the tail (lock held): uploads
        only their fp16 rows and their CSR and appends both (no native sparse index is built
        here). When they would not fit, the tail is folded into the main indexes first (and the new
        points with it when they alone exceed a tail)."""
        lo, hi = self._built_rows, self.count
        self._graphs = {}
        new = self._upload(self._host_dense(lo, hi))
        cap = self._tail_capacity()
        tail_rows = self._tail.n_rows if self._tail is not None else 0
        if tail_rows + (hi - lo) > cap:
            dense_parts = list(self._tail.parts) if tail_rows else []
            csr_parts = []
            if self.hybrid and tail_rows:
                ts = self._tail_sparse
                csr_parts.append((ts.indptr, ts.indices, ts.values))
            fits = hi - lo <= cap
            if not fits:
                dense_parts.append(new)
                if self.hybrid:
                    csr_parts.append(tuple(self._upload(a) for a in self._host_csr(lo, hi)))
            self._fold(dense_parts, csr_parts)
            self._tail = self._tail_sparse = None
            if not fits:
                self._built_rows = hi
                return
        if self._tail is None:
            self._tail = TailIndex(self.dim, cap, self._main_rows, self.device)
        self._tail.append(new)
        if self.hybrid:
            if self._tail_sparse is None:
                self._tail_sparse = TailSparseIndex(self._main_rows, self.device)
            self._tail_sparse.append(*(self._upload(a) for a in self._host_csr(lo, hi)),
                                     vocab=max(BGE_M3_VOCAB, self._vmax + 1))
        self._built_rows = hi

    def compact(self) -> None:
        """Folds the tail into the main indexes now (device-side concatenations; the tail starts
        empty afterwards). Nothing to do without a tail."""
        self._ensure_built()
        with self._lock:
            if self._tail is None or self._tail.n_rows == 0:
                return
            self._graphs = {}
            csr = []
            if self.hybrid:
                ts = self._tail_sparse
                csr.append((ts.indptr, ts.indices, ts.values))
            self._fold(list(self._tail.parts), csr)
            self._tail = self._tail_sparse = None

    def segments(self) -> Segments:
        """The device segments every search has to cover (see Segments)."""
        self._ensure_built()
        with self._lock:
            return Segments(self._dense, self._sparse, self._tail, self._tail_sparse,
                            self._main_rows)

    def segment_masks(self, filter_metadata: dict | None):
        """filter_mask per segment: (main mask, tail mask) device bitmasks, the tail's bit 0 being
        the tail's first row; None without a filter."""
        if not filter_metadata:
            return None
        seg = self.segments()
        if seg.tail is None or seg.tail.n_rows == 0:
            return self.filter_mask(filter_metadata), None
        key = tuple(sorted((k, repr(v)) for k, v in filter_metadata.items()))
        cached = self._seg_mask_cache.get(key)
        if cached is not None and cached[0] == (self.count, seg.main_rows):
            return cached[1]
        n = self.count
        ok = np.ones(n, dtype=bool)
        for k, v in filter_metadata.items():
            ok &= self._key_matches(k, v, n)
        masks = tuple(torch.from_numpy(w.view(np.int64)).to(self.device)
                      for w in split_mask_words(ok, seg.main_rows))
        self._seg_mask_cache[key] = ((n, seg.main_rows), masks)
        return masks

    def segment_row_lists(self, filter_metadata: dict, max_rows: int | None = None):
        """filter_rows per segment, for the row-list searches (DenseIndex.topk_rows):
        (main rows, tail rows, matches), the first two int32 device tensors of ascending local rows
        (main: ordinal - the main indexes' ordinal base; tail: ordinal - main_rows, None without a
        tail), matches their total over this rank's rows. A filter matching more than max_rows rows
        is only counted (both lists None: its search will be a masked scan). Cached per filter
        like segment_masks, and dropped with it (an upsert, a fold, a compaction)."""
        seg = self.segments()
        live = seg.tail is not None and seg.tail.n_rows > 0
        key = tuple(sorted((k, repr(v)) for k, v in filter_metadata.items()))
        state = (self.count, seg.main_rows, live)
        cached = self._seg_rows_cache.get(key)
        if cached is not None and cached[0] == state and (
                cached[1][0] is not None or (max_rows is not None and cached[1][2] > max_rows)):
            return cached[1]
        rows = self.filter_rows(filter_metadata)
        if not live:
            lo, hi = self.shard_bounds(self.count)
            rows = rows[np.searchsorted(rows, lo):np.searchsorted(rows, hi)]
        if max_rows is not None and len(rows) > max_rows:
            lists = (None, None, len(rows))
            self._seg_rows_cache[key] = (state, lists)
            return lists
        if live:
            cut = int(np.searchsorted(rows, seg.main_rows))
            parts = (rows[:cut], rows[cut:] - seg.main_rows)
        else:
            parts = (rows - lo, None)
        up = lambda a: None if a is None else torch.from_numpy(a.astype(np.int32)).to(self.device)
        lists = (up(parts[0]), up(parts[1]), sum(len(a) for a in parts if a is not None))
        self._seg_rows_cache[key] = (state, lists)
        return lists

    def query_graphs(self) -> dict:
        """The captured single-query searches of the current indexes (key -> graph)."""
        self._ensure_built()
        return self._graphs

    @property
    def dense_index(self) -> DenseIndex:
        """One index holding every point (a live collection folds its tail in first; live-aware
        code uses segments())."""
        self.compact()
        return self._dense

    @property
    def sparse_index(self) -> SparseIndex | None:
        self.compact()
        return self._sparse

    # ------------------------------------------------------------------------------ filter

    def filter_mask(self, filter_metadata: dict | None) -> torch.Tensor | None:
        """Bitmask (int64 words on the device) of points whose payload metadata matches every
        condition: Filter(must=[FieldCondition(key=f"metadata.{k}", match=MatchValue(v))])
        (qdrant.py:263-269). Bit r = row r of this rank's shard (ordinal lo + r)."""
        if not filter_metadata:
            return None
        key = tuple(sorted((k, repr(v)) for k, v in filter_metadata.items()))
        cached = self._mask_cache.get(key)
        if cached is not None and cached[0] == self.count:
            return cached[1]
        n = self.count
        ok = np.ones(n, dtype=bool)
        for k, v in filter_metadata.items():
            ok &= self._key_matches(k, v, n)
        lo, hi = self.shard_bounds(n)
        ok = ok[lo:hi]
        words = np.zeros(max((hi - lo + 63) // 64, 1), dtype=np.uint64)
        idx = np.nonzero(ok)[0]
        np.bitwise_or.at(words, idx >> 6, np.left_shift(np.uint64(1), (idx & 63).astype(np.uint64)))
        mask = torch.from_numpy(words.view(np.int64)).to(self.device)
        self._mask_cache[key] = (n, mask)
        return mask

    def filter_rows(self, filter_metadata: dict | None) -> np.ndarray:
        """Ascending unique int64 ordinals of the points whose payload metadata matches every
        condition (the set filter_mask marks; every point without a filter). A condition whose
        wanted value is a canonical scalar and whose key holds no value of an unusual type takes
        the key index's ordinal arrays directly, and those are intersected: O(matches), not
        O(points). Any other condition goes through _key_matches."""
        n = self.count
        if not filter_metadata:
            return np.arange(n, dtype=np.int64)
        rows = None
        general = []
        for k, v in filter_metadata.items():
            c = _canon(v)
            if c is None:
                general.append((k, v))
                continue
            _, inv, gen = self._key_entry(k, n)
            if gen:
                general.append((k, v))
                continue
            hit = inv.get(c) if c is not _NO_MATCH else None
            if hit is None:
                return np.zeros(0, dtype=np.int64)
            rows = hit if rows is None else np.intersect1d(rows, hit, assume_unique=True)
        if general:
            ok = np.ones(n, dtype=bool)
            for k, v in general:
                ok &= self._key_matches(k, v, n)
            rows = np.nonzero(ok)[0] if rows is None else rows[ok[rows]]
        return np.ascontiguousarray(rows, dtype=np.int64)

    def _key_entry(self, key: str, n: int) -> tuple:
        """The key index of a metadata key over the first n points: (n, {value class: ascending
        unique ordinals}, points whose value needs the general comparison)."""
        cached = self._key_index.get(key)
        if cached is None or cached[0] != n:
            inv: dict = {}
            general: list[int] = []  # points whose value needs the general comparison
            for i, p in enumerate(self.payloads[:n]):
                md = p.get("metadata") or {}
                if key not in md:
                    continue
                fv = md[key]
                for x in (fv if isinstance(fv, list) else (fv,)):
                    c = _canon(x)
                    if c is None:
                        general.append(i)
                    elif c is not _NO_MATCH:
                        inv.setdefault(c, []).append(i)
            cached = (n, {c: np.unique(np.asarray(v, dtype=np.int64)) for c, v in inv.items()},
                      general)
            self._key_index[key] = cached
        return cached

    def _key_matches(self, key: str, wanted, n: int) -> np.ndarray:
        """bool [n]: points whose metadata[key] matches `wanted` (_match_value). One pass over
        the payloads per metadata key (cached until the next upsert) builds an inverted map
        value-class -> ordinals, so a new filter value costs O(matches), not O(points)."""
        _, inv, general = self._key_entry(key, n)
        ok = np.zeros(n, dtype=bool)
        c = _canon(wanted)
        if c is not None and c is not _NO_MATCH and c in inv:
            ok[inv[c]] = True
        for i in general:  # rare value types (None, dicts): the reference comparison
            if not ok[i] and _match_value(self.payloads[i]["metadata"][key], wanted):
                ok[i] = True
        if c is None:  # an unusual wanted value: compare every point that has the key
            for i, p in enumerate(self.payloads[:n]):
                md = p.get("metadata") or {}
                if key in md and _match_value(md[key], wanted):
                    ok[i] = True
        return ok

    @classmethod
    def from_indexes(cls, name: str, dense: DenseIndex, payloads: list[dict],
                     sparse: SparseIndex | None = None, shard: tuple = (0, 1)) -> "ChunkCollection":
        """A read-only collection over device indexes built elsewhere (a loaded store shard, a
        synthetic benchmark corpus). Nothing is staged on the host, so it cannot be saved or
        extended with upsert(). Sharded (shard = (rank, world)): the indexes hold this rank's
        shard_range of the corpus (ordinal_base = its first ordinal), payloads every point."""
        coll = cls(name, dense.dim, sparse is not None, dense.device)
        coll.shard = tuple(shard)
        lo, hi = coll.shard_bounds(len(payloads))
        if dense.n_rows != hi - lo or dense.ordinal_base != lo:
            raise ValueError("the dense index must hold this rank's shard of the payloads "
                             f"(ordinals [{lo}, {hi}))")
        coll.payloads = payloads
        coll._dense, coll._sparse = dense, sparse
        coll._built_rows = len(payloads)
        coll._frozen = True
        return coll

    # ------------------------------------------------------------------------ persistence

    def save(self, path) -> None:
        """Writes the collection as an on-disk chunk store (retrieval/store.py)."""
        from audio_rag_amd.retrieval.store import save_arrays

        if self._frozen:
            raise ValueError(f"collection {self.name} has no host copy (built from device indexes)")
        with self._lock:
            rows = (np.concatenate(self.dense_rows) if self.dense_rows
                    else np.zeros((0, self.dim), dtype=np.float16))
            save_arrays(path, self.name, rows, list(self.sparse_rows), list(self.payloads),
                        self.hybrid)

    @classmethod
    def load(cls, path, device: torch.device, name: str | None = None) -> "ChunkCollection":
        """A collection holding every point of an on-disk chunk store, in ordinal order."""
        from audio_rag_amd.retrieval.store import load_shard

        sh = load_shard(path)
        coll = cls(name or sh.name, sh.dim, sh.hybrid, device)
        coll.upsert(np.ascontiguousarray(sh.dense, dtype=np.float16), sh.sparse_rows(),
                    sh.payloads)
        return coll

    def attach_server(self, server) -> None:
        """Registers a StreamServer over this collection's indexes: close() stops it first."""
        self._servers.add(server)

    def close(self) -> None:
        # the native servers' dispatcher threads launch searches on these indexes: stop them
        # before the indexes are freed
        for srv in list(self._servers):
            srv.close()
        self._graphs = {}
        for ix in (self._dense, self._sparse, self._tail, self._tail_sparse):
            if ix is not None:
                ix.close()
        self._dense = self._sparse = self._tail = self._tail_sparse = None
        self._built_rows = -1
