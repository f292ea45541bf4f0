"""Device-side chunk-store handles over libarmi (torch tensors in, torch tensors out).

Everything here runs on the GPU through the C ABI in include/armi.h; torch only provides device
memory and the stream. Results stay on the device until the caller materialises them.
"""

from __future__ import annotations

import ctypes
import os
import threading

import torch

from audio_rag_amd import _armi
from audio_rag_amd._armi import call, ptr, query, stream_handle

MAX_K = 240
QUERY_BLOCK = 64  # queries per scan pass of armi_dense_topk


class TopK:
    """Per-query top-k on the device. ids are chunk ordinals (-1 past count).

    scores  float32 [B, k]
    ids     int64   [B, k]
    rank    float64 [B, k] ranking key (dense: the exact cosine key; sparse: the scores; fused
            lists: the RRF score)
    count   int32   [B]
    flags   int32   [B] ARMI_FLAG_* bits, or None

    A list whose kernel writes only one of scores / rank gets the other converted on first access
    (on the stream current then), so a hybrid step that reads neither launches no conversion."""

    __slots__ = ("_scores", "ids", "_rank", "count", "flags")

    def __init__(self, scores=None, ids=None, rank=None, count=None, flags=None):
        self._scores, self.ids, self._rank, self.count, self.flags = scores, ids, rank, count, flags

    @property
    def scores(self) -> torch.Tensor | None:
        if self._scores is None and self._rank is not None:
            self._scores = self._rank.float()
        return self._scores

    @scores.setter
    def scores(self, t) -> None:
        self._scores = t

    @property
    def rank(self) -> torch.Tensor | None:
        if self._rank is None and self._scores is not None:
            self._rank = self._scores.double()
        return self._rank

    @rank.setter
    def rank(self, t) -> None:
        self._rank = t

    def tensors(self) -> tuple:
        """The device tensors this list holds now (no lazy conversion)."""
        return tuple(t for t in (self._scores, self.ids, self._rank, self.count, self.flags)
                     if t is not None)

    @classmethod
    def empty(cls, b: int, k: int, device: torch.device, rank: bool, flags: bool = True) -> "TopK":
        """Uninitialised outputs of a call over b queries: scores, ids, count, and rank / flags
        when the call writes them."""
        def new(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=device)

        return cls(scores=new((b, k), torch.float32), ids=new((b, k), torch.int64),
                   rank=new((b, k), torch.float64) if rank else None, count=new(b, torch.int32),
                   flags=new(b, torch.int32) if flags else None)


def _check_k(k: int) -> None:
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}]")


def _check_query_csr(q_indptr: torch.Tensor, q_indices: torch.Tensor,
                     q_values: torch.Tensor) -> None:
    for t, dt, name in ((q_indptr, torch.int32, "q_indptr"), (q_indices, torch.int32, "q_indices"),
                        (q_values, torch.float32, "q_values")):
        if t.dtype != dt or t.dim() != 1 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 1-D {dt} device tensor")


def _workspace(workspace: torch.Tensor | None, need: int, device: torch.device) -> torch.Tensor:
    """The caller's workspace when it holds `need` bytes, else a fresh one."""
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    return workspace


def _check_row_lists(list_ptr: torch.Tensor, list_rows: torch.Tensor, q_list: torch.Tensor,
                     n_queries: int, max_list_rows: int, n_rows: int,
                     device: torch.device) -> int:
    """Argument checks of the row-list encoding shared by DenseIndex.topk_rows and
    SparseIndex.topk_rows (include/armi.h, armi_dense_rowlist_topk); returns n_lists. q_list is
    checked for its range only when it lives on the host (a device q_list is not read back: that
    would synchronise every call)."""
    for t, dt, name in ((list_ptr, torch.int64, "list_ptr"), (list_rows, torch.int32, "list_rows"),
                        (q_list, torch.int32, "q_list")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D {dt} tensor")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    n_lists = int(list_ptr.numel()) - 1
    if n_lists < 1:
        raise ValueError("list_ptr must hold at least one list (n_lists + 1 offsets)")
    if int(q_list.numel()) != n_queries:
        raise ValueError(f"q_list names {q_list.numel()} lists for {n_queries} queries")
    if not q_list.is_cuda and n_queries and not (0 <= int(q_list.min()) and
                                                 int(q_list.max()) < n_lists):
        raise ValueError(f"q_list entries must be in [0, {n_lists})")
    if not 0 <= max_list_rows <= n_rows:
        raise ValueError(f"max_list_rows must be in [0, {n_rows}]")
    return n_lists


def _check_row_mask(row_mask: torch.Tensor | None, n_rows: int) -> None:
    """The one shared mask of DenseIndex.topk and TailIndex.tail_topk (None: no filter)."""
    if row_mask is None:
        return
    need = (n_rows + 63) // 64
    if row_mask.dtype != torch.int64 or row_mask.numel() < need or not row_mask.is_cuda:
        raise ValueError(f"row_mask must be an int64 device tensor of >= {need} words")


def _check_row_masks(row_masks: torch.Tensor, q_mask: torch.Tensor, n_queries: int,
                     n_rows: int) -> tuple[int, int]:
    """Argument checks of DenseIndex.topk_masks and SparseIndex.topk_masks (include/armi.h); returns
    (n_masks, stride in words). q_mask is checked for its range only when it lives on the host (a
    device q_mask is not read back: that would synchronise every call; the kernels treat an entry
    outside [-1, n_masks) as -1)."""
    need = (n_rows + 63) // 64
    if not isinstance(row_masks, torch.Tensor) or row_masks.dtype != torch.int64 or \
            row_masks.dim() != 2 or not row_masks.is_cuda or not row_masks.is_contiguous():
        raise ValueError("row_masks must be a contiguous 2-D int64 device tensor [n_masks, words]")
    n_masks, stride = int(row_masks.shape[0]), int(row_masks.shape[1])
    if stride < need:
        raise ValueError(f"row_masks rows must hold >= {need} words")
    if not isinstance(q_mask, torch.Tensor) or q_mask.dtype != torch.int32 or q_mask.dim() != 1 \
            or not q_mask.is_contiguous():
        raise ValueError("q_mask must be a contiguous 1-D int32 tensor")
    if int(q_mask.numel()) != n_queries:
        raise ValueError(f"q_mask names {q_mask.numel()} masks for {n_queries} queries")
    if not q_mask.is_cuda and n_queries and not (-1 <= int(q_mask.min()) and
                                                 int(q_mask.max()) < n_masks):
        raise ValueError(f"q_mask entries must be in [-1, {n_masks})")
    return n_masks, stride


def _mask_table(masks, q_mask: torch.Tensor, n_queries: int, n_rows: int,
                device: torch.device) -> torch.Tensor:
    """Argument checks of DenseIndex.topk_mask_ptrs and SparseIndex.topk_mask_ptrs, and the call's
    pointer table: an int64 device tensor [max(n_masks, 1)] holding each mask's address (0 for
    None: unfiltered). Every mask is a row_mask of topk (its own int64 device tensor of
    >= ceil(rows / 64) words); the caller keeps `masks` referenced until the call is enqueued."""
    if not isinstance(masks, (list, tuple)):
        raise ValueError("masks must be a list of int64 device tensors (None: unfiltered)")
    for m in masks:
        _check_row_mask(m, n_rows)
        if m is not None and (m.device != device or not m.is_contiguous()):
            raise ValueError("every mask must be a contiguous tensor on the index's device")
    if not isinstance(q_mask, torch.Tensor) or q_mask.dtype != torch.int32 or q_mask.dim() != 1 \
            or not q_mask.is_contiguous():
        raise ValueError("q_mask must be a contiguous 1-D int32 tensor")
    if int(q_mask.numel()) != n_queries:
        raise ValueError(f"q_mask names {q_mask.numel()} masks for {n_queries} queries")
    if not q_mask.is_cuda and n_queries and not (-1 <= int(q_mask.min()) and
                                                 int(q_mask.max()) < len(masks)):
        raise ValueError(f"q_mask entries must be in [-1, {len(masks)})")
    addrs = [0 if m is None else int(m.data_ptr()) for m in masks] or [0]
    return torch.tensor(addrs, dtype=torch.int64, device=device)


def _on_device(t: torch.Tensor, device: torch.device) -> torch.Tensor:
    return t if t.is_cuda else t.to(device)


def _check_fp16_2d(t: torch.Tensor, name: str, dim: int | None = None) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float16 or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D float16 tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dim is not None and t.shape[1] != dim:
        raise ValueError(f"{name} has dim {t.shape[1]}, index has {dim}")


class DenseIndex:
    """The Qdrant named vector "dense" (VectorParams(size=dim, distance=COSINE)) of
    src/audio_rag/retrieval/qdrant.py:93-109, as an fp16 row store in HBM.

    rows: [N, dim] float16 on the device (kept alive by this object)."""

    def __init__(self, rows: torch.Tensor, ordinal_base: int = 0):
        _check_fp16_2d(rows, "rows")
        self.rows = rows
        self.dim = int(rows.shape[1])
        self.n_rows = int(rows.shape[0])
        self.ordinal_base = int(ordinal_base)
        self.device = rows.device
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            call("armi_index_create", self.device.index or 0, ptr(rows), self.n_rows, self.dim,
                 self.ordinal_base, ctypes.byref(self._handle), stream_handle())

    def close(self) -> None:
        if self._handle and self._handle.value:
            torch.cuda.synchronize(self.device)
            _armi.call("armi_index_destroy", self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._handle

    def invalid_rows(self) -> int:
        torch.cuda.current_stream(self.device).synchronize()
        return int(query("armi_index_invalid_rows", self._handle))

    def norms(self) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(norm2 int64, inv_norm float64, inv_norm32 float32) copies of the index's arrays."""
        p2, pi, p32 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        call("armi_index_norms", self._handle, ctypes.byref(p2), ctypes.byref(pi), ctypes.byref(p32))
        n = self.n_rows
        out = (torch.empty(n, dtype=torch.int64, device=self.device),
               torch.empty(n, dtype=torch.float64, device=self.device),
               torch.empty(n, dtype=torch.float32, device=self.device))
        torch.cuda.current_stream(self.device).synchronize()
        for src, dst in zip((p2, pi, p32), out):
            _device_copy(dst.data_ptr(), src.value, dst.numel() * dst.element_size())
        return out

    def scan_form(self, n_queries: int, k: int) -> int:
        """Which scan armi_dense_topk runs for this call shape (_armi.SCAN_*)."""
        return int(query("armi_dense_scan_form", self._handle, n_queries, k))

    def scan_nontemporal(self, n_queries: int, k: int) -> bool:
        """Whether the int8 first pass of this call shape streams with nontemporal loads."""
        return int(query("armi_dense_scan_nontemporal", self._handle, n_queries, k)) == 1

    def workspace_bytes(self, n_queries: int, k: int, exact: bool = False) -> int:
        fn = "armi_dense_exact_workspace_bytes" if exact else "armi_dense_workspace_bytes"
        return int(query(fn, self._handle, n_queries, k))

    def topk(self, queries: torch.Tensor, k: int, row_mask: torch.Tensor | None = None,
             exact: bool = False, workspace: torch.Tensor | None = None,
             out: TopK | None = None) -> TopK:
        """Cosine top-k of every query row. row_mask: int64 tensor holding a bitmask of enabled
        rows (bit r of word r // 64), or None."""
        _check_fp16_2d(queries, "queries", self.dim)
        _check_k(k)
        b = int(queries.shape[0])
        dev = self.device
        _check_row_mask(row_mask, self.n_rows)
        if out is None:
            out = TopK.empty(b, k, dev, rank=True)
        workspace = _workspace(workspace, self.workspace_bytes(max(b, 1), k, exact), dev)
        s = stream_handle()
        if exact:
            call("armi_dense_exact_topk", self._handle, ptr(queries), b, k, ptr(row_mask),
                 ptr(out.scores), ptr(out.ids), ptr(out.rank), ptr(out.count), ptr(workspace),
                 workspace.numel(), s)
            if out.flags is not None:
                out.flags.fill_(_armi.ARMI_FLAG_FALLBACK)
        else:
            call("armi_dense_topk", self._handle, ptr(queries), b, k, ptr(row_mask),
                 ptr(out.scores), ptr(out.ids), ptr(out.rank), ptr(out.count), ptr(out.flags),
                 ptr(workspace), workspace.numel(), s)
        return out

    def qmask_supported(self, n_queries: int, k: int) -> bool:
        """Whether topk_masks answers this call shape (an int8 image, <= 128 queries, k <= 64)."""
        return int(query("armi_dense_qmask_supported", self._handle, n_queries, k)) == 1

    def qmask_workspace_bytes(self, n_queries: int, k: int, n_masks: int) -> int:
        return int(query("armi_dense_qmask_workspace_bytes", self._handle, n_queries, k, n_masks))

    def topk_masks(self, queries: torch.Tensor, k: int, row_masks: torch.Tensor,
                   q_mask: torch.Tensor, workspace: torch.Tensor | None = None,
                   out: TopK | None = None) -> TopK:
        """Cosine top-k of every query under its own row mask, one pass over the int8 image per
        64 queries (armi_dense_topk_qmask): row_masks int64 [n_masks, words] device bitmasks
        (topk's row_mask convention, one per row of the tensor), q_mask int32 [B] the mask of each
        query or -1 for none (a host tensor is uploaded). The same ranking, scores and rank keys
        as topk(row_mask=...) called once per mask; flags carry ARMI_FLAG_QMASK. A call shape
        outside qmask_supported() raises ArmiError (ARMI_ERR_UNSUPPORTED)."""
        _check_fp16_2d(queries, "queries", self.dim)
        _check_k(k)
        b = int(queries.shape[0])
        dev = self.device
        n_masks, stride = _check_row_masks(row_masks, q_mask, b, self.n_rows)
        q_mask = _on_device(q_mask, dev)
        if out is None:
            out = TopK.empty(b, k, dev, rank=True)
        if b == 0:
            return out
        workspace = _workspace(workspace, self.qmask_workspace_bytes(b, k, n_masks), dev)
        call("armi_dense_topk_qmask", self._handle, ptr(queries), b, k, ptr(row_masks), stride,
             ptr(q_mask), n_masks, ptr(out.scores), ptr(out.ids), ptr(out.rank), ptr(out.count),
             ptr(out.flags), ptr(workspace), workspace.numel(), stream_handle())
        return out

    def topk_mask_ptrs(self, queries: torch.Tensor, k: int, masks: list, q_mask: torch.Tensor,
                       workspace: torch.Tensor | None = None, out: TopK | None = None) -> TopK:
        """topk_masks with every mask a tensor of its own (armi_dense_topk_qmask_ptrs): masks is a
        list of row_mask tensors (topk's convention; None = unfiltered) that are read in place
        through a table of their addresses instead of being stacked; q_mask int32 [B] names each
        query's entry of the list, or -1. The same results, bit for bit, as topk_masks over the
        stacked masks. The tensors of `masks` must stay alive until the call has run on the
        device (they are referenced here until it is enqueued; the stream orders the rest)."""
        _check_fp16_2d(queries, "queries", self.dim)
        _check_k(k)
        b = int(queries.shape[0])
        dev = self.device
        table = _mask_table(masks, q_mask, b, self.n_rows, dev)
        q_mask = _on_device(q_mask, dev)
        if out is None:
            out = TopK.empty(b, k, dev, rank=True)
        if b == 0:
            return out
        workspace = _workspace(workspace, self.qmask_workspace_bytes(b, k, len(masks)), dev)
        call("armi_dense_topk_qmask_ptrs", self._handle, ptr(queries), b, k, ptr(table),
             ptr(q_mask), len(masks), ptr(out.scores), ptr(out.ids), ptr(out.rank),
             ptr(out.count), ptr(out.flags), ptr(workspace), workspace.numel(), stream_handle())
        return out

    def rowlist_workspace_bytes(self, n_queries: int, k: int, max_list_rows: int) -> int:
        return int(query("armi_dense_rowlist_workspace_bytes", self._handle, n_queries, k,
                         int(max_list_rows)))

    def topk_rows(self, queries: torch.Tensor, k: int, list_ptr: torch.Tensor,
                  list_rows: torch.Tensor, q_list: torch.Tensor, max_list_rows: int,
                  workspace: torch.Tensor | None = None, out: TopK | None = None) -> TopK:
        """Cosine top-k of every query over the rows of its list instead of a masked scan
        (armi_dense_rowlist_topk): list l = list_rows[list_ptr[l] : list_ptr[l + 1]], ascending
        unique int32 local rows; q_list int32 [B] names each query's list; max_list_rows >= the
        longest list (a host value: it sizes the grid). list_ptr / q_list may be host tensors
        (they are uploaded); the same ranking, scores and rank keys as topk(row_mask=...), flags
        ARMI_FLAG_ROWLIST."""
        _check_fp16_2d(queries, "queries", self.dim)
        _check_k(k)
        b = int(queries.shape[0])
        dev = self.device
        n_lists = _check_row_lists(list_ptr, list_rows, q_list, b, int(max_list_rows),
                                   self.n_rows, dev)
        list_ptr, list_rows, q_list = (_on_device(t, dev) for t in (list_ptr, list_rows, q_list))
        if out is None:
            out = TopK.empty(b, k, dev, rank=True)
        if b == 0:
            return out
        workspace = _workspace(workspace, self.rowlist_workspace_bytes(b, k, max_list_rows), dev)
        call("armi_dense_rowlist_topk", self._handle, ptr(queries), b, k, ptr(list_ptr),
             ptr(list_rows), ptr(q_list), n_lists, int(max_list_rows), ptr(out.scores),
             ptr(out.ids), ptr(out.rank), ptr(out.count), ptr(out.flags), ptr(workspace),
             workspace.numel(), stream_handle())
        return out


class TailIndex(DenseIndex):
    """A growable fp16 segment (armi_index_create_tail): the rows added to a live collection
    since its last compaction. The native index owns its row buffer; `parts` keeps the appended
    device blocks for the device-side concatenation of a compaction. Every DenseIndex search
    works on it (fp16 scan forms); tail_topk() is the fused pass that extends a finished list of
    the main index by this segment's rows."""

    def __init__(self, dim: int, capacity: int, ordinal_base: int, device: torch.device):
        self.rows = None
        self.parts: list[torch.Tensor] = []
        self.dim, self.n_rows = int(dim), 0
        self.ordinal_base = int(ordinal_base)
        self.device = device
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            call("armi_index_create_tail", device.index or 0, self.dim, int(capacity),
                 self.ordinal_base, ctypes.byref(self._handle), stream_handle())
        self.capacity = int(query("armi_index_capacity", self._handle))

    def append(self, rows: torch.Tensor) -> None:
        """Adds fp16 rows [n, dim] behind the current end, ordered on the current stream. Not
        under graph capture; searches of this index on other streams must not overlap it."""
        _check_fp16_2d(rows, "rows", self.dim)
        with torch.cuda.device(self.device):
            call("armi_index_append", self._handle, ptr(rows), int(rows.shape[0]), stream_handle())
        self.n_rows = int(query("armi_index_rows", self._handle))
        if rows.shape[0]:
            self.parts.append(rows)

    @staticmethod
    def list_cap() -> int:
        """Survivors the fused pass keeps per query before it falls back to the exact pass."""
        return int(query("armi_dense_tail_list_cap"))

    def tail_workspace_bytes(self, n_queries: int, k: int) -> int:
        return int(query("armi_dense_tail_workspace_bytes", self._handle, n_queries, k))

    def _tail_pass(self, queries: torch.Tensor, k: int, main: TopK,
                   workspace: torch.Tensor | None, row_mask: torch.Tensor | None = None,
                   row_masks: torch.Tensor | None = None,
                   q_mask: torch.Tensor | None = None) -> TopK:
        """The body of tail_topk (row_masks None: one mask or none) and tail_topk_masks."""
        _check_fp16_2d(queries, "queries", self.dim)
        _check_k(k)
        b = int(queries.shape[0])
        if tuple(main.ids.shape) != (b, k):
            raise ValueError("main must be the main index's top-k of the same queries and k")
        dev = self.device
        if row_masks is None:
            _check_row_mask(row_mask, self.n_rows)
            fn, masks = "armi_dense_tail_topk", (ptr(row_mask),)
        else:
            n_masks, stride = _check_row_masks(row_masks, q_mask, b, self.n_rows)
            q_mask = _on_device(q_mask, dev)
            fn, masks = "armi_dense_tail_topk_qmask", (ptr(row_masks) if n_masks else None, stride,
                                                       ptr(q_mask), n_masks)
        out = TopK.empty(b, k, dev, rank=True)
        if b == 0:
            return out
        workspace = _workspace(workspace, self.tail_workspace_bytes(b, k), dev)
        m_scores, m_ids, m_rank, m_count = (t.contiguous() for t in
                                            (main.scores, main.ids, main.rank, main.count))
        call(fn, self._handle, ptr(queries), b, k, *masks, ptr(m_scores), ptr(m_ids), ptr(m_rank),
             ptr(m_count), ptr(out.scores), ptr(out.ids), ptr(out.rank), ptr(out.count),
             ptr(out.flags), ptr(workspace), workspace.numel(), stream_handle())
        return out

    def tail_topk(self, queries: torch.Tensor, k: int, main: TopK,
                  row_mask: torch.Tensor | None = None,
                  workspace: torch.Tensor | None = None) -> TopK:
        """The top-k over the main index and this segment, from `main` = the main index's
        topk(queries, k) (armi_dense_tail_topk). row_mask: bit r = row r of this segment."""
        return self._tail_pass(queries, k, main, workspace, row_mask=row_mask)

    def tail_topk_masks(self, queries: torch.Tensor, k: int, main: TopK, row_masks: torch.Tensor,
                        q_mask: torch.Tensor, workspace: torch.Tensor | None = None) -> TopK:
        """tail_topk with one mask over this segment's rows per query, in the same two launches
        (armi_dense_tail_topk_qmask): row_masks int64 [n_masks, words] device bitmasks (bit r =
        row r of this segment), q_mask int32 [B] the mask of each query or -1 for none (a host
        tensor is uploaded). `main` = the main index's list of the same queries and k, each query
        under its own filter (DenseIndex.topk_masks). The same answer as tail_topk(row_mask=...)
        called once per mask; flags carry ARMI_FLAG_QMASK. Any k that tail_topk takes."""
        return self._tail_pass(queries, k, main, workspace, row_masks=row_masks, q_mask=q_mask)


class SparseIndex:
    """The Qdrant sparse vector "sparse" (SparseVectorParams(index=SparseIndexParams(on_disk=
    False)), no IDF modifier) of src/audio_rag/retrieval/qdrant.py:103-107, as a CSR in HBM.

    indptr int64 [N+1], indices int32 (ascending within a row), values float32; device tensors
    kept alive by this object."""

    def __init__(self, indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                 vocab: int, ordinal_base: int = 0):
        for t, dt, name in ((indptr, torch.int64, "indptr"), (indices, torch.int32, "indices"),
                            (values, torch.float32, "values")):
            if t.dtype != dt or t.dim() != 1 or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous 1-D {dt} device tensor")
        self.indptr, self.indices, self.values = indptr, indices, values
        self.n_rows = int(indptr.numel()) - 1
        self.vocab = int(vocab)
        self.ordinal_base = int(ordinal_base)
        self.device = indptr.device
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            call("armi_sparse_index_create", self.device.index or 0, ptr(indptr), ptr(indices),
                 ptr(values), self.n_rows, int(indices.numel()), self.vocab, self.ordinal_base,
                 ctypes.byref(self._handle), stream_handle())

    def close(self) -> None:
        if self._handle and self._handle.value:
            torch.cuda.synchronize(self.device)
            _armi.call("armi_sparse_index_destroy", self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._handle

    def workspace_bytes(self, n_queries: int, k: int) -> int:
        return int(query("armi_sparse_workspace_bytes", self._handle, n_queries, k))

    def set_filter(self, enable: bool) -> bool:
        """Turns armi_sparse_topk's MFMA filter on / off (on by default; off = the exact scan
        alone, the same results); returns whether the index can use it (every value >= 0)."""
        usable = ctypes.c_int()
        torch.cuda.current_stream(self.device).synchronize()
        call("armi_sparse_index_set_filter", self._handle, int(bool(enable)), ctypes.byref(usable))
        return bool(usable.value)

    def topk(self, q_indptr: torch.Tensor, q_indices: torch.Tensor, q_values: torch.Tensor, k: int,
             row_mask: torch.Tensor | None = None, workspace: torch.Tensor | None = None) -> TopK:
        """Sparse dot top-k for a query CSR (q_indptr int32 [B+1], ascending q_indices int32,
        q_values float32, all on the device)."""
        _check_k(k)
        b = int(q_indptr.numel()) - 1
        dev = self.device
        out = TopK.empty(b, k, dev, rank=False)
        if b == 0:
            return out
        workspace = _workspace(workspace, self.workspace_bytes(b, k), dev)
        call("armi_sparse_topk", self._handle, ptr(q_indptr), ptr(q_indices), ptr(q_values), b, k,
             ptr(row_mask), ptr(out.scores), ptr(out.ids), ptr(out.count), ptr(out.flags),
             ptr(workspace), workspace.numel(), stream_handle())
        return out

    def topk_masks(self, q_indptr: torch.Tensor, q_indices: torch.Tensor, q_values: torch.Tensor,
                   k: int, row_masks: torch.Tensor, q_mask: torch.Tensor,
                   workspace: torch.Tensor | None = None) -> TopK:
        """Sparse dot top-k of every query under its own row mask, in the launches of one topk
        call (armi_sparse_topk_qmask): row_masks int64 [n_masks, words] device bitmasks (topk's
        row_mask convention, one per row of the tensor; [0, words] when no query is filtered),
        q_mask int32 [B] the mask of each query or -1 for none (a host tensor is uploaded). The
        same ids, scores and counts as topk(row_mask=...) called once per mask; flags carry
        ARMI_FLAG_QMASK. Any batch size and k that topk takes; the workspace is topk's."""
        _check_k(k)
        b = int(q_indptr.numel()) - 1
        dev = self.device
        n_masks, stride = _check_row_masks(row_masks, q_mask, b, self.n_rows)
        q_mask = _on_device(q_mask, dev)
        out = TopK.empty(b, k, dev, rank=False)
        if b == 0:
            return out
        workspace = _workspace(workspace, self.workspace_bytes(b, k), dev)
        call("armi_sparse_topk_qmask", self._handle, ptr(q_indptr), ptr(q_indices), ptr(q_values),
             b, k, ptr(row_masks) if n_masks else None, stride, ptr(q_mask), n_masks,
             ptr(out.scores), ptr(out.ids), ptr(out.count), ptr(out.flags), ptr(workspace),
             workspace.numel(), stream_handle())
        return out

    def topk_mask_ptrs(self, q_indptr: torch.Tensor, q_indices: torch.Tensor,
                       q_values: torch.Tensor, k: int, masks: list, q_mask: torch.Tensor,
                       workspace: torch.Tensor | None = None) -> TopK:
        """topk_masks with every mask a tensor of its own (armi_sparse_topk_qmask_ptrs; the mask
        arguments as DenseIndex.topk_mask_ptrs): the same results, bit for bit, as topk_masks over
        the stacked masks."""
        _check_k(k)
        b = int(q_indptr.numel()) - 1
        dev = self.device
        table = _mask_table(masks, q_mask, max(b, 0), self.n_rows, dev)
        q_mask = _on_device(q_mask, dev)
        out = TopK.empty(b, k, dev, rank=False)
        if b == 0:
            return out
        workspace = _workspace(workspace, self.workspace_bytes(b, k), dev)
        call("armi_sparse_topk_qmask_ptrs", self._handle, ptr(q_indptr), ptr(q_indices),
             ptr(q_values), b, k, ptr(table), ptr(q_mask), len(masks), ptr(out.scores),
             ptr(out.ids), ptr(out.count), ptr(out.flags), ptr(workspace), workspace.numel(),
             stream_handle())
        return out

    @staticmethod
    def rowlist_workspace_bytes(n_queries: int, k: int, max_list_rows: int) -> int:
        return int(query("armi_sparse_rowlist_workspace_bytes", n_queries, k, int(max_list_rows)))

    def topk_rows(self, q_indptr: torch.Tensor, q_indices: torch.Tensor, q_values: torch.Tensor,
                  k: int, list_ptr: torch.Tensor, list_rows: torch.Tensor, q_list: torch.Tensor,
                  max_list_rows: int, workspace: torch.Tensor | None = None) -> TopK:
        """Sparse dot top-k of every query over the rows of its list, from this index's forward
        CSR (armi_sparse_rowlist_topk; the list arguments as DenseIndex.topk_rows): the same
        ranking and scores as topk(row_mask=...), flags ARMI_FLAG_ROWLIST."""
        _check_k(k)
        _check_query_csr(q_indptr, q_indices, q_values)
        b = int(q_indptr.numel()) - 1
        dev = self.device
        n_lists = _check_row_lists(list_ptr, list_rows, q_list, max(b, 0), int(max_list_rows),
                                   self.n_rows, dev)
        list_ptr, list_rows, q_list = (_on_device(t, dev) for t in (list_ptr, list_rows, q_list))
        out = TopK.empty(max(b, 0), k, dev, rank=False)
        if b <= 0:
            return out
        workspace = _workspace(workspace, self.rowlist_workspace_bytes(b, k, max_list_rows), dev)
        with torch.cuda.device(dev):
            call("armi_sparse_rowlist_topk", ptr(self.indptr), ptr(self.indices), ptr(self.values),
                 self.n_rows, self.ordinal_base, ptr(q_indptr), ptr(q_indices), ptr(q_values), b, k,
                 ptr(list_ptr), ptr(list_rows), ptr(q_list), n_lists, int(max_list_rows),
                 ptr(out.scores), ptr(out.ids), ptr(out.count), ptr(out.flags), ptr(workspace),
                 workspace.numel(), stream_handle())
        return out


def csr_append(indptr: torch.Tensor | None, indices: torch.Tensor | None,
               values: torch.Tensor | None, new_indptr: torch.Tensor, new_indices: torch.Tensor,
               new_values: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The CSR of `rows + new rows`: (indptr int64, indices int32, values float32), the new block
    given as a CSR of its own (new_indptr starts at 0). indptr None = the first append. Tensors of
    any one device; the last offset is added as a tensor, so nothing is read back to the host."""
    if new_indptr.dtype != torch.int64 or new_indptr.dim() != 1 or new_indptr.numel() < 1:
        raise ValueError("new_indptr must be a 1-D int64 tensor of n + 1 offsets")
    if new_indices.dtype != torch.int32 or new_values.dtype != torch.float32 or \
            new_indices.shape != new_values.shape or new_indices.dim() != 1:
        raise ValueError("new_indices / new_values must be 1-D int32 / float32 of one length")
    if indptr is None:
        return new_indptr.clone(), new_indices.clone(), new_values.clone()
    return (torch.cat([indptr, new_indptr[1:] + indptr[-1:]]), torch.cat([indices, new_indices]),
            torch.cat([values, new_values]))


class TailSparseIndex:
    """The sparse side of a live collection's tail: the forward CSR of the rows added since the
    last compaction, on the device, and nothing else. append() extends it with the new rows' CSR
    (a device-side concatenation); tail_topk() is the fused pass that extends a finished list of
    the main SparseIndex by these rows (armi_sparse_tail_topk reads the CSR directly);
    topk_rows() is SparseIndex's row-list search, which needs the forward CSR only. topk(), the
    general search over the tail alone, runs on a native SparseIndex built on first use and
    dropped by the next append (general_built tells whether one exists): no flush and no fused
    search pays for an inverted index over rows that are folded into the main index soon.

    A search takes one snapshot of (indptr, indices, values, n_rows): an append replaces the
    snapshot, it never writes into arrays a search may be reading."""

    def __init__(self, ordinal_base: int, device: torch.device, vocab: int = 1):
        self.ordinal_base = int(ordinal_base)
        self.device = device
        self.vocab = int(vocab)
        self._csr = (torch.zeros(1, dtype=torch.int64, device=device),
                     torch.zeros(0, dtype=torch.int32, device=device),
                     torch.zeros(0, dtype=torch.float32, device=device), 0)
        self._general: SparseIndex | None = None
        self._lock = threading.Lock()

    indptr = property(lambda self: self._csr[0])
    indices = property(lambda self: self._csr[1])
    values = property(lambda self: self._csr[2])
    n_rows = property(lambda self: self._csr[3])

    @property
    def general_built(self) -> bool:
        """Whether a native SparseIndex over the tail's rows exists now (topk() builds one)."""
        return self._general is not None

    def append(self, indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
               vocab: int | None = None) -> None:
        """Adds the rows of a CSR of their own (indptr from 0; device tensors) behind the current
        end, on the current stream. vocab: the vocabulary the general index is built with from
        now on (it only grows)."""
        for t in (indptr, indices, values):
            if not t.is_cuda:
                raise ValueError("the appended CSR must live on the GPU")
        with self._lock:  # (two appends never interleave; searches read one snapshot, unlocked)
            old = self._csr
            first = old[3] == 0
            csr = csr_append(None if first else old[0], old[1], old[2], indptr, indices, values)
            self._csr = (*csr, old[3] + int(indptr.numel()) - 1)
            if vocab is not None:
                self.vocab = max(self.vocab, int(vocab))
            # (not closed: a search that fetched it may still be using it; it dies with its last
            # reference)
            self._general = None

    def close(self) -> None:
        with self._lock:
            general, self._general = self._general, None
        if general is not None:
            general.close()

    def _general_index(self) -> "SparseIndex":
        with self._lock:
            if self._general is None:
                indptr, indices, values, _ = self._csr
                vocab = max(self.vocab, 1)
                self._general = SparseIndex(indptr, indices, values, vocab,
                                            ordinal_base=self.ordinal_base)
            return self._general

    def topk(self, q_indptr: torch.Tensor, q_indices: torch.Tensor, q_values: torch.Tensor, k: int,
             row_mask: torch.Tensor | None = None, workspace: torch.Tensor | None = None) -> TopK:
        """SparseIndex.topk over the tail's rows alone (builds the native index when missing)."""
        return self._general_index().topk(q_indptr, q_indices, q_values, k, row_mask=row_mask,
                                          workspace=workspace)

    @staticmethod
    def chunk_rows() -> int:
        """Tail rows one scan workgroup of the fused pass covers."""
        return int(query("armi_sparse_tail_chunk_rows"))

    def tail_workspace_bytes(self, n_queries: int, k: int) -> int:
        return int(query("armi_sparse_tail_workspace_bytes", self.n_rows, n_queries, k))

    def _tail_pass(self, q_indptr: torch.Tensor, q_indices: torch.Tensor, q_values: torch.Tensor,
                   k: int, main: TopK, workspace: torch.Tensor | None,
                   row_mask: torch.Tensor | None = None, row_masks: torch.Tensor | None = None,
                   q_mask: torch.Tensor | None = None) -> TopK:
        """The body of tail_topk (row_masks None: one mask or none) and tail_topk_masks."""
        _check_k(k)
        _check_query_csr(q_indptr, q_indices, q_values)
        b = int(q_indptr.numel()) - 1
        indptr, indices, values, n_rows = self._csr
        dev = indptr.device
        self._check_main(main, b, k, dev)
        if q_indptr.device != dev:
            raise ValueError(f"the query CSR must live on {dev}")
        if row_masks is not None:
            n_masks, stride = _check_row_masks(row_masks, q_mask, b, n_rows)
            if row_masks.device != dev:
                raise ValueError(f"row_masks must live on {dev}")
            q_mask = _on_device(q_mask, dev)
            fn, masks = "armi_sparse_tail_topk_qmask", (ptr(row_masks) if n_masks else None, stride,
                                                        ptr(q_mask), n_masks)
        else:
            if row_mask is not None:
                need = (n_rows + 63) // 64
                if row_mask.dtype != torch.int64 or row_mask.numel() < need or \
                        row_mask.device != dev or not row_mask.is_contiguous():
                    raise ValueError(f"row_mask must be a contiguous int64 tensor of >= {need} "
                                     f"words on {dev}")
            if os.environ.get("ARMI_TAIL_PASS", "")[:1] == "g":
                t = self.topk(q_indptr, q_indices, q_values, k, row_mask=row_mask)
                scores = torch.stack([main.scores, t.scores])
                m = merge_shards(scores.double(), scores, torch.stack([main.ids, t.ids]),
                                 torch.stack([main.count, t.count]), k)
                m.flags = main.flags
                return m
            fn, masks = "armi_sparse_tail_topk", (ptr(row_mask),)
        out = TopK.empty(b, k, dev, rank=False)
        if b == 0:
            return out
        need = int(query("armi_sparse_tail_workspace_bytes", n_rows, b, k))
        workspace = _workspace(workspace, need, dev)
        m_scores, m_ids, m_count = (t.contiguous() for t in (main.scores, main.ids, main.count))
        m_flags = None if main.flags is None else main.flags.contiguous()
        with torch.cuda.device(dev):
            call(fn, ptr(indptr), ptr(indices), ptr(values), n_rows, self.ordinal_base,
                 ptr(q_indptr), ptr(q_indices), ptr(q_values), b, k, *masks, ptr(m_scores),
                 ptr(m_ids), ptr(m_count), ptr(m_flags), ptr(out.scores), ptr(out.ids),
                 ptr(out.count), ptr(out.flags), ptr(workspace), workspace.numel(),
                 stream_handle())
        return out

    def tail_topk(self, q_indptr: torch.Tensor, q_indices: torch.Tensor, q_values: torch.Tensor,
                  k: int, main: TopK, row_mask: torch.Tensor | None = None,
                  workspace: torch.Tensor | None = None) -> TopK:
        """The top-k over the main index and this segment, from `main` = the main SparseIndex's
        topk of the same queries and k (armi_sparse_tail_topk). row_mask: bit r = row r of this
        segment. ARMI_TAIL_PASS=general (read per call) computes the same answer by topk() over
        the tail and a merge of the two lists."""
        return self._tail_pass(q_indptr, q_indices, q_values, k, main, workspace,
                               row_mask=row_mask)

    @staticmethod
    def _check_main(main: TopK, b: int, k: int, dev: torch.device) -> None:
        for t, dt, shape, name in ((main.ids, torch.int64, (b, k), "ids"),
                                   (main.scores, torch.float32, (b, k), "scores"),
                                   (main.count, torch.int32, (b,), "count"),
                                   (main.flags, torch.int32, (b,), "flags")):
            if name == "flags" and t is None:
                continue
            if b < 0 or not isinstance(t, torch.Tensor) or t.dtype != dt or \
                    tuple(t.shape) != shape or t.device != dev:
                raise ValueError("main must be the main index's top-k of the same queries and k "
                                 f"on {dev} (its {name} is not a {dt} tensor of shape {shape} there)")

    def tail_topk_masks(self, q_indptr: torch.Tensor, q_indices: torch.Tensor,
                        q_values: torch.Tensor, k: int, main: TopK, row_masks: torch.Tensor,
                        q_mask: torch.Tensor, workspace: torch.Tensor | None = None) -> TopK:
        """tail_topk with one mask over this segment's rows per query, in the same launches
        (armi_sparse_tail_topk_qmask): row_masks int64 [n_masks, words] device bitmasks (bit r =
        row r of this segment), q_mask int32 [B] the mask of each query or -1 for none (a host
        tensor is uploaded). `main` = the main SparseIndex's list of the same queries and k, each
        query under its own filter (SparseIndex.topk_masks); its flags pass through. The same
        answer as tail_topk(row_mask=...) called once per mask."""
        return self._tail_pass(q_indptr, q_indices, q_values, k, main, workspace,
                               row_masks=row_masks, q_mask=q_mask)

    rowlist_workspace_bytes = staticmethod(SparseIndex.rowlist_workspace_bytes)
    topk_rows = SparseIndex.topk_rows  # reads indptr / indices / values / n_rows / ordinal_base


def merge_shards(rank: torch.Tensor, scores: torch.Tensor, ids: torch.Tensor, count: torch.Tensor,
                 k_out: int) -> TopK:
    """Global top-k from per-shard lists [S, B, k_in] (+ count [S, B]) gathered from all ranks."""
    s, b, k_in = ids.shape
    dev = ids.device
    out = TopK.empty(b, k_out, dev, rank=True, flags=False)
    # hold the contiguous copies until the launch is enqueued (a freed temporary's block can be
    # handed to the next allocation before the kernel reads it)
    rank, scores, ids, count = (t.contiguous() for t in (rank, scores, ids, count))
    call("armi_topk_merge_shards", ptr(rank), ptr(scores), ptr(ids), ptr(count), s, b, k_in,
         k_out, ptr(out.rank), ptr(out.scores), ptr(out.ids), ptr(out.count), stream_handle())
    return out


def merge_shards_packed(buf: torch.Tensor, row0: int, n_queries: int, offsets: tuple[int, int, int, int],
                        k_in: int, k_out: int) -> TopK:
    """merge_shards over the all-gathered exchange buffer in place: buf uint8 [S, rows, W] (one
    byte row per (shard, query), shards.pack_rows' layout), this rank's queries at rows
    [row0, row0 + n_queries); offsets = byte offsets of (rank f64, scores f32, ids i64, count i32)
    inside a row. One launch, no per-field copies (armi_topk_merge_shards_packed)."""
    s, rows, w = buf.shape
    if not buf.is_contiguous():
        raise ValueError("merge_shards_packed: the exchange buffer must be contiguous")
    dev = buf.device
    out = TopK.empty(n_queries, k_out, dev, rank=True, flags=False)
    off_rank, off_scores, off_ids, off_count = offsets
    call("armi_topk_merge_shards_packed", buf.data_ptr() + row0 * w, rows * w, w, off_rank,
         off_scores, off_ids, off_count, s, n_queries, k_in, k_out, ptr(out.rank),
         ptr(out.scores), ptr(out.ids), ptr(out.count), stream_handle())
    return out


def rrf_fuse(a: TopK, b: TopK, limit: int, rrf_k: int = 2) -> TopK:
    """FusionQuery(RRF) of two prefetch lists (qdrant.py:295). rank/scores hold the fp64 RRF
    score (scores as float32 for convenience)."""
    n, ka = a.ids.shape
    kb = b.ids.shape[1]
    dev = a.ids.device
    out_ids = torch.empty((n, limit), dtype=torch.int64, device=dev)
    out_score = torch.empty((n, limit), dtype=torch.float64, device=dev)
    out_count = torch.empty(n, dtype=torch.int32, device=dev)
    a_ids, b_ids = a.ids.contiguous(), b.ids.contiguous()
    a_cnt, b_cnt = a.count.to(torch.int32).contiguous(), b.count.to(torch.int32).contiguous()
    call("armi_rrf_fuse", ptr(a_ids), ptr(a_cnt), ka, ptr(b_ids), ptr(b_cnt), kb, n, rrf_k, limit,
         ptr(out_ids), ptr(out_score), ptr(out_count), stream_handle())
    return TopK(ids=out_ids, rank=out_score, count=out_count)


class ConcurrentHybrid:
    """The two prefetches of one hybrid search (qdrant.py:281-298) on two HIP streams: the
    sparse top-k on a side stream, the dense scan and merge on the caller's stream (the two share
    nothing until the fusion), then RRF on the caller's stream. The two scans cannot share a CU
    (each fills its LDS and register file), so in a kernel trace they run nearly one after the
    other (profiles/r05m_hybrid_kernel_stats.csv); what overlaps is the small kernels
    of one chain (merges, collect passes, pass_terms) with the other chain's scan and tail: both
    chains on one stream measured 0.550 against 0.522 ms per step on one box (r05t)."""

    def __init__(self, device: torch.device):
        self.side = torch.cuda.Stream(device=device)

    def __call__(self, dense_fn, sparse_fn, sparse_inputs, limit: int, rrf_k: int = 2) -> TopK:
        main = torch.cuda.current_stream()
        self.side.wait_stream(main)
        # (under graph capture the graph's pool owns every block: no cross-stream bookkeeping)
        capturing = torch.cuda.is_current_stream_capturing()
        for t in sparse_inputs:
            if isinstance(t, torch.Tensor) and t.is_cuda and not capturing:
                t.record_stream(self.side)
        # the sparse chain is issued first (round-3 A/B: profiles/r03x_*)
        with torch.cuda.stream(self.side):
            s = sparse_fn()
        d = dense_fn()
        main.wait_stream(self.side)
        if not capturing:
            for t in s.tensors():
                t.record_stream(main)
        return rrf_fuse(d, s, limit, rrf_k=rrf_k)


_hip = None


def _device_copy(dst: int, src: int, nbytes: int) -> None:
    """Synchronous device-to-device copy through the process's HIP runtime (the one torch
    loaded), for reading the index's internal arrays in tests."""
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so.7")
        _hip.hipMemcpy.restype = ctypes.c_int
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    rc = _hip.hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(src), nbytes, 3)  # DeviceToDevice
    if rc != 0:
        raise RuntimeError(f"hipMemcpy failed: {rc}")


class HybridGraph:
    """One hybrid step over a fixed batch size (ConcurrentHybrid: dense top-k, sparse top-k, RRF)
    captured as a HIP graph. The step's inputs live in one staging buffer (fp16 queries, query
    CSR indptr / indices / values at fixed offsets): a call copies a batch into it, one copy for
    a batch prepared by pack() (or one per array), and replays every kernel of the step. The
    eager step's ~20 launches with their Python argument handling take longer on the host than
    the step takes on the GPU, so eager steps leave the GPU idle between them (30 us per 0.54 ms
    step in profiles/r05m_hybrid_kernel_stats.csv's trace).

    The returned TopK's tensors are the graph's outputs: a later call overwrites them, so callers
    consume (or clone) a result before the next call."""

    def __init__(self, dense: DenseIndex, sparse: SparseIndex, batch: int, pre_k: int, limit: int,
                 rrf_k: int = 2, max_terms: int = 256):
        dev = dense.device
        self.batch, self.dim, self.max_terms = int(batch), dense.dim, int(max_terms)
        self._off = self._layout(self.batch, self.dim, self.max_terms)
        self.stage = torch.zeros(self._off[-1], dtype=torch.uint8, device=dev)
        self.q, self.qi, self.qx, self.qv = self._views(self.stage)
        ws = torch.empty(max(dense.workspace_bytes(batch, pre_k), 1), dtype=torch.uint8, device=dev)
        sws = torch.empty(max(sparse.workspace_bytes(batch, pre_k), 1), dtype=torch.uint8,
                          device=dev)
        hybrid = ConcurrentHybrid(dev)

        def run() -> TopK:
            return hybrid(lambda: dense.topk(self.q, pre_k, workspace=ws),
                          lambda: sparse.topk(self.qi, self.qx, self.qv, pre_k, workspace=sws),
                          (self.qi, self.qx, self.qv), limit, rrf_k)

        # warm-up on a side stream, then capture under inference mode (as _QueryGraph and the
        # reranker's graphs do: the CUDA generator's graph state is shared by every capture).
        # The warm-up batch is one-hot dense queries with empty sparse parts: all-zero queries
        # tie every row at cosine 0, so their top-k cannot be certified and the warm-up ran the
        # dense collect pass over the whole shard (~0.16 s per call at 1M rows, r05z trace)
        rows = torch.arange(self.batch, device=dev)
        self.q[rows, rows % self.dim] = 1.0
        with torch.inference_mode():
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):
                    run()
            torch.cuda.current_stream(dev).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = run()
        self._keep = (ws, sws, hybrid, dense, sparse)

    @staticmethod
    def _layout(batch: int, dim: int, max_terms: int) -> tuple[int, int, int, int, int]:
        def up(x: int) -> int:
            return (x + 255) // 256 * 256

        o_qi = up(batch * dim * 2)
        o_qx = o_qi + up((batch + 1) * 4)
        o_qv = o_qx + up(batch * max_terms * 4)
        return 0, o_qi, o_qx, o_qv, o_qv + up(batch * max_terms * 4)

    def _views(self, buf: torch.Tensor):
        o_q, o_qi, o_qx, o_qv, end = self._off
        b, n = self.batch, self.batch * self.max_terms
        return (buf[o_q:o_qi].view(torch.float16)[: b * self.dim].view(b, self.dim),
                buf[o_qi:o_qx].view(torch.int32)[: b + 1], buf[o_qx:o_qv].view(torch.int32)[:n],
                buf[o_qv:end].view(torch.float32)[:n])

    def _check(self, queries, q_indptr, q_indices, q_values) -> int:
        """Shape checks of a batch. The per-query limit of max_terms (armi_sparse_topk scores a
        longer query's first 256 terms only and flags it) is checked here for a host indptr; a
        device indptr is not read back (that would synchronise every step): callers keep each
        query within max_terms, as query_sparse_arrays does for the pipeline."""
        n = int(q_indices.numel())
        if (tuple(queries.shape) != (self.batch, self.dim) or int(q_indptr.numel()) != self.batch + 1
                or n > self.batch * self.max_terms or int(q_values.numel()) != n):
            raise ValueError("HybridGraph: batch shape differs from the captured one")
        if not q_indptr.is_cuda and self.batch > 0:
            lens = q_indptr[1:].to(torch.int64) - q_indptr[:-1].to(torch.int64)
            if int(lens.max()) > self.max_terms or int(lens.min()) < 0:
                raise ValueError(f"HybridGraph: a query has more than {self.max_terms} terms")
        return n

    def pack(self, queries: torch.Tensor, q_indptr: torch.Tensor, q_indices: torch.Tensor,
             q_values: torch.Tensor) -> torch.Tensor:
        """A batch in the staging layout (one device buffer), for __call__(packed)."""
        n = self._check(queries, q_indptr, q_indices, q_values)
        buf = torch.zeros_like(self.stage)
        q, qi, qx, qv = self._views(buf)
        q.copy_(queries)
        qi.copy_(q_indptr)
        qx[:n].copy_(q_indices)
        qv[:n].copy_(q_values)
        return buf

    def __call__(self, *batch: torch.Tensor) -> TopK:
        """hg(packed) with a pack() buffer (one copy), or hg(queries, q_indptr, q_indices,
        q_values)."""
        if len(batch) == 1:
            if batch[0].shape != self.stage.shape or batch[0].dtype != torch.uint8:
                raise ValueError("HybridGraph: not a pack() buffer of this graph")
            self.stage.copy_(batch[0])
        else:
            queries, q_indptr, q_indices, q_values = batch
            n = self._check(queries, q_indptr, q_indices, q_values)
            self.q.copy_(queries)
            self.qi.copy_(q_indptr)
            self.qx[:n].copy_(q_indices)
            self.qv[:n].copy_(q_values)
        self.graph.replay()
        return self.out
