"""armi_dense_topk_qmask_ptrs / armi_sparse_topk_qmask_ptrs (DenseIndex.topk_mask_ptrs,
SparseIndex.topk_mask_ptrs): the per-query-mask searches with the masks addressed through a table
of pointers, every mask a device allocation of its own of exactly ceil(rows / 64) words.

Every answer must be bit-identical (ids, rank keys, scores, counts, padding) to the CPU oracle run
with that query's mask, and to the stack form (topk_masks) on the same index; flags carry
ARMI_FLAG_QMASK. A null table entry, -1, and a q_mask entry outside [0, n_masks) are unfiltered.
References are computed once per store and sliced per k (a top-k list is a prefix of the top-64)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = 3      # ordinal_base of every dense index here
KMAX = 64
CERTIFIED, FALLBACK, FILTERED, QMASK = 1, 2, 4, 16
VOCAB = 250002


def _bits(on: np.ndarray) -> np.ndarray:
    """bool [n] -> uint64 bitmask of exactly ceil(n / 64) words (bit r of word r // 64)."""
    n = on.shape[0]
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    idx = np.flatnonzero(on)
    np.bitwise_or.at(w, idx >> 6, np.left_shift(np.uint64(1), (idx & 63).astype(np.uint64)))
    return w


def _dev(a: np.ndarray, gpu) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _f16(a: np.ndarray, gpu) -> torch.Tensor:
    return _dev(a.view(np.float16), gpu)


def _own(masks: list, gpu) -> list:
    """Every mask as a device tensor of its own, exactly its words long (None stays None)."""
    return [None if m is None else _dev(m.view(np.int64), gpu) for m in masks]


def _stack(masks: list, gpu) -> torch.Tensor:
    """The stack form's tensor of the same masks (a None entry: a zero row no query names)."""
    words = max(len(m) for m in masks if m is not None)
    out = np.zeros((len(masks), words), dtype=np.uint64)
    for i, m in enumerate(masks):
        if m is not None:
            out[i] = m
    return _dev(out.view(np.int64), gpu)


def _stated(q_mask: list, masks: list) -> list:
    """q_mask as include/armi.h reads it: outside [0, n_masks) and a null entry are unfiltered."""
    return [m if 0 <= m < len(masks) and masks[m] is not None else -1 for m in q_mask]


def _q_mask(nq: int, n_masks: int) -> list:
    """Query q under mask q % n_masks (several queries share a mask), every fifth unfiltered (-1),
    one entry n_masks and one -7; a single query keeps a real mask."""
    if nq == 1:
        return [1]
    qm = [q % n_masks for q in range(nq)]
    for q in range(0, nq, 5):
        qm[q] = -1
    qm[3], qm[7] = n_masks, -7
    return qm


# ------------------------------------------------------------------------------------- dense

def _arrays(out) -> dict:
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "rank", "count", "flags")}


class Ref:
    """oracle.dense_topk per (query, mask) at k = KMAX, computed once and sliced per k."""

    def __init__(self, oracle_mod, rows, qs, base=BASE):
        self.o, self.rows, self.qs, self.base = oracle_mod, rows, qs, base
        self.cache: dict = {}

    def lists(self, masks: list, q_mask) -> dict:
        b = len(q_mask)
        ref = {"ids": np.empty((b, KMAX), np.int64), "rank": np.empty((b, KMAX), np.float64),
               "scores": np.empty((b, KMAX), np.float32), "count": np.empty(b, np.int32)}
        for m in sorted(set(q_mask)):
            sel = [q for q in range(b) if q_mask[q] == m]
            mask = None if m < 0 else np.ascontiguousarray(masks[m])
            key = None if mask is None else mask.tobytes()
            todo = [q for q in sel if (q, key) not in self.cache]
            if todo:
                r = self.o.dense_topk(self.rows, self.qs[todo], KMAX, row_mask=mask,
                                      ordinal_base=self.base)
                for j, q in enumerate(todo):
                    self.cache[(q, key)] = (r.ids[j], r.rank[j], r.scores[j], r.count[j])
            for q in sel:
                ref["ids"][q], ref["rank"][q], ref["scores"][q], ref["count"][q] = \
                    self.cache[(q, key)]
        return ref


def _assert_same(got: dict, ref: dict, k: int, msg=""):
    count = np.minimum(ref["count"], k)
    np.testing.assert_array_equal(got["count"], count, err_msg=msg)
    for b, c in enumerate(count):
        for f in ("ids", "rank", "scores"):
            np.testing.assert_array_equal(got[f][b, :c], ref[f][b, :c], err_msg=f"{msg} {f} q{b}")
        assert (got["ids"][b, c:] == -1).all(), f"{msg} ids past the count, query {b}"
        assert np.isneginf(got["scores"][b, c:]).all(), f"{msg} scores past the count, query {b}"


def _assert_identical(got: dict, stack: dict, msg=""):
    for f in ("ids", "rank", "scores", "count", "flags"):
        np.testing.assert_array_equal(got[f], stack[f], err_msg=f"{msg} {f} (table vs stack)")


def _assert_flags(got: dict):
    assert ((got["flags"] & QMASK) != 0).all(), got["flags"]
    assert set(np.unique(got["flags"] & ~np.uint32(QMASK))) <= {CERTIFIED, FALLBACK}, got["flags"]


_stores: dict = {}


def _store(oracle_mod, gpu, dim):
    """(index, rows, 128 queries, 8 table masks, Ref) at n = 32 * 97 + 5 rows: random 40 % masks,
    an all-zero one, one with 1-bits past n in its last word, and a null entry."""
    from audio_rag_amd.retrieval.device import DenseIndex

    n = 32 * 97 + 5
    if dim not in _stores:
        rows = oracle_mod.unit_fp16(n, dim, seed=2000 + dim)
        qs = oracle_mod.unit_fp16(128, dim, seed=2001 + dim)
        rng = np.random.default_rng(2002 + dim)
        masks = [_bits(rng.random(n) < 0.4) for _ in range(8)]
        masks[2] = _bits(np.zeros(n, dtype=bool))
        masks[3][-1] |= ~np.uint64(0) << np.uint64(n & 63)        # 1-bits past the last row
        masks[4] = None
        idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
        _stores[dim] = (idx, rows, qs, masks, Ref(oracle_mod, rows, qs))
    return _stores[dim]


def _run_dense(idx, q, k, masks, qm, gpu):
    """(table form, stack form) of one call; q_mask on the device (not read back, so entries
    outside the table reach the kernels)."""
    qm_dev = _dev(np.asarray(qm, dtype=np.int32), gpu)
    own = _own(masks, gpu)
    got = _arrays(idx.topk_mask_ptrs(q, k, own, qm_dev))
    stack_qm = _dev(np.asarray(_stated(qm, masks), dtype=np.int32), gpu)
    return got, _arrays(idx.topk_masks(q, k, _stack(masks, gpu), stack_qm))


@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("nq", [1, 65, 128])
def test_dense_matches_oracle_and_stack_form(gpu, oracle_mod, nq, k):
    idx, rows, qs, masks, ref = _store(oracle_mod, gpu, 256)
    qm = _q_mask(nq, len(masks))
    got, stack = _run_dense(idx, _f16(qs[:nq], gpu), k, masks, qm, gpu)
    stated = _stated(qm, masks)
    _assert_same(got, ref.lists(masks, stated), k, f"nq={nq} k={k}")
    _assert_identical(got, stack, f"nq={nq} k={k}")
    _assert_flags(got)
    zero = [q for q in range(nq) if stated[q] == 2]
    assert (got["count"][zero] == 0).all() and (got["ids"][zero] == -1).all()
    assert got["ids"].max() < BASE + rows.shape[0]                # no row past n from mask 3


def test_dense_dim_1024(gpu, oracle_mod):
    idx, rows, qs, masks, ref = _store(oracle_mod, gpu, 1024)
    nq, k = 65, 5
    qm = _q_mask(nq, len(masks))
    got, stack = _run_dense(idx, _f16(qs[:nq], gpu), k, masks, qm, gpu)
    _assert_same(got, ref.lists(masks, _stated(qm, masks)), k)
    _assert_identical(got, stack)
    _assert_flags(got)


@pytest.mark.parametrize("pile", [300, 5000], ids=["collect-list", "overflow-helpers"])
def test_dense_duplicate_pile_under_table_masks(gpu, oracle_mod, pile):
    """The duplicate pile of the stack form's collect-pass test: 300 identical rows (the collect
    list answers) and 5000 (more than the 4096 it holds: the helper workgroups score the store
    under each query's OWN table mask). This is where the collect merge reads the masks."""
    from audio_rag_amd.retrieval.device import DenseIndex

    dim, k, lo = 1024, 10, 3000
    base = oracle_mod.unit_fp16(9000, dim, seed=1500)
    v = oracle_mod.unit_fp16(1, dim, seed=1501)
    rows = np.concatenate([base[:lo], np.repeat(v, pile, axis=0), base[lo:]])
    n = rows.shape[0]
    other = oracle_mod.unit_fp16(70, dim, seed=1502)
    pos = [0, 33, 40, 69]                  # the pile queries: both query blocks
    qs = other.copy()
    qs[pos] = v
    in_pile = (np.arange(n) >= lo) & (np.arange(n) < lo + pile)
    third = ~(in_pile & ((np.arange(n) - lo) % 3 == 0))
    seventh = ~(in_pile & ((np.arange(n) - lo) % 7 == 0))
    rng = np.random.default_rng(1503)
    masks = [_bits(third), _bits(~in_pile), _bits(rng.random(n) < 0.4), _bits(seventh)]
    qm = [2 if q % 2 else -1 for q in range(70)]
    qm[0], qm[40], qm[69], qm[33] = -1, 0, 1, 3
    idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
    got, stack = _run_dense(idx, _f16(qs, gpu), k, masks, qm, gpu)
    _assert_same(got, Ref(oracle_mod, rows, qs).lists(masks, qm), k)
    _assert_identical(got, stack)
    assert list(got["ids"][0]) == [BASE + lo + i for i in range(k)]
    assert list(got["ids"][40]) == [BASE + lo + i for i in range(3 * k // 2 + 1) if i % 3][:k]
    assert list(got["ids"][33]) == [BASE + lo + i for i in range(2 * k) if i % 7][:k]
    assert not (set(got["ids"][69]) & set(range(BASE + lo, BASE + lo + pile)))
    for q in (0, 33, 40):                       # ties at the k-th key: no certificate
        assert got["flags"][q] == FALLBACK | QMASK
    _assert_flags(got)


def test_dense_unsupported_shapes_and_short_workspace(gpu, oracle_mod):
    from audio_rag_amd import _armi
    from audio_rag_amd._armi import ptr, stream_handle
    from audio_rag_amd.retrieval.device import TopK

    idx, rows, qs, masks, ref = _store(oracle_mod, gpu, 256)
    own = _own(masks[:2], gpu)
    many = _f16(np.concatenate([qs, qs[:1]]), gpu)
    for q, k in ((_f16(qs[:4], gpu), 65), (many, 5)):
        with pytest.raises(_armi.ArmiError) as e:
            idx.topk_mask_ptrs(q, k, own, torch.zeros(q.shape[0], dtype=torch.int32, device=gpu))
        assert e.value.code == _armi.ARMI_ERR_UNSUPPORTED
    q = _f16(qs[:4], gpu)
    qm = torch.zeros(4, dtype=torch.int32, device=gpu)
    out = TopK.empty(4, 5, gpu, rank=True)
    ws = torch.empty(idx.qmask_workspace_bytes(4, 5, 2), dtype=torch.uint8, device=gpu)
    table = torch.tensor([m.data_ptr() for m in own], dtype=torch.int64, device=gpu)
    with pytest.raises(_armi.ArmiError, match="workspace too small") as e:
        _armi.call("armi_dense_topk_qmask_ptrs", idx.handle, ptr(q), 4, 5, ptr(table), ptr(qm), 2,
                   ptr(out.scores), ptr(out.ids), ptr(out.rank), ptr(out.count), ptr(out.flags),
                   ptr(ws), 16, stream_handle())
    assert e.value.code == _armi.ARMI_ERR_INVALID
    # the Python layer's own checks: a short mask, a host q_mask outside the list
    with pytest.raises(ValueError, match="words"):
        idx.topk_mask_ptrs(q, 5, [own[0][:-1]], qm)
    with pytest.raises(ValueError, match=r"in \[-1, 2\)"):
        idx.topk_mask_ptrs(q, 5, own, torch.tensor([0, 1, 2, -1], dtype=torch.int32))


def test_dense_graph_capture_and_replay(gpu, oracle_mod):
    from audio_rag_amd.retrieval.device import TopK

    idx, rows, qs, masks, ref = _store(oracle_mod, gpu, 256)
    nq, k = 65, 5
    qm = _q_mask(nq, len(masks))
    own = _own(masks, gpu)
    qm_dev = _dev(np.asarray(qm, np.int32), gpu)
    ws = torch.empty(idx.qmask_workspace_bytes(nq, k, len(masks)), dtype=torch.uint8, device=gpu)
    q = torch.zeros((nq, 256), dtype=torch.float16, device=gpu)
    q[torch.arange(nq), torch.arange(nq)] = 1.0     # warm-up queries: one-hot, not all-zero
    out = TopK.empty(nq, k, gpu, rank=True)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        idx.topk_mask_ptrs(q, k, own, qm_dev, workspace=ws, out=out)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    # the table is an argument of the captured kernels: it must outlive the graph
    from audio_rag_amd._armi import call, ptr, stream_handle

    table = torch.tensor([0 if m is None else m.data_ptr() for m in own], dtype=torch.int64,
                         device=gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call("armi_dense_topk_qmask_ptrs", idx.handle, ptr(q), nq, k, ptr(table), ptr(qm_dev),
             len(own), ptr(out.scores), ptr(out.ids), ptr(out.rank), ptr(out.count),
             ptr(out.flags), ptr(ws), ws.numel(), stream_handle())
    q.copy_(_f16(qs[:nq], gpu))
    graph.replay()
    got = _arrays(out)
    _assert_same(got, ref.lists(masks, _stated(qm, masks)), k, "replay")
    _assert_flags(got)


# ------------------------------------------------------------------------------------ sparse

def _t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _sub(q, sel):
    qi, qx, qv = q
    lists = [(qx[qi[b]:qi[b + 1]], qv[qi[b]:qi[b + 1]]) for b in sel]
    ni = np.zeros(len(lists) + 1, np.int32)
    ni[1:] = np.cumsum([t.size for t, _ in lists])
    return (ni, np.concatenate([t for t, _ in lists] + [np.zeros(0, np.int32)]).astype(np.int32),
            np.concatenate([w for _, w in lists] + [np.zeros(0, np.float32)]).astype(np.float32))


def _sparse_oracle(oracle_mod, csr, q, k, masks, q_mask) -> dict:
    """The oracle's lists of every query under its own mask: one oracle run per distinct mask."""
    nq = q[0].size - 1
    ids = np.full((nq, k), -1, np.int64)
    scores = np.full((nq, k), -np.inf, np.float32)
    count = np.zeros(nq, np.int32)
    for m in sorted(set(q_mask)):
        sel = [b for b in range(nq) if q_mask[b] == m]
        ref = oracle_mod.sparse_topk(*csr, *_sub(q, sel), k, row_mask=None if m < 0 else masks[m])
        for j, b in enumerate(sel):
            c = int(ref.count[j])
            count[b] = c
            ids[b, :c] = ref.ids[j, :c]
            scores[b, :c] = ref.scores[j, :c]
    return {"ids": ids, "scores": scores, "count": count}


def _sparse_arrays(out) -> dict:
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "count", "flags")}


def _sparse_same(got: dict, ref: dict, msg=""):
    np.testing.assert_array_equal(got["count"], ref["count"], err_msg=msg)
    for b in range(ref["count"].shape[0]):
        c = ref["count"][b]
        np.testing.assert_array_equal(got["ids"][b, :c], ref["ids"][b, :c], err_msg=f"{msg} q{b}")
        np.testing.assert_array_equal(got["scores"][b, :c], ref["scores"][b, :c],
                                      err_msg=f"{msg} q{b}")
        assert (got["ids"][b, c:] == -1).all(), f"{msg} query {b}"


_SPARSE: dict = {}
N_SPARSE = 3 * 1024 + 5


def _sparse_store(oracle_mod, gpu):
    """(csr, 130 queries (query 3 with a negative weight: the exact scan), 6 table masks, index,
    the oracle's lists at k = 130) of a 3 077-row corpus, built once."""
    from audio_rag_amd import synthetic
    from audio_rag_amd.retrieval.device import SparseIndex

    if not _SPARSE:
        n = N_SPARSE
        csr = tuple(a.cpu().numpy() for a in synthetic.make_sparse_rows(0, n, gpu, seed=63))
        q = tuple(a.cpu().numpy() for a in synthetic.make_sparse_queries(130, gpu, seed=64))
        qv = q[2].copy()
        qv[q[0][3]] = -0.25
        q = (q[0], q[1], qv)
        masks = [_bits(np.random.default_rng(710 + m).random(n) < 0.3) for m in range(6)]
        masks[1] = _bits(np.zeros(n, dtype=bool))
        masks[2][-1] |= ~np.uint64(0) << np.uint64(n & 63)
        masks[4] = None
        idx = SparseIndex(*(_t(a, gpu) for a in csr), VOCAB, 0)
        qm = _q_mask(130, len(masks))
        clean = [None if m is None else m.copy() for m in masks]
        clean[2][-1] &= (np.uint64(1) << np.uint64(n & 63)) - np.uint64(1)
        ref = _sparse_oracle(oracle_mod, csr, q, 130, clean, _stated(qm, masks))
        _SPARSE["s"] = (csr, q, masks, idx, qm, ref)
    return _SPARSE["s"]


@pytest.mark.parametrize("filt", [True, False], ids=["filter", "exact-scan"])
@pytest.mark.parametrize("k", [5, 130])
@pytest.mark.parametrize("nq", [1, 65, 130])
def test_sparse_matches_oracle_and_stack_form(gpu, oracle_mod, nq, k, filt):
    """One, two and three passes of 64 queries; k = 130 skips the MFMA filter; the filter on and
    forced off; query 3 carries a negative weight and takes the exact scan either way."""
    csr, q130, masks, idx, qm130, ref130 = _sparse_store(oracle_mod, gpu)
    # (a single query is query 5 of the store under table mask 0, a random one)
    sel = [5] if nq == 1 else list(range(nq))
    qm = [0] if nq == 1 else qm130[:nq]
    q = _sub(q130, sel)
    if nq == 1:
        ref = _sparse_oracle(oracle_mod, csr, q, k, masks, qm)
    else:
        ref = {"count": np.minimum(ref130["count"][:nq], k), "ids": ref130["ids"][:nq, :k].copy(),
               "scores": ref130["scores"][:nq, :k].copy()}
    idx.set_filter(filt)
    try:
        qd = tuple(_t(a, gpu) for a in q)
        got = _sparse_arrays(idx.topk_mask_ptrs(*qd, k, _own(masks, gpu),
                                                _t(np.asarray(qm, np.int32), gpu)))
        stack = _sparse_arrays(idx.topk_masks(*qd, k, _stack(masks, gpu),
                                              _t(np.asarray(_stated(qm, masks), np.int32), gpu)))
    finally:
        idx.set_filter(True)
    _sparse_same(got, ref, f"nq={nq} k={k} filter={filt}")
    for f in ("ids", "scores", "count", "flags"):
        np.testing.assert_array_equal(got[f], stack[f], err_msg=f"{f} (table vs stack)")
    f = got["flags"]
    assert ((f & QMASK) != 0).all(), f
    assert (((f & CERTIFIED) != 0) ^ ((f & FALLBACK) != 0)).all(), f
    if not filt or k > 128:
        assert not (f & FILTERED).any(), f
    if nq > 3:
        assert not (f[3] & FILTERED)


def test_sparse_graph_capture_and_replay(gpu, oracle_mod):
    from audio_rag_amd._armi import call, ptr, stream_handle
    from audio_rag_amd.retrieval.device import TopK

    csr, q130, masks, idx, qm130, ref130 = _sparse_store(oracle_mod, gpu)
    nq, k = 65, 5
    qd = tuple(_t(a, gpu) for a in _sub(q130, range(nq)))
    own = _own(masks, gpu)
    table = torch.tensor([0 if m is None else m.data_ptr() for m in own], dtype=torch.int64,
                         device=gpu)
    qm_dev = torch.full((nq,), -1, dtype=torch.int32, device=gpu)   # warm-up: unfiltered
    ws = torch.empty(idx.workspace_bytes(nq, k), dtype=torch.uint8, device=gpu)
    out = TopK.empty(nq, k, gpu, rank=False)

    def launch():
        call("armi_sparse_topk_qmask_ptrs", idx.handle, ptr(qd[0]), ptr(qd[1]), ptr(qd[2]), nq, k,
             ptr(table), ptr(qm_dev), len(own), ptr(out.scores), ptr(out.ids), ptr(out.count),
             ptr(out.flags), ptr(ws), ws.numel(), stream_handle())

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    qm_dev.copy_(_t(np.asarray(qm130[:nq], np.int32), gpu))
    graph.replay()
    got = _sparse_arrays(out)
    ref = {"count": np.minimum(ref130["count"][:nq], k), "ids": ref130["ids"][:nq, :k],
           "scores": ref130["scores"][:nq, :k]}
    _sparse_same(got, ref, "replay")
    assert ((got["flags"] & QMASK) != 0).all()
