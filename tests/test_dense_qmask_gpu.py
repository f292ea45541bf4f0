"""armi_dense_topk_qmask (DenseIndex.topk_masks): a dense top-k in which every query carries its
own row mask, answered by one int8 first pass per 64-query block and one collect pass.

Every answer must be bit-identical (ids, rank keys, scores, counts) to oracle.dense_topk called
with that query's mask, and, where noted, to DenseIndex.topk(row_mask=...) called once per mask on
the same index. Rows are oracle.unit_fp16; a reference is computed once per (rows, queries, mask)
at the largest k and its prefixes serve the smaller k (a top-k list is a prefix of the top-64)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = 3      # ordinal_base of every index here
KMAX = 64


def _bits(on: np.ndarray, words: int | None = None) -> np.ndarray:
    """bool [n] -> uint64 bitmask words (bit r of word r // 64)."""
    n = on.shape[0]
    w = np.zeros(words or (n + 63) // 64, dtype=np.uint64)
    idx = np.flatnonzero(on)
    np.bitwise_or.at(w, idx >> 6, np.left_shift(np.uint64(1), (idx & 63).astype(np.uint64)))
    return w


def _dev(a: np.ndarray, gpu) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _f16(a: np.ndarray, gpu) -> torch.Tensor:
    return _dev(a.view(np.float16), gpu)


def _stack(masks: list, gpu, stride: int | None = None) -> torch.Tensor:
    """uint64 mask arrays -> int64 [n_masks, stride] on the device (zero-padded rows)."""
    stride = stride or max(len(m) for m in masks)
    out = np.zeros((len(masks), stride), dtype=np.uint64)
    for i, m in enumerate(masks):
        out[i, :len(m)] = m
    return _dev(out.view(np.int64), gpu)


def _arrays(out) -> dict:
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "rank", "count", "flags")}


def _run(idx, q, k, stacked, q_mask, gpu) -> dict:
    qm = _dev(np.asarray(q_mask, dtype=np.int32), gpu)   # on the device: not read back
    return _arrays(idx.topk_masks(q, k, stacked, qm))


class Ref:
    """oracle.dense_topk per (query, mask) at k = KMAX, computed once and sliced per k."""

    def __init__(self, oracle_mod, rows, qs, base=BASE):
        self.o, self.rows, self.qs, self.base = oracle_mod, rows, qs, base
        self.cache: dict = {}

    def lists(self, masks: list, q_mask) -> dict:
        b = len(q_mask)
        ref = {"ids": np.empty((b, KMAX), np.int64), "rank": np.empty((b, KMAX), np.float64),
               "scores": np.empty((b, KMAX), np.float32), "count": np.empty(b, np.int32)}
        n = self.rows.shape[0]
        for m in sorted(set(q_mask)):
            sel = [q for q in range(b) if q_mask[q] == m]
            mask = None if m < 0 else np.ascontiguousarray(masks[m][:(n + 63) // 64])
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


def _assert_flags(got: dict, allowed=(1, 2)):
    from audio_rag_amd import _armi

    assert ((got["flags"] & _armi.ARMI_FLAG_QMASK) != 0).all(), got["flags"]
    assert set(np.unique(got["flags"] & ~_armi.ARMI_FLAG_QMASK)) <= set(allowed), got["flags"]


# ------------------------------------------------------------------------------------ shapes

_stores: dict = {}


def _store(oracle_mod, gpu, n, dim):
    """(index, rows, 128 queries, 128 random 40 % masks, Ref) of one (n, dim), shared by its cases."""
    from audio_rag_amd.retrieval.device import DenseIndex

    if (n, dim) not in _stores:
        rows = oracle_mod.unit_fp16(n, dim, seed=1000 + n + dim)
        qs = oracle_mod.unit_fp16(128, dim, seed=1001 + n + dim)
        rng = np.random.default_rng(n + dim)
        masks = [_bits(rng.random(n) < 0.4) for _ in range(128)]
        idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
        _stores[(n, dim)] = (idx, rows, qs, masks, Ref(oracle_mod, rows, qs))
    return _stores[(n, dim)]


def _q_mask(nq: int, n_masks: int) -> list:
    """Query q under mask q % n_masks, every fifth query unfiltered (-1); a single query keeps its
    mask."""
    qm = [q % n_masks for q in range(nq)]
    for q in range(0, nq, 5):
        if nq > 1:
            qm[q] = -1
    return qm


@pytest.mark.parametrize("nq", [1, 64, 65, 128])
@pytest.mark.parametrize("n,dim", [(32 * 97 + 5, 256), (32 * 97 + 5, 1024), (20011, 256),
                                   (20011, 1024)])
def test_shapes_match_oracle(gpu, oracle_mod, n, dim, nq):
    idx, rows, qs, masks, ref = _store(oracle_mod, gpu, n, dim)
    assert idx.qmask_supported(nq, KMAX)
    q = _f16(qs[:nq], gpu)
    for n_masks in sorted({1, 3, nq}):
        stacked = _stack(masks[:n_masks], gpu)
        qm = _q_mask(nq, n_masks)
        want = ref.lists(masks, qm)
        for k in (1, 5, 40, 64):
            got = _run(idx, q, k, stacked, qm, gpu)
            _assert_same(got, want, k, f"n={n} dim={dim} nq={nq} masks={n_masks} k={k}")
            _assert_flags(got)


def test_equals_one_masked_topk_per_mask(gpu, oracle_mod):
    """The same index, DenseIndex.topk(row_mask=...) once per mask: bit for bit."""
    idx, rows, qs, masks, _ = _store(oracle_mod, gpu, 20011, 1024)
    nq, n_masks = 65, 3
    qm = _q_mask(nq, n_masks)
    stacked = _stack(masks[:n_masks], gpu)
    for k in (5, 40):
        got = _run(idx, _f16(qs[:nq], gpu), k, stacked, qm, gpu)
        for m in sorted(set(qm)):
            sel = [q for q in range(nq) if qm[q] == m]
            one = _arrays(idx.topk(_f16(qs[sel], gpu), k, row_mask=None if m < 0 else stacked[m]))
            np.testing.assert_array_equal(got["count"][sel], one["count"])
            np.testing.assert_array_equal(got["ids"][sel], one["ids"])
            for j, q in enumerate(sel):
                c = one["count"][j]
                np.testing.assert_array_equal(got["rank"][q, :c], one["rank"][j, :c])
                np.testing.assert_array_equal(got["scores"][q, :c], one["scores"][j, :c])


def test_several_workgroups_and_ranges(gpu, oracle_mod):
    """60 000 x 1024: many tile ranges per query block, both blocks of a 128-query call."""
    from audio_rag_amd.retrieval.device import DenseIndex

    n, nq = 60000, 128
    rows = oracle_mod.unit_fp16(n, 1024, seed=1200)
    qs = oracle_mod.unit_fp16(nq, 1024, seed=1201)
    rng = np.random.default_rng(1202)
    masks = [_bits(rng.random(n) < 0.4) for _ in range(5)]
    qm = _q_mask(nq, 5)
    idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
    want = Ref(oracle_mod, rows, qs).lists(masks, qm)
    stacked = _stack(masks, gpu)
    for k in (5, 40):
        got = _run(idx, _f16(qs, gpu), k, stacked, qm, gpu)
        _assert_same(got, want, k, f"k={k}")
        _assert_flags(got)


# ------------------------------------------------------------------------- mask / query mix-ups

@pytest.mark.parametrize("step", [32, 1], ids=["pairs(q,q+32)", "pairs(q,q+1)"])
def test_a_query_is_filtered_by_its_own_mask(gpu, oracle_mod, step):
    """Each of 64 vectors is a row of the store (its planted row) and is asked twice in a
    128-query call, at positions (q, q + step): once under a mask that clears only its planted
    row, once under a mask that clears nothing. A kernel that applied a neighbour's word, the
    other lane half's, or the other query block's would show the planted row where it is cleared
    or lose it where it is not."""
    from audio_rag_amd.retrieval.device import DenseIndex

    n, dim, k = 4001, 256, 5
    rows = oracle_mod.unit_fp16(n, dim, seed=1300)
    planted = np.random.default_rng(1301).choice(n, size=64, replace=False)
    firsts = [q for q in range(128) if (q // step) % 2 == 0]      # q, its twin at q + step
    assert len(firsts) == 64
    qs = np.empty((128, dim), dtype=np.uint16)
    qm = np.empty(128, dtype=np.int32)
    cleared = np.zeros(128, dtype=bool)
    masks = []
    for v, q in enumerate(firsts):
        qs[q] = qs[q + step] = rows[planted[v]]
        on = np.ones(n, dtype=bool)
        on[planted[v]] = False
        masks.append(_bits(on))
        a, b = (q, q + step) if v % 2 == 0 else (q + step, q)    # which twin is cleared alternates
        qm[a], qm[b], cleared[a] = v, 64, True
    masks.append(_bits(np.ones(n, dtype=bool)))                  # mask 64 clears nothing
    idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
    got = _run(idx, _f16(qs, gpu), k, _stack(masks, gpu), qm, gpu)
    for v, q in enumerate(firsts):
        want = BASE + planted[v]
        for p in (q, q + step):
            if cleared[p]:
                assert want not in got["ids"][p], f"vector {v}: cleared row returned at query {p}"
            else:
                assert got["ids"][p, 0] == want, f"vector {v}: planted row lost at query {p}"
    _assert_same(got, Ref(oracle_mod, rows, qs).lists(masks, list(qm)), k)


# ----------------------------------------------------------------------------------- edge masks

def test_edge_masks_in_one_call(gpu, oracle_mod):
    """All rows, no row, three rows, only rows the index marks invalid, and masks with garbage
    1-bits past n_rows (in the last word and in two extra stride words), next to ordinary masks."""
    from audio_rag_amd.retrieval.device import DenseIndex

    n, dim, k = 32 * 97 + 5, 256, 5
    rows = oracle_mod.unit_fp16(n, dim, seed=1400).copy()
    invalid = [7, 1500, n - 1]
    rows[invalid, 0] = np.float16(4.0).view(np.uint16)           # outside the fp16 domain |x| < 2
    qs = oracle_mod.unit_fp16(24, dim, seed=1401)
    rng = np.random.default_rng(1402)
    words = (n + 63) // 64
    some = rng.random(n) < 0.4
    three = np.zeros(n, dtype=bool)
    three[[5, 1700, n - 2]] = True
    bad = np.zeros(n, dtype=bool)
    bad[invalid] = True
    garbage_all = _bits(np.ones(n, dtype=bool), words + 2)
    garbage_all[words - 1] = ~np.uint64(0)
    garbage_all[words:] = ~np.uint64(0)
    garbage_some = _bits(some, words + 2)
    garbage_some[words - 1] |= ~np.uint64(0) << np.uint64(n & 63)
    garbage_some[words:] = ~np.uint64(0)
    masks = [_bits(np.ones(n, dtype=bool)), _bits(np.zeros(n, dtype=bool)), _bits(three), _bits(bad),
             garbage_all, garbage_some, _bits(some), _bits(rng.random(n) < 0.4)]
    qm = [q % 8 for q in range(24)]
    qm[20] = -1
    idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
    assert idx.invalid_rows() == 3
    got = _run(idx, _f16(qs, gpu), k, _stack(masks, gpu, words + 2), qm, gpu)
    _assert_same(got, Ref(oracle_mod, rows, qs).lists(masks, qm), k)
    count = got["count"]
    assert (count[[q for q in range(24) if qm[q] == 1]] == 0).all()       # no row
    assert (got["ids"][[q for q in range(24) if qm[q] == 1]] == -1).all()
    assert (count[[q for q in range(24) if qm[q] == 2]] == 3).all()       # three rows < k
    assert (count[[q for q in range(24) if qm[q] == 3]] == 0).all()       # invalid rows only
    assert got["ids"].max() < BASE + n                                     # no padding position
    for bad_row in invalid:
        assert BASE + bad_row not in got["ids"]
    _assert_flags(got)


# ---------------------------------------------------------------------------------- collect pass

@pytest.mark.parametrize("pile", [300, 5000], ids=["collect-list", "overflow-helpers"])
def test_duplicate_pile_under_three_masks(gpu, oracle_mod, pile):
    """A pile of identical rows on top of the pile queries (300: the collect list; 5000: more than
    the 4096 it holds, so the helper workgroups score the store under each query's OWN mask): no
    mask, every third pile row cleared, the whole pile cleared, and every seventh cleared (which at
    5000 still leaves more than 4096: an overflow under a mask). Unrelated queries ride along in
    both query blocks; ties resolve by ordinal."""
    from audio_rag_amd import _armi
    from audio_rag_amd.retrieval.device import DenseIndex

    dim, k, lo = 1024, 10, 3000
    base = oracle_mod.unit_fp16(9000, dim, seed=1500)
    v = oracle_mod.unit_fp16(1, dim, seed=1501)
    rows = np.concatenate([base[:lo], np.repeat(v, pile, axis=0), base[lo:]])
    n = rows.shape[0]
    other = oracle_mod.unit_fp16(70, dim, seed=1502)
    pos = [0, 33, 40, 69]                  # the pile queries: columns r and 32 + r, both blocks
    qs = other.copy()
    qs[pos] = v
    in_pile = (np.arange(n) >= lo) & (np.arange(n) < lo + pile)
    third = ~(in_pile & ((np.arange(n) - lo) % 3 == 0))
    rng = np.random.default_rng(1503)
    seventh = ~(in_pile & ((np.arange(n) - lo) % 7 == 0))
    masks = [_bits(third), _bits(~in_pile), _bits(rng.random(n) < 0.4), _bits(seventh)]
    qm = [2 if q % 2 else -1 for q in range(70)]
    qm[0], qm[40], qm[69], qm[33] = -1, 0, 1, 3
    idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
    got = _run(idx, _f16(qs, gpu), k, _stack(masks, gpu), qm, gpu)
    _assert_same(got, Ref(oracle_mod, rows, qs).lists(masks, qm), k)
    assert list(got["ids"][0]) == [BASE + lo + i for i in range(k)]
    assert list(got["ids"][40]) == [BASE + lo + i for i in range(3 * k // 2 + 1) if i % 3][:k]
    assert list(got["ids"][33]) == [BASE + lo + i for i in range(2 * k) if i % 7][:k]
    assert not (set(got["ids"][69]) & set(range(BASE + lo, BASE + lo + pile)))
    for q in (0, 33, 40):                       # ties at the k-th key: no certificate
        assert got["flags"][q] == _armi.ARMI_FLAG_FALLBACK | _armi.ARMI_FLAG_QMASK
    _assert_flags(got)


# ----------------------------------------------------------------------- flags, argument errors

def test_unsupported_shapes_and_argument_errors(gpu, oracle_mod):
    from audio_rag_amd import _armi
    from audio_rag_amd._armi import ptr, stream_handle
    from audio_rag_amd.retrieval.device import TailIndex, TopK

    idx, rows, qs, masks, ref = _store(oracle_mod, gpu, 32 * 97 + 5, 256)
    n = rows.shape[0]
    stacked = _stack(masks[:2], gpu)
    assert idx.qmask_supported(1, 1) and idx.qmask_supported(128, 64)
    assert not idx.qmask_supported(128, 65) and not idx.qmask_supported(129, 5)
    assert not idx.qmask_supported(0, 5)
    assert idx.qmask_workspace_bytes(128, 65, 2) == 0
    many = _f16(np.concatenate([qs, qs[:1]]), gpu)
    for q, k in ((_f16(qs[:4], gpu), 65), (many, 5)):
        with pytest.raises(_armi.ArmiError) as e:
            idx.topk_masks(q, k, stacked, torch.zeros(q.shape[0], dtype=torch.int32, device=gpu))
        assert e.value.code == _armi.ARMI_ERR_UNSUPPORTED
    tail = TailIndex(256, 64, 0, gpu)
    tail.append(_f16(rows[:40], gpu))
    assert not tail.qmask_supported(4, 5)
    with pytest.raises(_armi.ArmiError) as e:
        tail.topk_masks(_f16(qs[:4], gpu), 5, _stack([masks[0][:1]], gpu),
                        torch.zeros(4, dtype=torch.int32, device=gpu))
    assert e.value.code == _armi.ARMI_ERR_UNSUPPORTED
    tail.close()
    # the Python checks (no device work, a device q_mask is not read)
    q = _f16(qs[:4], gpu)
    qm = torch.zeros(4, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="words"):
        idx.topk_masks(q, 5, stacked[:, :-1].contiguous(), qm)
    with pytest.raises(ValueError, match="q_mask names 3 masks for 4 queries"):
        idx.topk_masks(q, 5, stacked, qm[:3])
    with pytest.raises(ValueError, match=r"in \[-1, 2\)"):
        idx.topk_masks(q, 5, stacked, torch.tensor([0, 1, 2, -1], dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        idx.topk_masks(q, 5, stacked.to(torch.int32), qm)
    # the C boundary: a short stride is ARMI_ERR_INVALID before any device work
    out = TopK.empty(4, 5, gpu, rank=True)
    ws = torch.empty(idx.qmask_workspace_bytes(4, 5, 2), dtype=torch.uint8, device=gpu)
    with pytest.raises(_armi.ArmiError, match="mask_stride_words") as e:
        _armi.call("armi_dense_topk_qmask", idx.handle, ptr(q), 4, 5, ptr(stacked),
                   (n + 63) // 64 - 1, ptr(qm), 2, ptr(out.scores), ptr(out.ids), ptr(out.rank),
                   ptr(out.count), ptr(out.flags), ptr(ws), ws.numel(), stream_handle())
    assert e.value.code == _armi.ARMI_ERR_INVALID
    with pytest.raises(_armi.ArmiError, match="workspace too small") as e:
        _armi.call("armi_dense_topk_qmask", idx.handle, ptr(q), 4, 5, ptr(stacked),
                   (n + 63) // 64, ptr(qm), 2, ptr(out.scores), ptr(out.ids), ptr(out.rank),
                   ptr(out.count), ptr(out.flags), ptr(ws), 16, stream_handle())
    assert e.value.code == _armi.ARMI_ERR_INVALID


def test_out_of_range_q_mask_is_unfiltered(gpu, oracle_mod):
    """include/armi.h: a q_mask entry outside [-1, n_masks) is treated as -1. A device q_mask is
    not checked by the Python layer, so these reach the kernels; none may index row_masks."""
    idx, rows, qs, masks, ref = _store(oracle_mod, gpu, 32 * 97 + 5, 256)
    qm = [0, 2, 7, -5, 2**31 - 1, -2**31, 1, -1]
    got = _run(idx, _f16(qs[:8], gpu), 5, _stack(masks[:2], gpu), qm, gpu)
    as_stated = [m if -1 <= m < 2 else -1 for m in qm]
    assert as_stated == [0, -1, -1, -1, -1, -1, 1, -1]
    _assert_same(got, ref.lists(masks, as_stated), 5)
    _assert_flags(got)
    # no mask at all: n_masks = 0, every query unfiltered
    empty = torch.empty((0, (rows.shape[0] + 63) // 64), dtype=torch.int64, device=gpu)
    got = _run(idx, _f16(qs[:8], gpu), 5, empty, [-1, 0, 3, -1, -1, 1, -1, -1], gpu)
    _assert_same(got, ref.lists(masks, [-1] * 8), 5)


def test_null_out_rank_and_caller_workspace(gpu, oracle_mod):
    from audio_rag_amd import _armi
    from audio_rag_amd._armi import ptr, stream_handle
    from audio_rag_amd.retrieval.device import TopK

    idx, rows, qs, masks, ref = _store(oracle_mod, gpu, 20011, 256)
    qm = _q_mask(65, 3)
    ws = torch.empty(idx.qmask_workspace_bytes(65, 40, 3), dtype=torch.uint8, device=gpu)
    assert ws.numel() >= 2 * ((20011 + 31) // 32) * 256          # two blocks of mask words
    out = TopK.empty(65, 40, gpu, rank=False)
    q = _f16(qs[:65], gpu)
    stacked, qm_dev = _stack(masks[:3], gpu), _dev(np.asarray(qm, np.int32), gpu)
    _armi.call("armi_dense_topk_qmask", idx.handle, ptr(q), 65, 40, ptr(stacked),
               int(stacked.shape[1]), ptr(qm_dev), 3, ptr(out._scores), ptr(out.ids), None,
               ptr(out.count), ptr(out.flags), ptr(ws), ws.numel(), stream_handle())
    torch.cuda.synchronize()
    want = ref.lists(masks, qm)
    count = np.minimum(want["count"], 40)
    np.testing.assert_array_equal(out.count.cpu().numpy(), count)
    np.testing.assert_array_equal(out.ids.cpu().numpy(), want["ids"][:, :40])
    np.testing.assert_array_equal(out._scores.cpu().numpy(), want["scores"][:, :40])


# --------------------------------------------------------------------------------- graph capture

def test_graph_capture_and_replay(gpu, oracle_mod):
    idx, rows, qs, masks, ref = _store(oracle_mod, gpu, 20011, 1024)
    from audio_rag_amd.retrieval.device import TopK

    nq, k, n_masks = 65, 5, 3
    qm = _q_mask(nq, n_masks)
    stacked = _stack(masks[:n_masks], gpu)
    qm_dev = _dev(np.asarray(qm, np.int32), gpu)
    ws = torch.empty(idx.qmask_workspace_bytes(nq, k, n_masks), dtype=torch.uint8, device=gpu)
    q = torch.zeros((nq, 1024), dtype=torch.float16, device=gpu)
    q[torch.arange(nq), torch.arange(nq)] = 1.0     # warm-up queries: one-hot, not all-zero
    out = TopK.empty(nq, k, gpu, rank=True)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        idx.topk_masks(q, k, stacked, qm_dev, workspace=ws, out=out)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx.topk_masks(q, k, stacked, qm_dev, workspace=ws, out=out)
    for lo in (0, 63):                              # two replays, new queries each
        q.copy_(_f16(qs[lo:lo + nq], gpu))
        graph.replay()
        got = _arrays(out)
        shifted = {f: a[lo:lo + nq] for f, a in ref.lists(masks[:n_masks], _shift(qm, lo)).items()}
        _assert_same(got, shifted, k, f"replay at {lo}")
        _assert_flags(got)


def _shift(qm: list, lo: int) -> list:
    """q_mask of the stored 128 queries such that queries lo .. lo + len(qm) - 1 carry qm."""
    return [-1] * lo + list(qm) + [-1] * (128 - lo - len(qm))
