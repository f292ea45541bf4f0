"""armi_sparse_tail_topk_qmask (TailSparseIndex.tail_topk_masks): the fused sparse tail pass in
which every query carries its own mask over the tail's rows.

Every answer must be bit-identical (ids, fp32 scores, counts, the -1 / -inf padding) to
oracle.sparse_topk over the concatenated CSR with the query's combined mask, and to
TailSparseIndex.tail_topk(row_mask=...) called once per distinct mask with the same main lists
(SparseIndex.topk_masks'); flags pass through from the main list. The main index holds 4,096
oracle.sparse_corpus rows; the oracle's lists are computed once per (tail size, query, mask) at
k = 240 and their prefixes serve k = 5."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAIN, VOCAB, KMAX = 4096, 250002, 240
CHUNK = 128   # armi_sparse_tail_chunk_rows(): asserted below
TAILS = (1, CHUNK, CHUNK + 1, 2 * CHUNK + 70)   # one chunk (finished by the scan), then the finish


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _np(out):
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "count", "flags")}


def _bits(on: np.ndarray) -> np.ndarray:
    w = np.zeros(max((len(on) + 63) // 64, 1), dtype=np.uint64)
    idx = np.flatnonzero(on)
    np.bitwise_or.at(w, idx >> 6, np.left_shift(np.uint64(1), (idx & 63).astype(np.uint64)))
    return w


def _rows(csr, lo, hi):
    ip, ix, iv = csr
    return ip[lo:hi + 1] - ip[lo], ix[ip[lo]:ip[hi]], iv[ip[lo]:ip[hi]]


def _query_csr(lists):
    qi = np.zeros(len(lists) + 1, dtype=np.int32)
    np.cumsum([len(q[0]) for q in lists], out=qi[1:])
    qx = np.concatenate([np.asarray(q[0], np.int32) for q in lists] + [np.zeros(1, np.int32)])
    qv = np.concatenate([np.asarray(q[1], np.float32) for q in lists] + [np.zeros(1, np.float32)])
    return qi, qx.astype(np.int32), qv.astype(np.float32)   # (one spare entry: non-null pointers)


def _tail(csr, gpu):
    from audio_rag_amd.retrieval.device import TailSparseIndex

    t = TailSparseIndex(MAIN, gpu, vocab=VOCAB)
    t.append(*(_dev(a, gpu) for a in csr))
    return t


def _masks(tail_n: int) -> list:
    """As in test_dense_tail_qmask_gpu: 0 a random half (shared), 1 all-zero, 2 tail bits only,
    3 main bits only, 4 a random 30 %, 5 three main rows and all but one tail row."""
    rng = np.random.default_rng(100 + tail_n)
    n = MAIN + tail_n
    oks = [rng.random(n) < 0.5, np.zeros(n, dtype=bool), np.arange(n) >= MAIN, np.arange(n) < MAIN,
           rng.random(n) < 0.3, np.zeros(n, dtype=bool)]
    oks[5][[5, 700, 4000]] = True
    oks[5][MAIN:] = True
    oks[5][MAIN + tail_n // 2] = False
    return oks


def _q_mask(nq: int, n_masks: int) -> list:
    pattern = [0, -1, 0, 1, 2, 3, 4, 5, n_masks, -7]
    return [pattern[q % len(pattern)] for q in range(nq)]


def _eff(m: int, n_masks: int) -> int:
    return m if 0 <= m < n_masks else -1


def _stacks(oks, tail_n, gpu):
    """(main stack, tail stack): the tail's with every bit past its last row set, in the last word
    and in a spare word behind it."""
    words = (tail_n + 63) // 64
    t = np.full((len(oks), words + 1), ~np.uint64(0), dtype=np.uint64)
    for i, ok in enumerate(oks):
        t[i, :words] = _bits(ok[MAIN:])
        if tail_n % 64:
            t[i, words - 1] |= ~np.uint64(0) << np.uint64(tail_n % 64)
    m = np.stack([_bits(ok[:MAIN]) for ok in oks])
    return _dev(m.view(np.int64), gpu), _dev(t.view(np.int64), gpu)


@pytest.fixture(scope="module")
def seg(gpu, oracle_mod):
    """(corpus CSR of main + the largest tail, 70 query term lists, the main SparseIndex). Query 13
    has no terms."""
    from audio_rag_amd.retrieval.device import SparseIndex, TailSparseIndex

    assert TailSparseIndex.chunk_rows() == CHUNK
    csr = oracle_mod.sparse_corpus(MAIN + max(TAILS), seed=401)
    qi, qx, qv = oracle_mod.sparse_queries(70, seed=402)
    lists = [(qx[qi[b]:qi[b + 1]], qv[qi[b]:qi[b + 1]]) for b in range(70)]
    lists[13] = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    main = SparseIndex(*(_dev(a, gpu) for a in _rows(csr, 0, MAIN)), VOCAB)
    return csr, lists, main


_oracle: dict = {}


def _oracle_lists(oracle_mod, csr, lists, oks, q_mask, tail_n) -> dict:
    b = len(q_mask)
    ref = {"ids": np.empty((b, KMAX), np.int64), "scores": np.empty((b, KMAX), np.float32),
           "count": np.empty(b, np.int32)}
    eff = [_eff(m, len(oks)) for m in q_mask]
    for m in sorted(set(eff)):
        todo = [q for q in range(b) if eff[q] == m and (tail_n, q, m) not in _oracle]
        if todo:
            qi, qx, qv = _query_csr([lists[q] for q in todo])
            r = oracle_mod.sparse_topk(*_rows(csr, 0, MAIN + tail_n), qi, qx[:qi[-1]], qv[:qi[-1]],
                                       KMAX, row_mask=None if m < 0 else _bits(oks[m]))
            for j, q in enumerate(todo):
                _oracle[(tail_n, q, m)] = (r.ids[j], r.scores[j], r.count[j])
        for q in range(b):
            if eff[q] == m:
                ref["ids"][q], ref["scores"][q], ref["count"][q] = _oracle[(tail_n, q, m)]
    return ref


def _assert_oracle(got, ref, k):
    count = np.minimum(ref["count"], k)
    np.testing.assert_array_equal(got["count"], count)
    for b, c in enumerate(count):
        for f in ("ids", "scores"):
            np.testing.assert_array_equal(got[f][b, :c], ref[f][b, :c], err_msg=f"{f} q{b}")
        assert (got["ids"][b, c:] == -1).all() and np.isneginf(got["scores"][b, c:]).all()


@pytest.mark.parametrize("tail_n,nq,k", [(t, 70, k) for t in TAILS for k in (5, 240)] +
                         [(CHUNK + 1, 1, 5), (CHUNK, 65, 240)])
def test_matches_the_oracle_and_one_call_per_mask(gpu, oracle_mod, seg, tail_n, nq, k):
    from audio_rag_amd import _armi

    csr, lists, main_idx = seg
    oks = _masks(tail_n)
    q_mask = _q_mask(nq, len(oks))
    q = tuple(_dev(a, gpu) for a in _query_csr(lists[:nq]))
    tail = _tail(_rows(csr, MAIN, MAIN + tail_n), gpu)
    mstack, tstack = _stacks(oks, tail_n, gpu)
    qm = _dev(np.asarray(q_mask, np.int32), gpu)   # exactly nq entries, on the device
    main = main_idx.topk_masks(*q, k, mstack, qm)
    one_chunk = tail_n <= CHUNK
    assert (tail.tail_workspace_bytes(nq, k) == 0) == one_chunk
    got = _np(tail.tail_topk_masks(*q, k, main, tstack, qm))
    _assert_oracle(got, _oracle_lists(oracle_mod, csr, lists, oks, q_mask, tail_n), k)
    # flags pass through from the main list, which carries ARMI_FLAG_QMASK
    np.testing.assert_array_equal(got["flags"], _np(main)["flags"])
    assert ((got["flags"] & _armi.ARMI_FLAG_QMASK) != 0).all()
    eff = [_eff(m, len(oks)) for m in q_mask]
    for m in sorted(set(eff)):
        one = _np(tail.tail_topk(*q, k, main, row_mask=None if m < 0 else tstack[m]))
        sel = [i for i in range(nq) if eff[i] == m]
        for f in ("ids", "scores", "count", "flags"):
            np.testing.assert_array_equal(got[f][sel], one[f][sel], err_msg=f"mask {m} {f}")
    if nq > 13:  # the query without terms adds no tail row: its main list comes back
        m13 = _np(main)
        for f in ("ids", "scores", "count"):
            np.testing.assert_array_equal(got[f][13], m13[f][13])


def test_one_chunk_tail_takes_a_null_workspace(gpu, oracle_mod, seg):
    """A tail of one chunk needs no workspace: size 0 and a null pointer are accepted by the entry
    point itself."""
    from audio_rag_amd import _armi
    from audio_rag_amd._armi import call, ptr, stream_handle
    from audio_rag_amd.retrieval.device import TopK

    csr, lists, main_idx = seg
    tail_n, nq, k = CHUNK, 9, 5
    oks = _masks(tail_n)
    q_mask = _q_mask(nq, len(oks))
    q = tuple(_dev(a, gpu) for a in _query_csr(lists[:nq]))
    t_ip, t_ix, t_iv = (_dev(a, gpu) for a in _rows(csr, MAIN, MAIN + tail_n))
    mstack, tstack = _stacks(oks, tail_n, gpu)
    qm = _dev(np.asarray(q_mask, np.int32), gpu)
    main = main_idx.topk_masks(*q, k, mstack, qm)
    assert int(_armi.query("armi_sparse_tail_workspace_bytes", tail_n, nq, k)) == 0
    out = TopK.empty(nq, k, gpu, rank=False)
    call("armi_sparse_tail_topk_qmask", ptr(t_ip), ptr(t_ix), ptr(t_iv), tail_n, MAIN, ptr(q[0]),
         ptr(q[1]), ptr(q[2]), nq, k, ptr(tstack), int(tstack.shape[1]), ptr(qm), len(oks),
         ptr(main.scores), ptr(main.ids), ptr(main.count), ptr(main.flags), ptr(out.scores),
         ptr(out.ids), ptr(out.count), ptr(out.flags), None, 0, stream_handle())
    _assert_oracle(_np(out), _oracle_lists(oracle_mod, csr, lists, oks, q_mask, tail_n), k)
    # outputs that alias the main list are refused before any device work
    with pytest.raises(_armi.ArmiError, match="alias") as e:
        call("armi_sparse_tail_topk_qmask", ptr(t_ip), ptr(t_ix), ptr(t_iv), tail_n, MAIN,
             ptr(q[0]), ptr(q[1]), ptr(q[2]), nq, k, ptr(tstack), int(tstack.shape[1]), ptr(qm),
             len(oks), ptr(main.scores), ptr(main.ids), ptr(main.count), ptr(main.flags),
             ptr(main.scores), ptr(out.ids), ptr(out.count), ptr(out.flags), None, 0,
             stream_handle())
    assert e.value.code == _armi.ARMI_ERR_INVALID


def test_no_masks_at_all(gpu, oracle_mod, seg):
    csr, lists, main_idx = seg
    tail_n, nq, k = 2 * CHUNK + 70, 9, 5
    q = tuple(_dev(a, gpu) for a in _query_csr(lists[:nq]))
    tail = _tail(_rows(csr, MAIN, MAIN + tail_n), gpu)
    main = main_idx.topk(*q, k)
    empty = torch.empty((0, (tail_n + 63) // 64), dtype=torch.int64, device=gpu)
    got = _np(tail.tail_topk_masks(*q, k, main, empty, _dev(np.full(nq, -1, np.int32), gpu)))
    want = _np(tail.tail_topk(*q, k, main))
    for f in ("ids", "scores", "count", "flags"):
        np.testing.assert_array_equal(got[f], want[f])
