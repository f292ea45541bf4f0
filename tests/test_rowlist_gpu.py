"""Row-list top-k on the GPU (armi_dense_rowlist_topk / armi_sparse_rowlist_topk through
DenseIndex.topk_rows / SparseIndex.topk_rows): ranking given rows must give, bit for bit, what the
masked scan of the whole index gives for the mask of those rows, and what the CPU oracle gives.

Every comparison is exact on ids, scores, rank (dense) and count. N = 2,085 rows (ragged tiles and
mask words), ordinal_base = 3; CHUNK is the kernels' chunk size (kRowlistChunk / kRlChunk).
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, BASE, CHUNK, NQ = 2085, 3, 512, 70
BAD = 700                                  # a row with a component outside the fp16 domain
DUPS = [10, 509, 511, 512, 514, 1030]      # copies of query 0's vector, across the chunk boundary


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(ok: np.ndarray) -> np.ndarray:
    words = np.zeros(max((len(ok) + 63) // 64, 1), dtype=np.uint64)
    for r in np.nonzero(ok)[0]:
        words[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return words


def _mask_of(rows: np.ndarray, n: int = N) -> np.ndarray:
    ok = np.zeros(n, dtype=bool)
    ok[rows] = True
    return _bits(ok)


def _np(out, fields=("ids", "scores", "rank", "count", "flags")):
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in fields}


def _lists(k: int, seed: int, n: int = N, must=()) -> list[np.ndarray]:
    """Ascending unique row lists of the lengths the kernels treat differently: 0, 1, k - 1, k, one
    below / at / one above the chunk size, two chunks and a remainder, every row; then a list no
    query uses. `must` rows are forced into the two-chunk list."""
    rng = np.random.default_rng(seed)
    out = []
    for m in (0, 1, k - 1, k, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 37, n):
        m = min(m, n)
        rows = np.sort(rng.choice(n, size=m, replace=False))
        if m == 2 * CHUNK + 37:
            rows = np.unique(np.concatenate([rows[:m - len(must)], np.asarray(must, dtype=rows.dtype)]))
        out.append(rows.astype(np.int32))
    out.append(np.sort(rng.choice(n, size=33, replace=False)).astype(np.int32))  # unused
    return out


def _encode(lists, gpu):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    rows = np.concatenate(lists).astype(np.int32)
    return _dev(ptr, gpu), _dev(rows, gpu), max(len(x) for x in lists)


def _q_list(nq: int, n_used: int, shift: int = 0) -> np.ndarray:
    """Every used list when nq allows, several queries per list; the last list stays unused."""
    return ((np.arange(nq) + shift) % n_used).astype(np.int32)


def _assert_equal(got, ref, msg=""):
    """got: this call's arrays; ref: arrays of the masked scan or the oracle for the same queries."""
    np.testing.assert_array_equal(got["count"], ref["count"], err_msg=msg)
    np.testing.assert_array_equal(got["ids"], ref["ids"], err_msg=msg)
    for b, c in enumerate(ref["count"]):
        for f in ("scores", "rank"):
            if f in got and f in ref and ref[f] is not None:
                np.testing.assert_array_equal(got[f][b, :c], ref[f][b, :c], err_msg=f"{msg} {f} q{b}")
        assert (got["ids"][b, c:] == -1).all() and np.isneginf(got["scores"][b, c:]).all()


def _oracle_arrays(ref):
    ids = ref.ids.copy()
    for b, c in enumerate(ref.count):
        ids[b, c:] = -1
    return {"ids": ids, "scores": ref.scores, "rank": ref.rank, "count": ref.count}


# ------------------------------------------------------------------------------------- dense

@pytest.fixture(scope="module")
def dense(gpu, oracle_mod):
    """dim -> (rows uint16, queries uint16, DenseIndex): one row outside the fp16 domain, copies of
    query 0's vector on both sides of a chunk boundary."""
    from audio_rag_amd.retrieval.device import DenseIndex

    out = {}
    for dim in (256, 1024):
        rows = oracle_mod.unit_fp16(N, dim, seed=300 + dim).copy()
        qs = oracle_mod.unit_fp16(NQ, dim, seed=301 + dim)
        rows[DUPS] = qs[0]
        rows[BAD, 5] = 0x4400  # 4.0: |x| >= 2
        idx = DenseIndex(_dev(rows.view(np.float16), gpu), ordinal_base=BASE)
        assert idx.invalid_rows() == 1
        out[dim] = (rows, qs, idx)
    return out


def _check_dense(oracle_mod, gpu, rows, qs, idx, k, lists, q_list, n=N, base=BASE, masked=True):
    from audio_rag_amd import _armi

    nq = len(q_list)
    q = _dev(qs[:nq].view(np.float16), gpu)
    ptr, lrows, longest = _encode(lists, gpu)
    got = _np(idx.topk_rows(q, k, ptr, lrows, _dev(q_list, gpu), longest))
    assert (got["flags"] == _armi.ARMI_FLAG_ROWLIST).all()
    for l in np.unique(q_list):
        sel = np.nonzero(q_list == l)[0]
        mine = {f: got[f][sel] for f in ("ids", "scores", "rank", "count")}
        mask = _mask_of(lists[l], n)
        ref = oracle_mod.dense_topk(rows, qs[sel], k, row_mask=mask, ordinal_base=base)
        _assert_equal(mine, _oracle_arrays(ref), f"oracle, list {l} ({len(lists[l])} rows)")
        assert (mine["count"] <= len(lists[l])).all()
        if masked:
            scan = _np(idx.topk(_dev(qs[sel].view(np.float16), gpu), k,
                                row_mask=_dev(mask.view(np.int64), gpu)))
            _assert_equal(mine, scan, f"masked scan, list {l} ({len(lists[l])} rows)")
    return got


@pytest.mark.parametrize("dim", [256, 1024])
@pytest.mark.parametrize("k", [1, 5, 40, 240])
def test_dense_rows_equal_masked_scan_and_oracle(gpu, oracle_mod, dense, dim, k):
    rows, qs, idx = dense[dim]
    lists = _lists(k, seed=k, must=[BAD] + DUPS)
    got = _check_dense(oracle_mod, gpu, rows, qs, idx, k, lists, _q_list(NQ, len(lists) - 1))
    assert not (got["ids"] == BASE + BAD).any()  # listed twice (two-chunk list, every row)
    # query 0 ranks list 0 (empty), query 8 every row
    assert got["count"][0] == 0 and got["count"][8] == min(k, N - 1)


@pytest.mark.parametrize("nq", [1, 3, 64])
def test_dense_rows_query_counts(gpu, oracle_mod, dense, nq):
    rows, qs, idx = dense[1024]
    lists = _lists(5, seed=50 + nq)
    # 1 query: every row; 3 queries: two share the two-chunk list, one ranks the chunk-sized list
    q_list = {1: np.array([8]), 3: np.array([7, 5, 7])}.get(nq, _q_list(nq, len(lists) - 1, 4))
    _check_dense(oracle_mod, gpu, rows, qs, idx, 5, lists, q_list.astype(np.int32))


@pytest.mark.parametrize("k", [1, 4, 5, 6, 240])
def test_dense_rows_exact_duplicates_by_ascending_ordinal(gpu, oracle_mod, dense, k):
    """Six copies of query 0's vector at rows that straddle the first chunk boundary (list
    positions = rows in the every-row list) and, for k = 4..6, the k-th position."""
    rows, qs, idx = dense[1024]
    lists = [np.arange(N, dtype=np.int32), np.array(DUPS[1:], dtype=np.int32)]
    got = _check_dense(oracle_mod, gpu, rows, qs, idx, k, lists, np.array([0, 1, 0], np.int32))
    np.testing.assert_array_equal(got["ids"][0, :min(k, 6)], BASE + np.array(DUPS[:k]))
    np.testing.assert_array_equal(got["ids"][1, :min(k, 5)], BASE + np.array(DUPS[1:1 + k]))
    assert len(set(got["rank"][0, :min(k, 6)].tolist())) == 1


def test_dense_rows_on_a_tail_index(gpu, oracle_mod):
    """The same call on a growable segment (no int8 image) holding 100 appended rows."""
    from audio_rag_amd.retrieval.device import TailIndex

    rows = oracle_mod.unit_fp16(100, 1024, seed=330).copy()
    qs = oracle_mod.unit_fp16(6, 1024, seed=331)
    rows[[3, 64, 99]] = qs[1]
    tail = TailIndex(1024, 256, BASE, gpu)
    tail.append(_dev(rows[:37].view(np.float16), gpu))
    tail.append(_dev(rows[37:].view(np.float16), gpu))
    rng = np.random.default_rng(4)
    lists = [np.arange(100, dtype=np.int32), np.zeros(0, np.int32),
             np.sort(rng.choice(100, 41, replace=False)).astype(np.int32)]
    for k in (5, 240):
        _check_dense(oracle_mod, gpu, rows, qs, tail, k, lists,
                     np.array([0, 0, 1, 2, 2, 0], np.int32), n=100)


def test_topk_rows_argument_checks(gpu, oracle_mod, dense):
    rows, qs, idx = dense[256]
    q = _dev(qs[:2].view(np.float16), gpu)
    ptr, lrows, longest = _encode([np.arange(5, dtype=np.int32)], gpu)
    ql = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="k must be"):
        idx.topk_rows(q, 241, ptr, lrows, ql, longest)
    with pytest.raises(ValueError, match="list_rows"):
        idx.topk_rows(q, 5, ptr, lrows.long(), ql, longest)
    with pytest.raises(ValueError, match="q_list"):
        idx.topk_rows(q, 5, ptr, lrows, torch.zeros(3, dtype=torch.int32), longest)
    with pytest.raises(ValueError, match=r"q_list entries"):
        idx.topk_rows(q, 5, ptr, lrows, torch.tensor([0, 1], dtype=torch.int32), longest)
    with pytest.raises(ValueError, match="max_list_rows"):
        idx.topk_rows(q, 5, ptr, lrows, ql, N + 1)
    with pytest.raises(ValueError, match="queries"):
        idx.topk_rows(q.float(), 5, ptr, lrows, ql, longest)


# ------------------------------------------------------------------------------------ sparse

@pytest.fixture(scope="module")
def sparse(gpu, oracle_mod):
    """(corpus CSR, query CSR, SparseIndex with the MFMA filter off): rows without terms, 70
    queries of which one has no terms."""
    from audio_rag_amd.retrieval.device import SparseIndex

    ip, ix, iv = oracle_mod.sparse_corpus(N, seed=340)
    keep = np.ones(len(ix), dtype=bool)
    for r in (0, 5, 511, 512, 1500, N - 1):  # rows without terms
        keep[ip[r]:ip[r + 1]] = False
    lens = np.diff(ip)
    lens[[0, 5, 511, 512, 1500, N - 1]] = 0
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ix, iv = ix[keep], iv[keep]
    qi, qx, qv = oracle_mod.sparse_queries(NQ, seed=341)
    cut = np.ones(len(qx), dtype=bool)
    cut[qi[17]:qi[18]] = False   # query 17: no terms (it ranks every row below)
    qlens = np.diff(qi)
    qlens[17] = 0
    qi = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    qx, qv = qx[cut], qv[cut]
    idx = SparseIndex(_dev(ip, gpu), _dev(ix, gpu), _dev(iv, gpu), 250002, ordinal_base=BASE)
    idx.set_filter(False)
    return (ip, ix, iv), (qi, qx, qv), idx


def _sub_csr(csr, sel):
    qi, qx, qv = csr
    lens = np.diff(qi)[sel]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    take = np.concatenate([np.arange(qi[s], qi[s + 1]) for s in sel] + [np.zeros(0, np.int64)])
    take = take.astype(np.int64)
    return ptr, qx[take], qv[take]


def _check_sparse(oracle_mod, gpu, corpus, queries, idx, k, lists, q_list, masked=True, n=N):
    from audio_rag_amd import _armi

    ip, ix, iv = corpus
    nq = len(q_list)
    qi, qx, qv = _sub_csr(queries, np.arange(nq))
    pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])  # non-null arrays for empty queries
    ptr, lrows, longest = _encode(lists, gpu)
    got = _np(idx.topk_rows(_dev(qi, gpu), _dev(pad(qx), gpu), _dev(pad(qv), gpu), k, ptr, lrows,
                            _dev(q_list, gpu), longest), ("ids", "scores", "count", "flags"))
    assert (got["flags"] == _armi.ARMI_FLAG_ROWLIST).all()
    for l in np.unique(q_list):
        sel = np.nonzero(q_list == l)[0]
        mine = {f: got[f][sel] for f in ("ids", "scores", "count")}
        mask = _mask_of(lists[l], n)
        si, sx, sv = _sub_csr(queries, sel)
        ref = oracle_mod.sparse_topk(ip, ix, iv, si, sx, sv, k, row_mask=mask, ordinal_base=BASE)
        _assert_equal(mine, {"ids": _oracle_arrays(ref)["ids"], "scores": ref.scores,
                             "count": ref.count}, f"oracle, list {l} ({len(lists[l])} rows)")
        if masked:
            scan = _np(idx.topk(_dev(si, gpu), _dev(pad(sx), gpu), _dev(pad(sv), gpu), k,
                                row_mask=_dev(mask.view(np.int64), gpu)), ("ids", "scores", "count"))
            _assert_equal(mine, scan, f"masked scan, list {l} ({len(lists[l])} rows)")
    return got


@pytest.mark.parametrize("k", [1, 5, 40, 240])
def test_sparse_rows_equal_masked_scan_and_oracle(gpu, oracle_mod, sparse, k):
    corpus, queries, idx = sparse
    lists = _lists(k, seed=20 + k, must=[0, 5, 511, 512, 1500, N - 1])
    got = _check_sparse(oracle_mod, gpu, corpus, queries, idx, k, lists,
                        _q_list(NQ, len(lists) - 1))
    assert got["count"][17] == 0 and (got["ids"][17] == -1).all()  # the query without terms
    assert got["count"][0] == 0                                     # the empty list


@pytest.mark.parametrize("nq", [1, 3, 64])
def test_sparse_rows_query_counts(gpu, oracle_mod, sparse, nq):
    corpus, queries, idx = sparse
    lists = _lists(5, seed=60 + nq)
    q_list = {1: np.array([8]), 3: np.array([7, 5, 7])}.get(nq, _q_list(nq, len(lists) - 1, 4))
    _check_sparse(oracle_mod, gpu, corpus, queries, idx, 5, lists, q_list.astype(np.int32))


def test_sparse_rows_zero_and_negative_scores_are_results(gpu, oracle_mod):
    """Hand-made postings: a zero-valued posting and a zero query weight leave fewer than k rows
    with a positive score; rows that share a term rank with score 0 or below. Against the oracle
    and against idx.topk under the equivalent mask: first an index whose negative value keeps the
    MFMA filter off, then the same rows with that value positive, where the filter is usable and
    has to leave these queries (a zero weight, zero-valued postings) to the exact scan."""
    from audio_rag_amd.retrieval.device import SparseIndex

    rows = [([7, 9], [0.5, 0.25]),      # 0: positive
            ([7], [0.0]),               # 1: zero-valued posting -> score 0, a result
            ([11], [0.3]),              # 2: shares only the zero-weight term -> score 0, a result
            ([12], [0.9]),              # 3: no shared term -> not a result
            ([], []),                   # 4: no terms
            ([9, 11], [-0.75, 0.1]),    # 5: negative score, a result
            ([7, 9], [0.5, 0.25])]      # 6: ties row 0 -> after it
    ip = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
    ix = np.concatenate([r[0] for r in rows]).astype(np.int32)
    iv = np.concatenate([r[1] for r in rows]).astype(np.float32)
    queries = (np.array([0, 3, 3, 4], np.int32), np.array([7, 9, 11, 7], np.int32),
               np.array([0.2, 0.1, 0.0, 0.2], np.float32))  # (query 2: the second index only)
    idx = SparseIndex(_dev(ip, gpu), _dev(ix, gpu), _dev(iv, gpu), 64, ordinal_base=BASE)
    lists = [np.arange(7, dtype=np.int32), np.array([1, 2, 3, 4], np.int32)]
    got = _check_sparse(oracle_mod, gpu, (ip, ix, iv), queries, idx, 6, lists,
                        np.array([0, 0], np.int32), n=7)
    assert got["ids"][0, :5].tolist() == [BASE + 0, BASE + 6, BASE + 1, BASE + 2, BASE + 5]
    assert got["count"].tolist() == [5, 0] and got["scores"][0, 4] < 0
    assert got["scores"][0, 2] == 0 and got["scores"][0, 3] == 0
    got = _check_sparse(oracle_mod, gpu, (ip, ix, iv), queries, idx, 6, lists,
                        np.array([1, 1], np.int32), n=7)
    assert got["ids"][0, :2].tolist() == [BASE + 1, BASE + 2] and got["count"].tolist() == [2, 0]
    assert not idx.set_filter(True)  # (a negative value: not usable)
    iv = np.abs(iv)  # row 5 scores 0.075: behind rows 0 and 6, before the zero-score rows
    idx = SparseIndex(_dev(ip, gpu), _dev(ix, gpu), _dev(iv, gpu), 64, ordinal_base=BASE)
    assert idx.set_filter(True)
    # query 2 (term 7 alone, weight 0.2) is one the filter may answer: rows 0, 6 and the
    # zero-valued posting of row 1
    for l, want, want2 in ((0, [0, 6, 5, 1, 2], [0, 6, 1]), (1, [1, 2], [1])):
        got = _check_sparse(oracle_mod, gpu, (ip, ix, iv), queries, idx, 6, lists,
                            np.full(3, l, np.int32), n=7)
        assert got["ids"][0, :len(want)].tolist() == [BASE + r for r in want]
        assert got["ids"][2, :len(want2)].tolist() == [BASE + r for r in want2]
        assert got["count"].tolist() == [len(want), 0, len(want2)]
        assert (got["scores"][0, len(want) - 2:len(want)].view(np.uint32) == 0).all()  # +0.0
        assert got["scores"][2, len(want2) - 1:len(want2)].view(np.uint32)[0] == 0


def test_sparse_rows_negative_values(gpu, oracle_mod):
    from audio_rag_amd.retrieval.device import SparseIndex

    ip, ix, iv = oracle_mod.sparse_corpus(N, seed=350)
    iv = iv.copy()
    iv[::3] *= -1.0
    queries = oracle_mod.sparse_queries(16, seed=351)
    queries[2][::4] *= -1.0
    idx = SparseIndex(_dev(ip, gpu), _dev(ix, gpu), _dev(iv, gpu), 250002, ordinal_base=BASE)
    lists = _lists(40, seed=7)
    _check_sparse(oracle_mod, gpu, (ip, ix, iv), queries, idx, 40, lists,
                  _q_list(16, len(lists) - 1))


# ----------------------------------------------------------------------------------- capture

def test_topk_rows_under_graph_capture(gpu, oracle_mod, dense, sparse):
    """One dense and one sparse topk_rows call captured on a single stream, replayed twice."""
    rows, qs, didx = dense[1024]
    _, queries, sidx = sparse
    lists = _lists(5, seed=90)
    ptr, lrows, longest = _encode(lists, gpu)
    ql = _dev(_q_list(NQ, len(lists) - 1), gpu)
    q = _dev(qs.view(np.float16), gpu)
    qi, qx, qv = (_dev(a, gpu) for a in queries)
    eager_d = _np(didx.topk_rows(q, 5, ptr, lrows, ql, longest))
    eager_s = _np(sidx.topk_rows(qi, qx, qv, 5, ptr, lrows, ql, longest), ("ids", "scores", "count"))
    ws_d = torch.empty(didx.rowlist_workspace_bytes(NQ, 5, longest), dtype=torch.uint8, device=gpu)
    ws_s = torch.empty(sidx.rowlist_workspace_bytes(NQ, 5, longest), dtype=torch.uint8, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        didx.topk_rows(q, 5, ptr, lrows, ql, longest, workspace=ws_d)
        sidx.topk_rows(qi, qx, qv, 5, ptr, lrows, ql, longest, workspace=ws_s)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_d = didx.topk_rows(q, 5, ptr, lrows, ql, longest, workspace=ws_d)
        out_s = sidx.topk_rows(qi, qx, qv, 5, ptr, lrows, ql, longest, workspace=ws_s)
    for _ in range(2):
        for t in (*out_d.tensors(), *out_s.tensors()):
            t.zero_()
        graph.replay()
        got_d, got_s = _np(out_d), _np(out_s, ("ids", "scores", "count"))
        for f in ("ids", "scores", "rank", "count", "flags"):
            np.testing.assert_array_equal(got_d[f], eager_d[f], err_msg=f)
        for f in ("ids", "scores", "count"):
            np.testing.assert_array_equal(got_s[f], eager_s[f], err_msg=f)
