"""Live ingest on the GPU: the growable fp16 segment (armi_index_create_tail / _append), the fused
tail pass (armi_dense_tail_topk) and a retriever with RetrievalConfig.live_tail_rows, against the
CPU oracle over the concatenation of everything added so far.

Parity bar, as in test_dense_gpu.py / test_sparse_rrf_gpu.py: ids, counts, float64 ranking keys
and float32 scores bit-identical to the oracle.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAIN = 4096


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _np(out):
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "rank", "count", "flags")}


def _assert_same(got, ref, nq=None):
    nq = ref.count.shape[0] if nq is None else nq
    np.testing.assert_array_equal(got["count"], ref.count[:nq])
    for b in range(nq):
        c = ref.count[b]
        np.testing.assert_array_equal(got["ids"][b, :c], ref.ids[b, :c], err_msg=f"query {b}")
        np.testing.assert_array_equal(got["rank"][b, :c], ref.rank[b, :c], err_msg=f"query {b}")
        np.testing.assert_array_equal(got["scores"][b, :c], ref.scores[b, :c], err_msg=f"query {b}")
        assert (got["ids"][b, c:] == -1).all()


def _bits(ok: np.ndarray) -> np.ndarray:
    words = np.zeros(max((len(ok) + 63) // 64, 1), dtype=np.uint64)
    for r in np.nonzero(ok)[0]:
        words[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return words


def _tail(rows_u16, gpu, base, capacity=None):
    from audio_rag_amd.retrieval.device import TailIndex

    t = TailIndex(rows_u16.shape[1], capacity or max(len(rows_u16), 1), base, gpu)
    t.append(_dev(rows_u16.view(np.float16), gpu))
    return t


# ------------------------------------------------------------------------------------ append

@pytest.mark.parametrize("dim", [256, 1024])
def test_append_pieces_match_an_index_built_at_once(gpu, oracle_mod, dim):
    from audio_rag_amd import _armi
    from audio_rag_amd.retrieval.device import DenseIndex, TailIndex

    rows = oracle_mod.unit_fp16(199 + 70, dim, seed=70 + dim)
    qs = oracle_mod.unit_fp16(8, dim, seed=71 + dim)
    q = _dev(qs.view(np.float16), gpu)
    tail = TailIndex(dim, 256, 1000, gpu)
    assert tail.capacity == 256 and tail.n_rows == 0
    n = 0
    for piece in (1, 31, 33, 64, 70):
        tail.append(_dev(rows[n:n + piece].view(np.float16), gpu))
        n += piece
        assert tail.n_rows == n
        whole = DenseIndex(_dev(rows[:n].view(np.float16), gpu), ordinal_base=1000)
        for a, b in zip(tail.norms(), whole.norms()):
            assert torch.equal(a, b)
        for k in (5, 240):
            assert tail.scan_form(8, k) == _armi.SCAN_FP16
            _assert_same(_np(tail.topk(q, k)), oracle_mod.dense_topk(rows[:n], qs, k, ordinal_base=1000))
    assert n == 199
    with pytest.raises(_armi.ArmiError, match="capacity"):
        tail.append(_dev(rows[199:269].view(np.float16), gpu))
    assert tail.n_rows == 199 and int(_armi.query("armi_index_rows", tail.handle)) == 199


def test_appended_invalid_row_is_counted_and_never_returned(gpu, oracle_mod):
    rows = oracle_mod.unit_fp16(40, 256, seed=80).copy()
    rows[17, 3] = 0x7C00  # +inf
    qs = oracle_mod.unit_fp16(4, 256, seed=81)
    tail = _tail(rows, gpu, 0, capacity=64)
    assert tail.invalid_rows() == 1
    got = _np(tail.topk(_dev(qs.view(np.float16), gpu), 240))
    assert (got["count"] == 39).all() and not (got["ids"] == 17).any()
    keep = np.ones(40, dtype=bool)
    keep[17] = False
    _assert_same(got, oracle_mod.dense_topk(rows, qs, 240, row_mask=_bits(keep)))


# --------------------------------------------------------------------------------- tail pass

@pytest.fixture(scope="module")
def segs(gpu, oracle_mod):
    """dim -> (rows of main + the largest tail, 70 queries, the main DenseIndex)."""
    from audio_rag_amd.retrieval.device import DenseIndex

    out = {}
    for dim in (1024, 256):
        rows = oracle_mod.unit_fp16(MAIN + 1000, dim, seed=90 + dim)
        qs = oracle_mod.unit_fp16(70, dim, seed=91 + dim)
        out[dim] = (rows, qs, DenseIndex(_dev(rows[:MAIN].view(np.float16), gpu)))
    return out


_refs = {}


def _ref(oracle_mod, segs, dim, tail_n, k):
    key = (dim, tail_n, k)
    if key not in _refs:
        rows, qs, _ = segs[dim]
        _refs[key] = oracle_mod.dense_topk(rows[:MAIN + tail_n], qs, k)
    return _refs[key]


def _both_paths(monkeypatch, tail, q, k, main, mask=None):
    monkeypatch.delenv("ARMI_TAIL_PASS", raising=False)
    fused = _np(tail.tail_topk(q, k, main, row_mask=mask))
    monkeypatch.setenv("ARMI_TAIL_PASS", "general")
    general = _np(tail.tail_topk(q, k, main, row_mask=mask))
    monkeypatch.delenv("ARMI_TAIL_PASS")
    c = fused["count"]
    np.testing.assert_array_equal(c, general["count"])
    for b in range(len(c)):
        for f in ("ids", "scores", "rank"):
            np.testing.assert_array_equal(fused[f][b, :c[b]], general[f][b, :c[b]], err_msg=f)
    return fused


@pytest.mark.parametrize("tail_n,nq,k,dim",
                         [(t, b, k, 1024) for t in (1, 33, 1000) for b in (1, 64, 70)
                          for k in (5, 40, 240)] + [(33, 70, 40, 256)])
def test_tail_pass_matches_oracle_over_the_concatenation(gpu, oracle_mod, segs, monkeypatch,
                                                         tail_n, nq, k, dim):
    from audio_rag_amd import _armi

    rows, qs, main_idx = segs[dim]
    q = _dev(qs[:nq].view(np.float16), gpu)
    tail = _tail(rows[MAIN:MAIN + tail_n], gpu, MAIN)
    got = _both_paths(monkeypatch, tail, q, k, main_idx.topk(q, k))
    _assert_same(got, _ref(oracle_mod, segs, dim, tail_n, k), nq)
    # at most 84 survivors per query on these shapes (counted on the CPU with twice the delta):
    # nowhere near the list capacity, so no query may take the exhaustive pass
    assert (got["flags"] == _armi.ARMI_FLAG_CERTIFIED).all()


def test_tail_pass_with_row_masks_on_both_segments(gpu, oracle_mod, segs, monkeypatch):
    rows, qs, main_idx = segs[1024]
    rng = np.random.default_rng(5)
    for tail_n in (33, 1000):
        ok = rng.random(MAIN + tail_n) < 0.5
        m_main, m_tail = (_dev(_bits(x).view(np.int64), gpu) for x in (ok[:MAIN], ok[MAIN:]))
        q = _dev(qs.view(np.float16), gpu)
        tail = _tail(rows[MAIN:MAIN + tail_n], gpu, MAIN)
        for k in (5, 240):
            got = _both_paths(monkeypatch, tail, q, k, main_idx.topk(q, k, row_mask=m_main), m_tail)
            _assert_same(got, oracle_mod.dense_topk(rows[:MAIN + tail_n], qs, k, row_mask=_bits(ok)))


def test_main_list_shorter_than_k(gpu, oracle_mod, segs, monkeypatch):
    """A filter that leaves three main rows: the main list has no k-th key, the threshold is -inf
    and every enabled tail row is a survivor."""
    rows, qs, main_idx = segs[1024]
    ok = np.zeros(MAIN + 33, dtype=bool)
    ok[[5, 700, 4000]] = True
    ok[MAIN:] = True
    ok[MAIN + 4] = False
    m_main, m_tail = (_dev(_bits(x).view(np.int64), gpu) for x in (ok[:MAIN], ok[MAIN:]))
    q = _dev(qs[:8].view(np.float16), gpu)
    tail = _tail(rows[MAIN:MAIN + 33], gpu, MAIN)
    for k in (5, 40):
        main = main_idx.topk(q, k, row_mask=m_main)
        got = _both_paths(monkeypatch, tail, q, k, main, m_tail)
        _assert_same(got, oracle_mod.dense_topk(rows[:MAIN + 33], qs[:8], k, row_mask=_bits(ok)))


def test_overflowing_survivor_list_takes_the_exact_pass(gpu, oracle_mod, segs, monkeypatch):
    """More copies of the query vector than the survivor list holds: every copy ties and survives,
    the query is flagged FALLBACK and the copies come out by ascending ordinal."""
    from audio_rag_amd import _armi
    from audio_rag_amd.retrieval.device import TailIndex

    rows, qs, main_idx = segs[1024]
    n = TailIndex.list_cap() + 64
    trows = np.repeat(qs[:1], n, axis=0)
    q = _dev(qs[:2].view(np.float16), gpu)
    tail = _tail(trows, gpu, MAIN)
    for k in (5, 240):
        got = _both_paths(monkeypatch, tail, q, k, main_idx.topk(q, k))
        _assert_same(got, oracle_mod.dense_topk(np.concatenate([rows[:MAIN], trows]), qs[:2], k))
        np.testing.assert_array_equal(got["ids"][0], MAIN + np.arange(k))
        assert got["flags"][0] == _armi.ARMI_FLAG_FALLBACK
        assert got["flags"][1] == _armi.ARMI_FLAG_CERTIFIED


def test_tail_of_more_than_64_scan_workgroups(gpu, oracle_mod, segs, monkeypatch):
    """The finish kernel gathers the scan workgroups' lists 64 workgroups (16384 rows) at a time:
    a tail past that, with survivors on both sides of the boundary (copies of two queries)."""
    rows, qs, main_idx = segs[256]
    trows = oracle_mod.unit_fp16(16384 + 70, 256, seed=140).copy()
    trows[[3, 16383, 16384, 16450]] = qs[0]
    trows[[16390, 9000]] = qs[1]
    q = _dev(qs[:5].view(np.float16), gpu)
    tail = _tail(trows, gpu, MAIN)
    for k in (5, 40):
        got = _both_paths(monkeypatch, tail, q, k, main_idx.topk(q, k))
        _assert_same(got, oracle_mod.dense_topk(np.concatenate([rows[:MAIN], trows]), qs[:5], k))
    assert got["ids"][0, :4].tolist() == [MAIN + 3, MAIN + 16383, MAIN + 16384, MAIN + 16450]
    assert got["ids"][1, :2].tolist() == [MAIN + 9000, MAIN + 16390]


def test_same_vector_in_main_and_tail_main_first(gpu, oracle_mod, monkeypatch):
    from audio_rag_amd.retrieval.device import DenseIndex

    rows = oracle_mod.unit_fp16(MAIN + 33, 1024, seed=120).copy()
    qs = oracle_mod.unit_fp16(3, 1024, seed=121)
    rows[7] = qs[0]
    rows[MAIN] = qs[0]
    rows[MAIN + 20] = qs[0]
    main_idx = DenseIndex(_dev(rows[:MAIN].view(np.float16), gpu))
    q = _dev(qs.view(np.float16), gpu)
    tail = _tail(rows[MAIN:], gpu, MAIN)
    got = _both_paths(monkeypatch, tail, q, 5, main_idx.topk(q, 5))
    _assert_same(got, oracle_mod.dense_topk(rows, qs, 5))
    assert got["ids"][0, :3].tolist() == [7, MAIN, MAIN + 20]


# --------------------------------------------------------------------------------- retriever

N0, BATCHES, NQ, K = 2048, (2048, 100, 100, 100, 300), 16, 5
TOTAL = sum(BATCHES)


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    rows = oracle_mod.unit_fp16(TOTAL, 1024, seed=130)
    csr = oracle_mod.sparse_corpus(TOTAL, seed=131)
    sq = oracle_mod.sparse_queries(NQ, seed=132)
    qd = oracle_mod.unit_fp16(NQ, 1024, seed=133)
    return rows, csr, sq, qd


def _retriever(live: int):
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    return MI355XRetriever(RetrievalConfig(top_k=K, live_tail_rows=live,
                                           reproduce_sparse_drop=False), 1024)


def _add(ret, corpus, lo, hi):
    rows, (ip, ix, iv), _, _ = corpus
    sparse = [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(lo, hi)]
    payloads = [{"text": f"c{r}", "start": r, "end": r + 1, "speaker": None,
                 "metadata": {"lecture": r % 3}} for r in range(lo, hi)]
    ret.add_arrays(rows[lo:hi].view(np.float16), payloads, sparse=sparse)


def _batch(ret, corpus, gpu):
    from audio_rag_amd.retrieval.mi355x import QueryBatch

    _, _, (qi, qx, qv), qd = corpus
    return QueryBatch(dense=_dev(qd.view(np.float16), gpu), sparse_indptr=_dev(qi, gpu),
                      sparse_indices=_dev(qx, gpu), sparse_values=_dev(qv, gpu))


def _oracle(o, corpus, n, mode, flt):
    rows, (ip, ix, iv), (qi, qx, qv), qd = corpus
    mask = None if flt is None else _bits(np.arange(n) % 3 == flt["lecture"])
    k = 2 * K if mode == "hybrid" else K
    d = o.dense_topk(rows[:n], qd, k, row_mask=mask)
    if mode == "dense":
        return d
    s = o.sparse_topk(ip[:n + 1], ix[:ip[n]], iv[:ip[n]], qi, qx, qv, k, row_mask=mask)
    if mode == "sparse":
        return s
    return [o.rrf([d.ids[b, :d.count[b]].tolist(), s.ids[b, :s.count[b]].tolist()], K)
            for b in range(NQ)]


def _check_searches(o, corpus, gpu, live, plain, n):
    qb = _batch(live, corpus, gpu)
    for flt in (None, {"lecture": 1}):
        for mode in ("dense", "sparse", "hybrid"):
            a, ma = live.search_batch(qb, K, filter_metadata=flt, search_type=mode)
            b, mb = plain.search_batch(qb, K, filter_metadata=flt, search_type=mode)
            assert ma == mb == mode
            torch.cuda.synchronize()
            cnt = a.count.cpu().numpy()
            np.testing.assert_array_equal(cnt, b.count.cpu().numpy())
            ids, ids_b = a.ids.cpu().numpy(), b.ids.cpu().numpy()
            sc, sc_b = ((x.rank if mode == "hybrid" else x.scores).cpu().numpy() for x in (a, b))
            ref = _oracle(o, corpus, n, mode, flt)
            for q in range(NQ):
                c = cnt[q]
                np.testing.assert_array_equal(ids[q, :c], ids_b[q, :c], err_msg=f"{mode} {flt} {q}")
                np.testing.assert_array_equal(sc[q, :c], sc_b[q, :c], err_msg=f"{mode} {flt} {q}")
                if mode == "hybrid":
                    assert [(int(i), float(s)) for i, s in zip(ids[q, :c], sc[q, :c])] == \
                        [(int(i), float(s)) for i, s in ref[q]], (flt, q)
                else:
                    assert c == ref.count[q]
                    np.testing.assert_array_equal(ids[q, :c], ref.ids[q, :c], err_msg=f"{mode} {flt} {q}")
                    np.testing.assert_array_equal(sc[q, :c], ref.scores[q, :c],
                                                  err_msg=f"{mode} {flt} {q}")


def test_retriever_appends_without_rebuilding(gpu, oracle_mod, corpus):
    from audio_rag_amd.core import EmbeddingResult, SparseVector

    live, plain = _retriever(256), _retriever(0)
    _, _, (qi, qx, qv), qd = corpus
    n, mains = 0, []
    for i, size in enumerate(BATCHES):
        _add(live, corpus, n, n + size)
        _add(plain, corpus, n, n + size)
        n += size
        _check_searches(oracle_mod, corpus, gpu, live, plain, n)
        seg = live.collection().segments()
        mains.append((seg.dense, seg.sparse))
        tail_rows = seg.tail.n_rows if seg.tail is not None else 0
        assert seg.main_rows + tail_rows == n
        ps = plain.collection().segments()
        assert ps.tail is None and ps.main_rows == n
        if i == 1:  # single-query search(): the captured-graph path over both segments
            qf = qd.view(np.float16).astype(np.float32)
            for st in ("dense", "hybrid"):
                ref = _oracle(oracle_mod, corpus, n, st, None)
                for q in range(3):
                    emb = EmbeddingResult(dense=qf[q].tolist(),
                                          sparse=SparseVector(qx[qi[q]:qi[q + 1]].tolist(),
                                                              qv[qi[q]:qi[q + 1]].tolist()))
                    for _ in range(2):  # capture, then replay
                        got = [(r.chunk.text, r.score) for r in live.search(emb, K, search_type=st)]
                        if st == "hybrid":
                            assert got == [(f"c{p}", float(s)) for p, s in ref[q]]
                        else:
                            assert got == [(f"c{p}", float(s)) for p, s in
                                           zip(ref.ids[q, :ref.count[q]], ref.scores[q, :ref.count[q]])]
    # batches 2-4 went to the tail: the main indexes are the objects of the first build
    for later in mains[1:4]:
        assert later[0] is mains[0][0] and later[1] is mains[0][1]
    # batch 5 did not fit: the tail was folded into new main indexes
    assert mains[4][0] is not mains[0][0] and mains[4][1] is not mains[0][1]
    seg = live.collection().segments()
    assert seg.main_rows >= TOTAL - BATCHES[4]
    assert (seg.tail.n_rows if seg.tail is not None else 0) in (0, BATCHES[4])
    live.collection().compact()
    seg = live.collection().segments()
    assert seg.main_rows == TOTAL and seg.tail is None
    _check_searches(oracle_mod, corpus, gpu, live, plain, n)


def test_live_collection_persists_and_serves_every_point(gpu, oracle_mod, corpus, tmp_path):
    from audio_rag_amd.retrieval.batcher import StreamServer

    rows, _, _, qd = corpus
    ret = _retriever(256)
    _add(ret, corpus, 0, 500)
    ret.collection().segments()  # first build
    _add(ret, corpus, 500, 570)
    seg = ret.collection().segments()
    assert seg.main_rows == 500 and seg.tail.n_rows == 70
    want = oracle_mod.dense_topk(rows[:570], qd, K)

    ret.save_collection(tmp_path / "store")
    other = _retriever(256)
    other.load_collection(tmp_path / "store")
    assert other.count() == 570
    out, _ = other.search_batch(_batch(other, corpus, gpu), K, search_type="dense")
    _assert_same({**_np(out)}, want)

    # the native server binds one index: opening it folds the tail in first
    with StreamServer(ret, max_batch=8, max_wait_ms=0.5) as srv:
        tickets = [srv.submit_arrays(qd[i].view(np.float16)) for i in range(NQ)]
        got = [srv.result(t) for t in tickets]
    for i in range(NQ):
        assert [r.chunk.text for r in got[i]] == [f"c{p}" for p in want.ids[i, :want.count[i]]]
        assert [r.score for r in got[i]] == [float(s) for s in want.scores[i, :want.count[i]]]
    seg = ret.collection().segments()
    assert seg.main_rows == 570 and seg.tail is None
