"""A live retriever over the append-only sparse tail (TailSparseIndex): sparse and hybrid searches
after every append against the CPU oracle over everything added so far and against a retriever
without the knob, with and without a metadata filter, with the row-list planner on as well, the
captured single-query search and the QueryBatcher (single submissions, filtered and not). A flush and a search build no native sparse index over the tail.

Parity bar of test_live_tail_gpu.py: ids, counts, float32 scores and RRF scores bit-identical.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCHES, NQ, K = (2048, 100, 100, 100, 300), 16, 5
TOTAL = sum(BATCHES)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(ok: np.ndarray) -> np.ndarray:
    words = np.zeros(max((len(ok) + 63) // 64, 1), dtype=np.uint64)
    for r in np.nonzero(ok)[0]:
        words[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return words


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    rows = oracle_mod.unit_fp16(TOTAL, 1024, seed=230)
    csr = oracle_mod.sparse_corpus(TOTAL, seed=231)
    sq = oracle_mod.sparse_queries(NQ, seed=232)
    qd = oracle_mod.unit_fp16(NQ, 1024, seed=233)
    return rows, csr, sq, qd


def _retriever(live: int, lists: int = 0):
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    return MI355XRetriever(RetrievalConfig(top_k=K, live_tail_rows=live, filter_list_rows=lists,
                                           reproduce_sparse_drop=False), 1024)


def _add(ret, corpus, lo, hi):
    rows, (ip, ix, iv), _, _ = corpus
    sparse = [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(lo, hi)]
    payloads = [{"text": f"c{r}", "start": r, "end": r + 1, "speaker": None,
                 "metadata": {"lecture": r % 3}} for r in range(lo, hi)]
    ret.add_arrays(rows[lo:hi].view(np.float16), payloads, sparse=sparse)


def _batch(corpus, gpu):
    from audio_rag_amd.retrieval.mi355x import QueryBatch

    _, _, (qi, qx, qv), qd = corpus
    return QueryBatch(dense=_dev(qd.view(np.float16), gpu), sparse_indptr=_dev(qi, gpu),
                      sparse_indices=_dev(qx, gpu), sparse_values=_dev(qv, gpu))


_oracle_cache = {}


def _oracle(o, corpus, n, mode, flt):
    key = (n, mode, None if flt is None else flt["lecture"])
    if key not in _oracle_cache:
        rows, (ip, ix, iv), (qi, qx, qv), qd = corpus
        mask = None if flt is None else _bits(np.arange(n) % 3 == flt["lecture"])
        k = 2 * K if mode == "hybrid" else K
        s = o.sparse_topk(ip[:n + 1], ix[:ip[n]], iv[:ip[n]], qi, qx, qv, k, row_mask=mask)
        if mode == "hybrid":
            d = o.dense_topk(rows[:n], qd, k, row_mask=mask)
            s = [o.rrf([d.ids[b, :d.count[b]].tolist(), s.ids[b, :s.count[b]].tolist()], K)
                 for b in range(NQ)]
        _oracle_cache[key] = s
    return _oracle_cache[key]


def _check_searches(o, corpus, gpu, rets, plain, n):
    """Sparse and hybrid search_batch of every retriever in `rets` against `plain` and the oracle."""
    qb = _batch(corpus, gpu)
    for flt in (None, {"lecture": 1}):
        for mode in ("sparse", "hybrid"):
            b, mb = plain.search_batch(qb, K, filter_metadata=flt, search_type=mode)
            ref = _oracle(o, corpus, n, mode, flt)
            for ret in rets:
                a, ma = ret.search_batch(qb, K, filter_metadata=flt, search_type=mode)
                assert ma == mb == mode
                torch.cuda.synchronize()
                cnt = a.count.cpu().numpy()
                np.testing.assert_array_equal(cnt, b.count.cpu().numpy())
                ids, ids_b = a.ids.cpu().numpy(), b.ids.cpu().numpy()
                sc, sc_b = ((x.rank if mode == "hybrid" else x.scores).cpu().numpy()
                            for x in (a, b))
                for q in range(NQ):
                    c = cnt[q]
                    msg = f"{mode} {flt} {q}"
                    np.testing.assert_array_equal(ids[q, :c], ids_b[q, :c], err_msg=msg)
                    np.testing.assert_array_equal(sc[q, :c], sc_b[q, :c], err_msg=msg)
                    if mode == "hybrid":
                        assert [(int(i), float(s)) for i, s in zip(ids[q, :c], sc[q, :c])] == \
                            [(int(i), float(s)) for i, s in ref[q]], (flt, q)
                    else:
                        assert c == ref.count[q]
                        np.testing.assert_array_equal(ids[q, :c], ref.ids[q, :c], err_msg=msg)
                        np.testing.assert_array_equal(sc[q, :c], ref.scores[q, :c], err_msg=msg)


def _check_single(o, corpus, live, n):
    """search(): the captured single-query graph over both segments, captured and replayed."""
    from audio_rag_amd.core import EmbeddingResult, SparseVector

    _, _, (qi, qx, qv), qd = corpus
    qf = qd.view(np.float16).astype(np.float32)
    for st in ("sparse", "hybrid"):
        ref = _oracle(o, corpus, n, st, None)
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


def _check_batcher(o, corpus, live, plain, n):
    """QueryBatcher over both segments: single submissions, with and without a filter, coalesced
    into search_batch calls; the live retriever's answers against the plain one's and the oracle."""
    from audio_rag_amd.core import EmbeddingResult, SparseVector
    from audio_rag_amd.retrieval.batcher import QueryBatcher

    _, _, (qi, qx, qv), qd = corpus
    qf = qd.view(np.float16).astype(np.float32)
    queries = [EmbeddingResult(dense=qf[q].tolist(),
                               sparse=SparseVector(qx[qi[q]:qi[q + 1]].tolist(),
                                                   qv[qi[q]:qi[q + 1]].tolist()))
               for q in range(NQ)]
    filters = [None if q % 2 else {"lecture": 1} for q in range(NQ)]
    for st in ("sparse", "hybrid"):
        answers = []
        for ret in (live, plain):
            with QueryBatcher(ret, search_type=st, max_batch=NQ, max_wait_ms=1.0) as qb:
                futures = [qb.submit(e, f) for e, f in zip(queries, filters)]
                answers.append([[(r.chunk.text, r.score) for r in f.result(timeout=60)]
                                for f in futures])
        for q in range(NQ):
            ref = _oracle(o, corpus, n, st, filters[q])
            if st == "hybrid":
                want = [(f"c{p}", float(s)) for p, s in ref[q]]
            else:
                want = [(f"c{p}", float(s)) for p, s in
                        zip(ref.ids[q, :ref.count[q]], ref.scores[q, :ref.count[q]])]
            assert answers[0][q] == answers[1][q] == want, (st, q, filters[q])


def test_live_sparse_tail_appends_without_a_native_index(gpu, oracle_mod, corpus, monkeypatch):
    from audio_rag_amd.retrieval.device import TailSparseIndex

    monkeypatch.delenv("ARMI_TAIL_PASS", raising=False)
    live, lists, plain = _retriever(256), _retriever(256, 16384), _retriever(0)
    rets = (live, lists)
    n, mains = 0, []
    for i, size in enumerate(BATCHES):
        for r in (*rets, plain):
            _add(r, corpus, n, n + size)
        n += size
        _check_searches(oracle_mod, corpus, gpu, rets, plain, n)
        seg = live.collection().segments()
        mains.append(seg.sparse)
        if 1 <= i <= 3:  # batches 2-4 went to the tail
            for r in rets:
                ts = r.collection().segments().tail_sparse
                assert isinstance(ts, TailSparseIndex)
                assert ts.n_rows == n - BATCHES[0] and ts.ordinal_base == BATCHES[0]
                # neither the flush nor any search built a native sparse index over the tail
                assert not ts.general_built
            assert seg.sparse is mains[0] and seg.tail.n_rows == seg.tail_sparse.n_rows
            ip = corpus[1][0]
            assert int(seg.tail_sparse.indptr[-1]) == ip[n] - ip[BATCHES[0]]
        if i == 1:
            _check_single(oracle_mod, corpus, live, n)
            for r in rets:  # (with the row-list planner on, the filtered queries go through it)
                _check_batcher(oracle_mod, corpus, r, plain, n)
                ts = r.collection().segments().tail_sparse
                assert ts.n_rows == 100 and not ts.general_built
            assert not live.collection().segments().tail_sparse.general_built
        if i == 2:
            # the general path, forced: the same answers, and only now a native index exists ...
            monkeypatch.setenv("ARMI_TAIL_PASS", "general")
            _check_searches(oracle_mod, corpus, gpu, (live,), plain, n)
            monkeypatch.delenv("ARMI_TAIL_PASS")
            ts = seg.tail_sparse
            assert ts.general_built
    # ... which the next append (batch 4) dropped again: checked above for i == 3.
    # batch 5 did not fit: the tail was folded into new main indexes
    assert mains[4] is not mains[0]
    for r in rets:
        r.collection().compact()
        seg = r.collection().segments()
        assert seg.main_rows == TOTAL and seg.tail is None and seg.tail_sparse is None
    _check_searches(oracle_mod, corpus, gpu, rets, plain, n)


def test_compact_with_rows_in_the_tail(gpu, oracle_mod, corpus):
    """compact() while the tail holds rows: the device-side fold consumes the tail's CSR."""
    live, plain = _retriever(256), _retriever(0)
    n = 0
    for size in BATCHES[:3]:
        for r in (live, plain):
            _add(r, corpus, n, n + size)
        n += size
        live.collection().segments()
    seg = live.collection().segments()
    assert seg.tail_sparse.n_rows == 200 and not seg.tail_sparse.general_built
    live.collection().compact()
    seg = live.collection().segments()
    assert seg.main_rows == n and seg.tail is None and seg.tail_sparse is None
    _check_searches(oracle_mod, corpus, gpu, (live,), plain, n)
