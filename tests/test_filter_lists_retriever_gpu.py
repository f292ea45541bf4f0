"""Per-query filters and the row-list planner through MI355XRetriever (filter_list_rows): a batch
of 70 queries carrying 40 distinct filters must get, query by query and bit for bit, what a
knob-off retriever returns when it is called once per filter; only TopK.flags tell the paths apart.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, DIM, NQ, K, KNOB = 3000, 256, 70, 5, 256
# None, a broad filter (1000 rows > the knob: masked scan), a two-condition filter, a filter
# without a match, then 36 recordings of 81 or 82 rows each: 40 distinct filters
FILTERS = ([None, {"speaker": 1}, {"audio_id": 3, "speaker": 0}, {"audio_id": 99}]
           + [{"audio_id": a} for a in range(36)])
QUERY_FILTERS = [FILTERS[i % len(FILTERS)] for i in range(NQ)]
PLANNED = np.array([f is not None and "audio_id" in f for f in QUERY_FILTERS])
MODES = ("dense", "sparse", "hybrid")


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    rows = oracle_mod.unit_fp16(N, DIM, seed=400)
    csr = oracle_mod.sparse_corpus(N, seed=401)
    sq = oracle_mod.sparse_queries(NQ, seed=402)
    qd = oracle_mod.unit_fp16(NQ, DIM, seed=403)
    return rows, csr, sq, qd


def _retriever(knob: int, live: int = 0):
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    return MI355XRetriever(RetrievalConfig(top_k=K, filter_list_rows=knob, live_tail_rows=live,
                                           reproduce_sparse_drop=False), DIM)


def _add(ret, corpus, lo, hi, hybrid=True):
    rows, (ip, ix, iv), _, _ = corpus
    sparse = [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(lo, hi)] if hybrid else None
    payloads = [{"text": f"c{r}", "start": r, "end": r + 1, "speaker": None,
                 "metadata": {"audio_id": r % 37, "speaker": r % 3}} for r in range(lo, hi)]
    ret.add_arrays(rows[lo:hi].view(np.float16), payloads, sparse=sparse)


def _batch(corpus, gpu, sel=None, sparse=True):
    """The queries `sel` (default: all) as a device batch built from the host arrays."""
    from audio_rag_amd.retrieval.mi355x import QueryBatch

    _, _, (qi, qx, qv), qd = corpus
    sel = np.arange(NQ) if sel is None else np.asarray(sel)
    dense = _dev(qd[sel].view(np.float16), gpu)
    if not sparse:
        return QueryBatch(dense=dense)
    ptr = np.concatenate([[0], np.cumsum(np.diff(qi)[sel])]).astype(np.int32)
    take = np.concatenate([np.arange(qi[s], qi[s + 1]) for s in sel]).astype(np.int64)
    return QueryBatch(dense=dense, sparse_indptr=_dev(ptr, gpu), sparse_indices=_dev(qx[take], gpu),
                      sparse_values=_dev(qv[take], gpu))


def _arrays(out, mode):
    torch.cuda.synchronize()
    sc = out.rank if mode == "hybrid" else out.scores
    got = {"ids": out.ids.cpu().numpy(), "scores": sc.cpu().numpy(),
           "count": out.count.cpu().numpy()}
    if mode in ("dense", "legacy_dense"):
        got["rank"] = out.rank.cpu().numpy()
    return got


_refs: dict = {}


def _reference(plain, corpus, gpu, mode, sparse=True):
    """Query-ordered arrays of the knob-off retriever called once per distinct filter, each call
    with the sub-batch of that filter's queries. Computed once per mode and shared."""
    key = (id(plain), mode)
    if key not in _refs:
        ref = None
        for f in FILTERS:
            sel = [i for i, qf in enumerate(QUERY_FILTERS) if qf is f]
            out, m = plain.search_batch(_batch(corpus, gpu, sel, sparse), K, filter_metadata=f,
                                        search_type=mode)
            got = _arrays(out, m)
            if ref is None:
                ref = {n: np.empty((NQ,) + a.shape[1:], dtype=a.dtype) for n, a in got.items()}
            for n, a in got.items():
                ref[n][sel] = a
        _refs[key] = ref
    return _refs[key]


def _assert_same(got, ref, msg):
    np.testing.assert_array_equal(got["count"], ref["count"], err_msg=msg)
    np.testing.assert_array_equal(got["ids"], ref["ids"], err_msg=msg)
    for n in ("scores", "rank"):
        if n in ref:
            for b, c in enumerate(ref["count"]):
                np.testing.assert_array_equal(got[n][b, :c], ref[n][b, :c], err_msg=f"{msg} {n} q{b}")


def _check_batched(ret, plain, corpus, gpu, modes=MODES, sparse=True, planned=PLANNED):
    from audio_rag_amd import _armi

    for mode in modes:
        out, m = ret.search_batch(_batch(corpus, gpu, sparse=sparse), K,
                                  filter_metadata=QUERY_FILTERS, search_type=mode)
        _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, mode, sparse), mode)
        flags = out.flags.cpu().numpy()
        np.testing.assert_array_equal((flags & _armi.ARMI_FLAG_ROWLIST) != 0, planned, err_msg=mode)
        by = {repr(g.filter): g for g in ret.last_plan}
        assert len(by) == len(FILTERS)
        assert by[repr({"audio_id": 99})].matches == 0 and by[repr({"speaker": 1})].matches == 1000


@pytest.fixture(scope="module")
def plain(corpus):
    ret = _retriever(0)
    _add(ret, corpus, 0, N)
    return ret


def test_mixed_filters_equal_one_call_per_filter(gpu, corpus, plain):
    ret = _retriever(KNOB)
    _add(ret, corpus, 0, N)
    _check_batched(ret, plain, corpus, gpu)
    # no match: count 0 on every branch
    out, _ = ret.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                              search_type="hybrid")
    count = out.count.cpu().numpy()
    assert (count[[i for i, f in enumerate(QUERY_FILTERS) if f == {"audio_id": 99}]] == 0).all()
    assert (count[PLANNED & (np.arange(NQ) % len(FILTERS) != 3)] == K).all()


def test_legacy_dense_collection(gpu, corpus):
    ret, ref = _retriever(KNOB), _retriever(0)
    _add(ret, corpus, 0, N, hybrid=False)
    _add(ref, corpus, 0, N, hybrid=False)
    out, m = ret.search_batch(_batch(corpus, gpu, sparse=False), K, filter_metadata=QUERY_FILTERS)
    assert m == "legacy_dense"
    _check_batched(ret, ref, corpus, gpu, modes=("dense",), sparse=False)


def test_live_collection_matches_straddle_main_and_tail(gpu, corpus, plain):
    ret = _retriever(KNOB, live=64)
    _add(ret, corpus, 0, N - 100)
    ret.collection().segments()  # first build
    _add(ret, corpus, N - 100, N)
    seg = ret.collection().segments()
    assert seg.main_rows == N - 100 and seg.tail.n_rows == 100
    main, tail, m = ret.collection().segment_row_lists({"audio_id": 7}, KNOB)
    assert main.numel() > 0 and tail.numel() > 0 and main.numel() + tail.numel() == m
    _check_batched(ret, plain, corpus, gpu)
    ret.collection().compact()
    seg = ret.collection().segments()
    assert seg.main_rows == N and seg.tail is None
    main, tail, m2 = ret.collection().segment_row_lists({"audio_id": 7}, KNOB)
    assert tail is None and main.numel() == m2 == m  # the cached lists went with the fold
    _check_batched(ret, plain, corpus, gpu)


def test_knob_off_takes_the_list_form(gpu, corpus, plain):
    from audio_rag_amd import _armi

    for mode in MODES:
        out, m = plain.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                    search_type=mode)
        _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, mode), mode)
        assert not (out.flags.cpu().numpy() & _armi.ARMI_FLAG_ROWLIST).any()
        assert all(not g.rowlist and g.matches == -1 for g in plain.last_plan)


def _embedding(corpus, q):
    from audio_rag_amd.core import EmbeddingResult, SparseVector

    _, _, (qi, qx, qv), qd = corpus
    return EmbeddingResult(dense=qd[q].view(np.float16).astype(np.float32).tolist(),
                           sparse=SparseVector(qx[qi[q]:qi[q + 1]].tolist(),
                                               qv[qi[q]:qi[q + 1]].tolist()))


def test_search_with_a_filter_goes_through_the_planner(gpu, corpus, plain):
    ret = _retriever(KNOB)
    _add(ret, corpus, 0, N)
    for q in (1, 2, 3, 4, 9):
        for st in MODES:
            emb = _embedding(corpus, q)
            got = [(r.chunk.text, r.score) for r in ret.search(emb, K, filter_metadata=QUERY_FILTERS[q],
                                                               search_type=st)]
            want = [(r.chunk.text, r.score) for r in plain.search(emb, K, filter_metadata=QUERY_FILTERS[q],
                                                                  search_type=st)]
            assert got == want, (q, st)
            assert ret.last_plan[0].rowlist == bool(PLANNED[q])


def test_query_batcher_mixed_filter_stream(gpu, corpus, plain):
    from audio_rag_amd.retrieval.batcher import QueryBatcher

    ret = _retriever(KNOB)
    _add(ret, corpus, 0, N)
    with QueryBatcher(ret, top_k=K, search_type="hybrid", max_batch=64, max_wait_ms=50.0) as qb:
        futures = [qb.submit(_embedding(corpus, q), QUERY_FILTERS[q]) for q in range(NQ)]
        got = [[(r.chunk.text, r.score) for r in f.result(60)] for f in futures]
        assert qb.batches < NQ / 2  # mixed filters share batches (one search_batch per batch)
    for q in range(NQ):
        want = [(r.chunk.text, r.score) for r in plain.search(_embedding(corpus, q), K,
                                                              filter_metadata=QUERY_FILTERS[q],
                                                              search_type="hybrid")]
        assert got[q] == want, q
