"""Broad per-query filters through MI355XRetriever (filter_query_masks): a batch mixing broad
filters, unfiltered queries, a selective filter and a filter without a match must get, query by
query and bit for bit, what a knob-off retriever returns when it is called once per filter; only
the plan (last_plan) and, in dense mode, TopK.flags (ARMI_FLAG_QMASK) tell the paths apart."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, DIM, NQ, K, KNOB = 4000, 256, 70, 5, 256
# speaker: 4 values, 1000 rows each (broad); audio_id: 80 values, 50 rows each (selective)
FILTERS = [{"speaker": 0}, None, {"speaker": 1}, {"audio_id": 7}, {"speaker": 2, "kind": 0},
           {"audio_id": 999}, {"speaker": 3}]
QUERY_FILTERS = [FILTERS[i % len(FILTERS)] for i in range(NQ)]
MODES = ("dense", "hybrid", "sparse")


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    rows = oracle_mod.unit_fp16(N, DIM, seed=500)
    csr = oracle_mod.sparse_corpus(N, seed=501)
    sq = oracle_mod.sparse_queries(NQ, seed=502)
    qd = oracle_mod.unit_fp16(NQ, DIM, seed=503)
    return rows, csr, sq, qd


def _retriever(masks: bool, knob: int = 0, live: int = 0):
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    return MI355XRetriever(RetrievalConfig(top_k=K, filter_query_masks=masks, filter_list_rows=knob,
                                           live_tail_rows=live, reproduce_sparse_drop=False), DIM)


def _add(ret, corpus, lo, hi):
    rows, (ip, ix, iv), _, _ = corpus
    sparse = [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(lo, hi)]
    payloads = [{"text": f"c{r}", "start": r, "end": r + 1, "speaker": None,
                 "metadata": {"audio_id": r % 80, "speaker": r % 4, "kind": r % 3}}
                for r in range(lo, hi)]
    ret.add_arrays(rows[lo:hi].view(np.float16), payloads, sparse=sparse)


def _batch(corpus, gpu, sel=None):
    from audio_rag_amd.retrieval.mi355x import QueryBatch

    _, _, (qi, qx, qv), qd = corpus
    sel = np.arange(NQ) if sel is None else np.asarray(sel)
    ptr = np.concatenate([[0], np.cumsum(np.diff(qi)[sel])]).astype(np.int32)
    take = np.concatenate([np.arange(qi[s], qi[s + 1]) for s in sel]).astype(np.int64)
    return QueryBatch(dense=_dev(qd[sel].view(np.float16), gpu), sparse_indptr=_dev(ptr, gpu),
                      sparse_indices=_dev(qx[take], gpu), sparse_values=_dev(qv[take], gpu))


def _arrays(out, mode):
    torch.cuda.synchronize()
    sc = out.rank if mode == "hybrid" else out.scores
    got = {"ids": out.ids.cpu().numpy(), "scores": sc.cpu().numpy(),
           "count": out.count.cpu().numpy()}
    if mode == "dense":
        got["rank"] = out.rank.cpu().numpy()
    return got


_refs: dict = {}


def _reference(plain, corpus, gpu, mode, k=K, filters=None):
    """Query-ordered arrays of the knob-off retriever called once per distinct filter with that
    filter's queries. Computed once per (mode, k, filter list) and shared."""
    filters = QUERY_FILTERS if filters is None else filters
    key = (mode, k, repr(filters))
    if key not in _refs:
        ref = None
        distinct = []
        for f in filters:
            if f not in distinct:
                distinct.append(f)
        for f in distinct:
            sel = [i for i, qf in enumerate(filters) if qf == f]
            out, m = plain.search_batch(_batch(corpus, gpu, sel), k, filter_metadata=f,
                                        search_type=mode)
            got = _arrays(out, m)
            if ref is None:
                ref = {n: np.empty((len(filters),) + a.shape[1:], dtype=a.dtype)
                       for n, a in got.items()}
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


def _qmask_flags(out):
    from audio_rag_amd import _armi

    return (out.flags.cpu().numpy() & _armi.ARMI_FLAG_QMASK) != 0


@pytest.fixture(scope="module")
def plain(corpus):
    ret = _retriever(False)
    _add(ret, corpus, 0, N)
    return ret


@pytest.mark.parametrize("knob", [0, KNOB], ids=["masks", "masks+lists"])
def test_mixed_filters_equal_one_call_per_filter(gpu, corpus, plain, knob):
    from audio_rag_amd import _armi

    ret = _retriever(True, knob)
    _add(ret, corpus, 0, N)
    # with the row-list knob the selective filter and the one without a match leave the scan
    listed = [f is not None and "audio_id" in f for f in QUERY_FILTERS] if knob else [False] * NQ
    for mode in MODES:
        out, m = ret.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                  search_type=mode)
        assert m == mode
        _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, mode), f"{mode} knob={knob}")
        by = {repr(g.filter): g for g in ret.last_plan}
        assert len(by) == len(FILTERS)
        for f in FILTERS:
            g = by[repr(f)]
            is_listed = bool(knob) and f is not None and "audio_id" in f
            assert g.rowlist == is_listed, (mode, f)
            assert g.qmask == (mode != "sparse" and not is_listed), (mode, f)
        flags = out.flags.cpu().numpy()
        np.testing.assert_array_equal((flags & _armi.ARMI_FLAG_ROWLIST) != 0, np.array(listed))
        if mode == "dense":
            np.testing.assert_array_equal(_qmask_flags(out), ~np.array(listed))
        else:
            assert not _qmask_flags(out).any()
    count = _arrays(ret.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                     search_type="hybrid")[0], "hybrid")["count"]
    assert (count[[i for i, f in enumerate(QUERY_FILTERS) if f == {"audio_id": 999}]] == 0).all()


def test_knob_off_plan_and_flags_as_before(gpu, corpus, plain):
    for mode in MODES:
        out, m = plain.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                    search_type=mode)
        _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, mode), mode)
        assert all(not g.qmask and not g.rowlist and g.matches == -1 for g in plain.last_plan)
        assert not _qmask_flags(out).any()


def test_old_path_where_the_form_does_not_apply(gpu, corpus, plain):
    """top_k > 64 (the fp16 scan), a single group, and a collection with tail rows: no group is
    marked, no ARMI_FLAG_QMASK, the same answers."""
    ret = _retriever(True)
    _add(ret, corpus, 0, N)
    # top_k 70 > 64 in dense mode; hybrid's leg is 2 * 40 = 80 > 64
    for mode, k in (("dense", 70), ("hybrid", 40)):
        out, m = ret.search_batch(_batch(corpus, gpu), k, filter_metadata=QUERY_FILTERS,
                                  search_type=mode)
        _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, mode, k), f"{mode} k={k}")
        assert all(not g.qmask for g in ret.last_plan) and not _qmask_flags(out).any()
    # hybrid with a leg of 2 * 32 = 64 still takes the form
    out, m = ret.search_batch(_batch(corpus, gpu), 32, filter_metadata=QUERY_FILTERS,
                              search_type="hybrid")
    _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, "hybrid", 32), "hybrid k=32")
    assert all(g.qmask for g in ret.last_plan)
    # one group: one masked search, as without a plan
    one = [{"speaker": 1}] * NQ
    out, m = ret.search_batch(_batch(corpus, gpu), K, filter_metadata=one, search_type="dense")
    _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, "dense", K, one), "one group")
    assert [g.qmask for g in ret.last_plan] == [False] and not _qmask_flags(out).any()
    # a live collection with tail rows
    live = _retriever(True, live=64)
    _add(live, corpus, 0, N - 100)
    live.collection().segments()  # first build
    _add(live, corpus, N - 100, N)
    assert live.collection().segments().tail.n_rows == 100
    for mode in ("dense", "hybrid"):
        out, m = live.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                   search_type=mode)
        _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, mode), f"live {mode}")
        assert all(not g.qmask for g in live.last_plan) and not _qmask_flags(out).any()
    live.collection().compact()   # the tail folded in: the form applies again
    out, m = live.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                               search_type="dense")
    _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, "dense"), "compacted")
    assert all(g.qmask for g in live.last_plan) and _qmask_flags(out).all()


def test_more_than_128_queries_are_cut_into_calls(gpu, corpus, plain):
    """200 queries (the 70 repeated) under 5 masked groups: two topk_masks calls."""
    sel = [i % NQ for i in range(200)]
    filters = [QUERY_FILTERS[i] for i in sel]
    ret = _retriever(True)
    _add(ret, corpus, 0, N)
    out, m = ret.search_batch(_batch(corpus, gpu, sel), K, filter_metadata=filters,
                              search_type="dense")
    ref = _reference(plain, corpus, gpu, "dense")
    _assert_same(_arrays(out, m), {n: a[sel] for n, a in ref.items()}, "200 queries")
    assert _qmask_flags(out).all()


def test_query_batcher_mixed_filter_stream(gpu, corpus, plain):
    from audio_rag_amd.core import EmbeddingResult, SparseVector
    from audio_rag_amd.retrieval.batcher import QueryBatcher

    _, _, (qi, qx, qv), qd = corpus

    def emb(q):
        return EmbeddingResult(dense=qd[q].view(np.float16).astype(np.float32).tolist(),
                               sparse=SparseVector(qx[qi[q]:qi[q + 1]].tolist(),
                                                   qv[qi[q]:qi[q + 1]].tolist()))

    ret = _retriever(True)
    _add(ret, corpus, 0, N)
    with QueryBatcher(ret, top_k=K, search_type="hybrid", max_batch=64, max_wait_ms=50.0) as qb:
        futures = [qb.submit(emb(q), QUERY_FILTERS[q]) for q in range(NQ)]
        got = [[(r.chunk.text, r.score) for r in f.result(60)] for f in futures]
        assert qb.batches < NQ / 2  # mixed filters share batches (one search_batch per batch)
    for q in range(0, NQ, 3):
        want = [(r.chunk.text, r.score) for r in plain.search(emb(q), K,
                                                              filter_metadata=QUERY_FILTERS[q],
                                                              search_type="hybrid")]
        assert got[q] == want, q
