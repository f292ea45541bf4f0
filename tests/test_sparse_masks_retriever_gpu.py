"""Broad per-query filters through MI355XRetriever's sparse kernels (filter_query_masks_sparse):
in sparse mode, and for hybrid's sparse leg with filter_query_masks on as well, a batch mixing
broad filters, unfiltered queries, a selective filter and a filter without a match must get, query
by query and bit for bit, what a knob-off retriever returns when it is called once per filter;
only the plan (last_plan) and, in sparse mode, TopK.flags (ARMI_FLAG_QMASK) tell the paths apart.
The corpus and the filters are those of test_filter_masks_retriever_gpu.py."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, DIM, NQ, K, KNOB = 4000, 256, 70, 5, 256
# speaker: 4 values, 1000 rows each (broad); audio_id: 80 values, 50 rows each (selective)
FILTERS = [{"speaker": 0}, None, {"speaker": 1}, {"audio_id": 7}, {"speaker": 2, "kind": 0},
           {"audio_id": 999}, {"speaker": 3}]
QUERY_FILTERS = [FILTERS[i % len(FILTERS)] for i in range(NQ)]


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    rows = oracle_mod.unit_fp16(N, DIM, seed=500)
    csr = oracle_mod.sparse_corpus(N, seed=501)
    sq = oracle_mod.sparse_queries(NQ, seed=502)
    qd = oracle_mod.unit_fp16(NQ, DIM, seed=503)
    return rows, csr, sq, qd


def _retriever(dense_masks: bool, sparse_masks: bool, knob: int = 0, live: int = 0):
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    return MI355XRetriever(RetrievalConfig(top_k=K, filter_query_masks=dense_masks,
                                           filter_query_masks_sparse=sparse_masks,
                                           filter_list_rows=knob, live_tail_rows=live,
                                           reproduce_sparse_drop=False), DIM)


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
    return {"ids": out.ids.cpu().numpy(), "scores": sc.cpu().numpy(),
            "count": out.count.cpu().numpy()}


_refs: dict = {}


def _reference(plain, corpus, gpu, mode, k=K):
    """Query-ordered arrays of the knob-off retriever called once per distinct filter with that
    filter's queries. Computed once per (mode, k) and shared."""
    if (mode, k) not in _refs:
        ref = None
        for f in FILTERS:
            sel = [i for i, qf in enumerate(QUERY_FILTERS) if qf == f]
            out, m = plain.search_batch(_batch(corpus, gpu, sel), k, filter_metadata=f,
                                        search_type=mode)
            got = _arrays(out, m)
            if ref is None:
                ref = {n: np.empty((NQ,) + a.shape[1:], dtype=a.dtype) for n, a in got.items()}
            for n, a in got.items():
                ref[n][sel] = a
        _refs[(mode, k)] = ref
    return _refs[(mode, k)]


def _assert_same(got, ref, msg):
    np.testing.assert_array_equal(got["count"], ref["count"], err_msg=msg)
    np.testing.assert_array_equal(got["ids"], ref["ids"], err_msg=msg)
    for b, c in enumerate(ref["count"]):
        np.testing.assert_array_equal(got["scores"][b, :c], ref["scores"][b, :c],
                                      err_msg=f"{msg} q{b}")


def _qmask_flags(out):
    from audio_rag_amd import _armi

    return (out.flags.cpu().numpy() & _armi.ARMI_FLAG_QMASK) != 0


@pytest.fixture(scope="module")
def plain(corpus):
    ret = _retriever(False, False)
    _add(ret, corpus, 0, N)
    return ret


@pytest.mark.parametrize("knob", [0, KNOB], ids=["masks", "masks+lists"])
def test_mixed_filters_equal_one_call_per_filter(gpu, corpus, plain, knob, monkeypatch):
    from audio_rag_amd import _armi
    from audio_rag_amd.retrieval.device import SparseIndex

    ret = _retriever(True, True, knob)
    _add(ret, corpus, 0, N)
    calls = {"masks": 0, "topk": 0}
    real_masks, real_topk = SparseIndex.topk_masks, SparseIndex.topk
    monkeypatch.setattr(SparseIndex, "topk_masks", lambda self, *a, **kw: (
        calls.__setitem__("masks", calls["masks"] + 1), real_masks(self, *a, **kw))[1])
    monkeypatch.setattr(SparseIndex, "topk", lambda self, *a, **kw: (
        calls.__setitem__("topk", calls["topk"] + 1), real_topk(self, *a, **kw))[1])
    listed = [f is not None and "audio_id" in f for f in QUERY_FILTERS] if knob else [False] * NQ
    for mode in ("sparse", "hybrid"):
        ref = _reference(plain, corpus, gpu, mode)   # (the plain retriever's own topk calls)
        calls.update(masks=0, topk=0)
        out, m = ret.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                  search_type=mode)
        assert m == mode
        # one sparse search for all the masked groups, none per filter
        assert calls == {"masks": 1, "topk": 0}, (mode, calls)
        _assert_same(_arrays(out, m), ref, f"{mode} knob={knob}")
        by = {repr(g.filter): g for g in ret.last_plan}
        assert len(by) == len(FILTERS)
        for f in FILTERS:
            g = by[repr(f)]
            is_listed = bool(knob) and f is not None and "audio_id" in f
            assert g.rowlist == is_listed, (mode, f)
            assert g.qmask == (not is_listed), (mode, f)
        flags = out.flags.cpu().numpy()
        np.testing.assert_array_equal((flags & _armi.ARMI_FLAG_ROWLIST) != 0, np.array(listed))
        if mode == "sparse":
            np.testing.assert_array_equal(_qmask_flags(out), ~np.array(listed))
    count = _arrays(ret.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                     search_type="sparse")[0], "sparse")["count"]
    assert (count[[i for i, f in enumerate(QUERY_FILTERS) if f == {"audio_id": 999}]] == 0).all()


def test_200_queries_are_cut_into_two_calls(gpu, corpus, plain, monkeypatch):
    from audio_rag_amd.retrieval.device import SparseIndex

    sel = [i % NQ for i in range(200)]
    filters = [QUERY_FILTERS[i] for i in sel]
    ret = _retriever(True, True)
    _add(ret, corpus, 0, N)
    sizes = []
    real = SparseIndex.topk_masks
    monkeypatch.setattr(SparseIndex, "topk_masks", lambda self, qi, *a, **kw: (
        sizes.append(int(qi.numel()) - 1), real(self, qi, *a, **kw))[1])
    for mode in ("sparse", "hybrid"):
        del sizes[:]
        out, m = ret.search_batch(_batch(corpus, gpu, sel), K, filter_metadata=filters,
                                  search_type=mode)
        ref = _reference(plain, corpus, gpu, mode)
        _assert_same(_arrays(out, m), {n: a[sel] for n, a in ref.items()}, f"200 queries {mode}")
        assert sizes == [128, 72], (mode, sizes)
        if mode == "sparse":
            assert _qmask_flags(out).all()


def test_tail_rows_and_the_dense_knob_alone_take_the_old_path(gpu, corpus, plain):
    # a live collection with tail rows: armi_sparse_tail_topk takes one mask
    live = _retriever(True, True, live=64)
    _add(live, corpus, 0, N - 100)
    live.collection().segments()  # first build
    _add(live, corpus, N - 100, N)
    assert live.collection().segments().tail.n_rows == 100
    for mode in ("sparse", "hybrid"):
        out, m = live.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                   search_type=mode)
        _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, mode), f"live {mode}")
        assert all(not g.qmask for g in live.last_plan) and not _qmask_flags(out).any()
    # filter_query_masks alone: sparse mode unmarked, as before the sparse knob existed
    dense_only = _retriever(True, False)
    _add(dense_only, corpus, 0, N)
    out, m = dense_only.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                     search_type="sparse")
    _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, "sparse"), "dense knob only")
    assert all(not g.qmask for g in dense_only.last_plan) and not _qmask_flags(out).any()
    # the sparse knob alone: sparse mode takes the form, hybrid (no shared dense scan) does not
    sparse_only = _retriever(False, True)
    _add(sparse_only, corpus, 0, N)
    out, m = sparse_only.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                      search_type="sparse")
    _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, "sparse"), "sparse knob only")
    assert all(g.qmask for g in sparse_only.last_plan) and _qmask_flags(out).all()
    out, m = sparse_only.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                      search_type="hybrid")
    _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, "hybrid"), "sparse knob, hybrid")
    assert all(not g.qmask for g in sparse_only.last_plan)
