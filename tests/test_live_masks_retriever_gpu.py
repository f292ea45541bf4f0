"""Per-query filters over a live collection with tail rows through MI355XRetriever
(filter_query_masks_live): a batch mixing broad filters, unfiltered queries, a selective filter
and a filter without a match must get, query by query and bit for bit, what a knob-off retriever
over the same two segments returns when it is called once per distinct filter; only the plan
(last_plan) and TopK.flags (ARMI_FLAG_QMASK, ARMI_FLAG_ROWLIST) tell the paths apart."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, TAIL, DIM, NQ, K, KNOB = 4000, 100, 256, 70, 5, 256
# speaker: 4 values, 1000 rows each (broad); audio_id: 80 values, 50 rows each (selective)
FILTERS = [{"speaker": 0}, None, {"speaker": 1}, {"audio_id": 7}, {"speaker": 2, "kind": 0},
           {"audio_id": 999}, {"speaker": 3}]
QUERY_FILTERS = [FILTERS[i % len(FILTERS)] for i in range(NQ)]
MODES = ("dense", "hybrid", "sparse")


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    rows = oracle_mod.unit_fp16(N, DIM, seed=600)
    csr = oracle_mod.sparse_corpus(N, seed=601)
    sq = oracle_mod.sparse_queries(NQ, seed=602)
    qd = oracle_mod.unit_fp16(NQ, DIM, seed=603)
    return rows, csr, sq, qd


def _add(ret, corpus, lo, hi):
    rows, (ip, ix, iv), _, _ = corpus
    sparse = [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(lo, hi)]
    payloads = [{"text": f"c{r}", "start": r, "end": r + 1, "speaker": None,
                 "metadata": {"audio_id": r % 80, "speaker": r % 4, "kind": r % 3}}
                for r in range(lo, hi)]
    ret.add_arrays(rows[lo:hi].view(np.float16), payloads, sparse=sparse)


def _live_retriever(corpus, dense=False, sparse=False, live=False, knob=0):
    """A retriever over N - TAIL built rows and a tail of TAIL rows."""
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    ret = MI355XRetriever(RetrievalConfig(
        top_k=K, filter_query_masks=dense, filter_query_masks_sparse=sparse,
        filter_query_masks_live=live, filter_list_rows=knob, live_tail_rows=2 * TAIL,
        reproduce_sparse_drop=False), DIM)
    _add(ret, corpus, 0, N - TAIL)
    ret.collection().segments()  # first build
    _add(ret, corpus, N - TAIL, N)
    seg = ret.collection().segments()
    assert seg.tail.n_rows == TAIL and seg.tail_sparse.n_rows == TAIL and seg.main_rows == N - TAIL
    return ret


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


@pytest.fixture(scope="module")
def plain(corpus):
    """Every knob off: one masked search and one tail pass per filter."""
    return _live_retriever(corpus)


_refs: dict = {}


def _reference(plain, corpus, gpu, mode):
    """Query-ordered arrays of the knob-off retriever called once per distinct filter with that
    filter's queries; computed once per mode."""
    if mode not in _refs:
        ref = None
        for f in FILTERS:
            sel = [i for i, qf in enumerate(QUERY_FILTERS) if qf == f]
            out, m = plain.search_batch(_batch(corpus, gpu, sel), K, filter_metadata=f,
                                        search_type=mode)
            got = _arrays(out, m)
            if ref is None:
                ref = {n: np.empty((NQ,) + a.shape[1:], dtype=a.dtype) for n, a in got.items()}
            for n, a in got.items():
                ref[n][sel] = a
        _refs[mode] = ref
    return _refs[mode]


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


def _check(ret, corpus, plain, gpu, mode, knob, qmask_mode, msg):
    """One mixed call: the reference's answers; every group the row lists leave is `qmask` iff
    qmask_mode; ARMI_FLAG_QMASK where a kernel reports it (dense and sparse lists; RRF drops the
    legs' flags)."""
    from audio_rag_amd import _armi

    out, m = ret.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                              search_type=mode)
    assert m == mode
    _assert_same(_arrays(out, m), _reference(plain, corpus, gpu, mode), msg)
    listed = [bool(knob) and f is not None and "audio_id" in f for f in QUERY_FILTERS]
    by = {repr(g.filter): g for g in ret.last_plan}
    assert len(by) == len(FILTERS)
    for f in FILTERS:
        is_listed = bool(knob) and f is not None and "audio_id" in f
        assert by[repr(f)].rowlist == is_listed, (msg, f)
        assert by[repr(f)].qmask == (qmask_mode and not is_listed), (msg, f)
    flags = out.flags.cpu().numpy()
    np.testing.assert_array_equal((flags & _armi.ARMI_FLAG_ROWLIST) != 0, np.array(listed))
    if mode != "hybrid" and qmask_mode:
        np.testing.assert_array_equal(_qmask_flags(out), ~np.array(listed), err_msg=msg)
    else:
        assert not _qmask_flags(out).any(), msg
    return out


@pytest.mark.parametrize("knob", [0, KNOB], ids=["masks", "masks+lists"])
def test_live_mixed_filters_equal_one_call_per_filter(gpu, corpus, plain, knob):
    ret = _live_retriever(corpus, dense=True, sparse=True, live=True, knob=knob)
    for mode in MODES:
        _check(ret, corpus, plain, gpu, mode, knob, True, f"{mode} knob={knob}")
    count = _arrays(ret.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                                     search_type="hybrid")[0], "hybrid")["count"]
    assert (count[[i for i, f in enumerate(QUERY_FILTERS) if f == {"audio_id": 999}]] == 0).all()
    # the tail really holds answers: some result of the batch is a tail row
    out, _ = ret.search_batch(_batch(corpus, gpu), K, filter_metadata=QUERY_FILTERS,
                              search_type="dense")
    assert (out.ids.cpu().numpy() >= N - TAIL).any()
    # after a compaction the answers are the same (no tail: the forms of a built collection)
    ret.collection().compact()
    assert ret.collection().segments().tail is None
    for mode in MODES:
        _check(ret, corpus, plain, gpu, mode, knob, True, f"compacted {mode} knob={knob}")


def test_hybrid_without_the_sparse_knob(gpu, corpus, plain):
    """The dense leg shares one scan and one tail pass; the sparse leg stays one masked search and
    one tail pass per filter. Sparse mode on its own is not marked."""
    ret = _live_retriever(corpus, dense=True, sparse=False, live=True)
    _check(ret, corpus, plain, gpu, "hybrid", 0, True, "hybrid, dense knob only")
    _check(ret, corpus, plain, gpu, "dense", 0, True, "dense, dense knob only")
    _check(ret, corpus, plain, gpu, "sparse", 0, False, "sparse, dense knob only")


def test_sparse_knob_alone(gpu, corpus, plain):
    ret = _live_retriever(corpus, dense=False, sparse=True, live=True)
    _check(ret, corpus, plain, gpu, "sparse", 0, True, "sparse, sparse knob only")
    _check(ret, corpus, plain, gpu, "hybrid", 0, False, "hybrid, sparse knob only")
    _check(ret, corpus, plain, gpu, "dense", 0, False, "dense, sparse knob only")


def test_live_knob_off_keeps_the_plan_of_before(gpu, corpus, plain):
    ret = _live_retriever(corpus, dense=True, sparse=True, live=False)
    for mode in MODES:
        _check(ret, corpus, plain, gpu, mode, 0, False, f"live knob off, {mode}")
    # and the live knob alone changes nothing
    alone = _live_retriever(corpus, live=True)
    for mode in MODES:
        _check(alone, corpus, plain, gpu, mode, 0, False, f"live knob alone, {mode}")
