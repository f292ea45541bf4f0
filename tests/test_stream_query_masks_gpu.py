"""StreamServer(query_masks=True) (armi_stream_create_ex with ARMI_STREAM_QUERY_MASKS): requests of
different payload filters coalesce into one native batch, which is answered by the per-query-mask
kernels through a table of the requests' mask pointers. Every ticket's answer must equal the CPU
oracle's for that query under that filter (QdrantRetriever.search's branches, qdrant.py:227-352)
and, bit for bit, what a server without the flag returns for the same submissions.

Servers take max_batch = the number of queries submitted, from one thread, and a max_wait_ms of
2000: a batch leaves because it is full, never because of timing, and waits use a 10 s timeout so
a wrong seal rule fails an assertion instead of hanging. The servers WITHOUT the flag take a
max_wait_ms of 1 instead: consecutive submissions carry different filters there, so every query
closes the batch before it and the batch count is one per query whatever the timing, but the last
batch is closed by nothing and would sit out the whole 2 s."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, NQ, K = 3109, 256, 32, 5
WAIT = 10.0

# payload metadata of row r, and the filters over it: different selectivities (1/2 .. 1/77 of the
# rows), conjunctions, and one that matches nothing
KEYS = {"a": 2, "b": 3, "c": 5, "d": 7, "e": 11}
FILTERS = ([{"a": v} for v in range(2)] + [{"b": v} for v in range(3)] +
           [{"c": v} for v in range(5)] + [{"d": v} for v in range(7)] +
           [{"e": 3}, {"e": 7}, {"a": 0, "b": 1}, {"c": 1, "d": 2}, {"d": 3, "e": 5}, {"b": 99}])
assert len(FILTERS) == 23


def _bits(ok: np.ndarray) -> np.ndarray:
    w = np.zeros((ok.size + 63) // 64, dtype=np.uint64)
    idx = np.flatnonzero(ok)
    np.bitwise_or.at(w, idx >> 6, np.left_shift(np.uint64(1), (idx & 63).astype(np.uint64)))
    return w


def _filter_bits(flt):
    if flt is None:
        return None
    ok = np.ones(N, dtype=bool)
    for key, v in flt.items():
        ok &= (np.arange(N) % KEYS[key]) == v
    return _bits(ok)


class Store:
    """Rows, sparse corpus, NQ queries, the retriever over them and the oracle's lists per filter
    (2K long, computed once per filter for all queries; a top-K list is their prefix)."""

    def __init__(self, o):
        from audio_rag_amd.config import RetrievalConfig
        from audio_rag_amd.retrieval.mi355x import MI355XRetriever

        self.o = o
        self.rows = o.unit_fp16(N, DIM, seed=71)
        self.csr = o.sparse_corpus(N, seed=72)
        self.q_csr = o.sparse_queries(NQ, seed=73)
        self.qd = o.unit_fp16(NQ, DIM, seed=74)
        ip, ix, iv = self.csr
        sparse = [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(N)]
        payloads = [{"text": f"c{r}", "start": r, "end": r + 1, "speaker": None,
                     "metadata": {key: r % m for key, m in KEYS.items()}} for r in range(N)]
        self.ret = MI355XRetriever(RetrievalConfig(top_k=K), DIM)
        self.ret.add_arrays(self.rows.view(np.float16), payloads, sparse=sparse)
        self._lists: dict = {}

    def terms(self, i):
        qi, qx, qv = self.q_csr
        return qx[qi[i]:qi[i + 1]], qv[qi[i]:qi[i + 1]]

    def lists(self, flt):
        key = None if flt is None else tuple(sorted(flt.items()))
        if key not in self._lists:
            mask = _filter_bits(flt)
            d = self.o.dense_topk(self.rows, self.qd, 2 * K, row_mask=mask)
            s = self.o.sparse_topk(*self.csr, *self.q_csr, 2 * K, row_mask=mask)
            self._lists[key] = (d, s)
        return self._lists[key]

    def want(self, i, flt, st, empty=False):
        """(ids, scores) the reference path returns for query i under flt by branch st; empty: the
        query carries an empty sparse vector."""
        d, s = self.lists(flt)
        if st == "dense":
            c = min(int(d.count[i]), K)
            return d.ids[i, :c].tolist(), [float(x) for x in d.scores[i, :c]]
        if st == "sparse":
            c = 0 if empty else min(int(s.count[i]), K)
            return s.ids[i, :c].tolist(), [float(x) for x in s.scores[i, :c]]
        sp = [] if empty else s.ids[i, :s.count[i]].tolist()
        fused = self.o.rrf([d.ids[i, :d.count[i]].tolist(), sp], K)
        return [p for p, _ in fused], [float(x) for _, x in fused]


@pytest.fixture(scope="module")
def store(gpu, oracle_mod):
    return Store(oracle_mod)


def _answers(srv, store, subs):
    """Submits every (query, filter, search_type, empty) from this thread, then collects them:
    [(ids, scores)] per submission."""
    tickets = []
    for i, flt, st, empty in subs:
        sp = None
        if st != "dense":
            sp = (np.zeros(0, np.int32), np.zeros(0, np.float32)) if empty else store.terms(i)
        tickets.append(srv.submit_arrays(store.qd[i].view(np.float16), sp, flt, st))
    out = []
    for t in tickets:
        scores, ids, c = srv.raw_result(t, timeout=WAIT)
        out.append((ids[:c].tolist(), [float(x) for x in scores[:c]]))
    return out


def _check(store, subs, got, plain):
    for j, (i, flt, st, empty) in enumerate(subs):
        assert got[j] == store.want(i, flt, st, empty), (j, i, flt, st, empty)
    assert got == plain                           # the server without the flag, bit for bit


def _both(store, subs, search_type, max_batch):
    """The submissions through a query-masks server (one full batch) and through a server without
    the flag (one batch per query: consecutive filters differ)."""
    from audio_rag_amd.retrieval.batcher import StreamServer

    assert all(subs[j][1] != subs[j + 1][1] for j in range(len(subs) - 1))
    with StreamServer(store.ret, max_batch=max_batch, max_wait_ms=2000.0,
                      search_type=search_type, query_masks=True) as srv:
        got = _answers(srv, store, subs)
        stats = srv.stats_ex()
        assert not srv._masks                     # every filter reference released with its result
    with StreamServer(store.ret, max_batch=max_batch, max_wait_ms=1.0,
                      search_type=search_type) as srv:
        plain = _answers(srv, store, subs)
        assert srv.stats() == (len(subs), len(subs))   # the behaviour the flag must not touch
        assert srv.stats_ex() == (len(subs), len(subs), 0)
    return got, plain, stats


def test_dense_server_one_mixed_batch(store):
    """16 queries under 16 different filters (two of them None, one matching nothing): one batch,
    answered through armi_dense_topk_qmask_ptrs."""
    filters = [None] + FILTERS[:7] + [None] + FILTERS[16:]
    assert len(filters) == 16 and {"b": 99} in filters
    subs = [(j, filters[j], "dense", False) for j in range(16)]
    got, plain, stats = _both(store, subs, "dense", 16)
    assert stats == (1, 16, 1)
    _check(store, subs, got, plain)
    assert got[15] == ([], [])                    # {"b": 99} matches no row


def test_hybrid_server_one_mixed_batch(store):
    """k = 5 (dense and sparse prefetch 10), 24 queries: hybrid / dense / sparse branches across
    filters, one empty sparse vector on the hybrid branch and one on the sparse branch."""
    types = ["hybrid", "dense", "sparse"]
    filters = FILTERS + [None]
    subs = [(j, filters[j], types[j % 3], j in (9, 11)) for j in range(24)]
    got, plain, stats = _both(store, subs, "hybrid", 24)
    assert stats == (1, 24, 1)
    _check(store, subs, got, plain)
    assert got[11] == ([], [])                    # sparse-only with an empty vector


def test_dense_list_cut_into_two_calls(store):
    """160 queries over 20 filters in one batch: the dense side runs as 128 + 32 queries."""
    types = ["hybrid", "dense", "sparse"]
    filters = FILTERS[:19] + [None]
    subs = [(j % NQ, filters[j % 20], types[(j // 20) % 3], False) for j in range(160)]
    got, plain, stats = _both(store, subs, "hybrid", 160)
    assert stats == (1, 160, 1)
    _check(store, subs, got, plain)


def test_uniform_batches_are_not_mixed(store):
    """16 queries under one filter, then 16 unfiltered, on a query-masks server: two batches that
    run the calls of a server without the flag; mixed_batches stays 0."""
    from audio_rag_amd.retrieval.batcher import StreamServer

    with StreamServer(store.ret, max_batch=16, max_wait_ms=2000.0, query_masks=True) as srv:
        for flt, served in ((FILTERS[3], 16), (None, 32)):
            subs = [(j, flt, "dense", False) for j in range(16)]
            got = _answers(srv, store, subs)
            for j, (i, f, st, empty) in enumerate(subs):
                assert got[j] == store.want(i, f, st), (j, flt)
            assert srv.stats_ex() == (served // 16, served, 0)


def test_refused_shapes(store):
    from audio_rag_amd.core.exceptions import RetrievalError
    from audio_rag_amd.retrieval.batcher import StreamServer

    with pytest.raises(RetrievalError, match="ARMI_STREAM_QUERY_MASKS needs"):
        StreamServer(store.ret, top_k=65, max_batch=16, query_masks=True)
    with pytest.raises(RetrievalError, match="ARMI_STREAM_QUERY_MASKS needs"):
        StreamServer(store.ret, top_k=33, max_batch=16, search_type="hybrid", query_masks=True)
    # the same top_k without the flag still works, and the largest with it
    for kw in ({"top_k": 65}, {"top_k": 33, "search_type": "hybrid"},
               {"top_k": 64, "query_masks": True},
               {"top_k": 32, "search_type": "hybrid", "query_masks": True}):
        with StreamServer(store.ret, max_batch=4, max_wait_ms=0.5, **kw) as srv:
            scores, ids, c = srv.raw_result(
                srv.submit_arrays(store.qd[0].view(np.float16), None, FILTERS[0]), timeout=WAIT)
            d = store.o.dense_topk(store.rows, store.qd[:1], kw["top_k"],
                                   row_mask=_filter_bits(FILTERS[0]))
            assert ids[:c].tolist() == d.ids[0, :d.count[0]].tolist(), kw


def test_loadgen_with_filters(store):
    """The native load generator with a filter per arrival (armi_stream_loadgen_ex): arrival i is
    query i % NQ under filter i % 7; every answer equals the oracle's."""
    from audio_rag_amd.retrieval.batcher import StreamServer

    filters = [FILTERS[0], None, FILTERS[4], FILTERS[9], FILTERS[22], FILTERS[12], FILTERS[19]]
    n = 300
    with StreamServer(store.ret, max_batch=64, max_wait_ms=1.0, query_masks=True) as srv:
        lat, elapsed, ids, cnt = srv.loadgen(store.qd.view(np.float16), n, qps=20000.0, seed=5,
                                             answers=True, filters=filters)
        batches, served, mixed = srv.stats_ex()
    assert lat.shape == (n,) and (lat > 0).all() and elapsed > 0
    assert served == n and 1 <= mixed <= batches < n
    for i in range(n):
        want_ids, _ = store.want(i % NQ, filters[i % 7], "dense")
        assert ids[i, :cnt[i]].tolist() == want_ids, i
