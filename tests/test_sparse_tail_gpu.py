"""The fused sparse tail pass on the GPU (armi_sparse_tail_topk through TailSparseIndex.tail_topk):
the global sparse top-k over a main SparseIndex and an append-only forward-CSR tail, against the
CPU oracle over the concatenated CSR and against the general path (ARMI_TAIL_PASS=general: a native
index over the tail + the exact list merge).

Parity bar, as in test_live_tail_gpu.py: ids, counts and float32 scores bit-identical to the oracle,
fused == general field by field. The main index holds 4,096 oracle.sparse_corpus rows.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAIN, VOCAB = 4096, 250002
NEG_INF = np.float32(-np.inf)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _np(out):
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "count", "flags")}


def _assert_same(got, ref, nq=None):
    nq = ref.count.shape[0] if nq is None else nq
    np.testing.assert_array_equal(got["count"], ref.count[:nq])
    for b in range(nq):
        c = ref.count[b]
        np.testing.assert_array_equal(got["ids"][b, :c], ref.ids[b, :c], err_msg=f"query {b}")
        np.testing.assert_array_equal(got["scores"][b, :c], ref.scores[b, :c], err_msg=f"query {b}")
        assert (got["ids"][b, c:] == -1).all() and (got["scores"][b, c:] == NEG_INF).all()


def _bits(ok: np.ndarray) -> np.ndarray:
    words = np.zeros(max((len(ok) + 63) // 64, 1), dtype=np.uint64)
    for r in np.nonzero(ok)[0]:
        words[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return words


def _rows(csr, lo, hi):
    """Rows [lo, hi) of a host CSR as a CSR of their own (indptr from 0)."""
    ip, ix, iv = csr
    return ip[lo:hi + 1] - ip[lo], ix[ip[lo]:ip[hi]], iv[ip[lo]:ip[hi]]


def _from_lists(rows):
    """Host CSR of [(indices, values), ...]."""
    ip = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r[0]) for r in rows], out=ip[1:])
    ix = np.concatenate([np.asarray(r[0], dtype=np.int32) for r in rows] or [np.zeros(0, np.int32)])
    iv = np.concatenate([np.asarray(r[1], dtype=np.float32) for r in rows] or [np.zeros(0, np.float32)])
    return ip, ix.astype(np.int32), iv.astype(np.float32)


def _to_lists(csr):
    ip, ix, iv = csr
    return [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(len(ip) - 1)]


def _cat(*csrs):
    return _from_lists([r for c in csrs for r in _to_lists(c)])


def _queries(lists, gpu):
    """(host query CSR, device query CSR) of [(indices, values), ...]; one unused entry keeps the
    term arrays' device pointers non-null when every query is empty."""
    qi = np.zeros(len(lists) + 1, dtype=np.int32)
    np.cumsum([len(q[0]) for q in lists], out=qi[1:])
    qx = np.concatenate([np.asarray(q[0], dtype=np.int32) for q in lists] + [np.zeros(1, np.int32)])
    qv = np.concatenate([np.asarray(q[1], dtype=np.float32) for q in lists] + [np.zeros(1, np.float32)])
    host = (qi, qx[:qi[-1]], qv[:qi[-1]])
    return host, (_dev(qi, gpu), _dev(qx.astype(np.int32), gpu), _dev(qv.astype(np.float32), gpu))


def _first(qs, n, gpu):
    qi, qx, qv = qs
    host = (qi[:n + 1], qx[:qi[n]], qv[:qi[n]])
    return host, tuple(_dev(a, gpu) for a in host)


def _tail(csr, gpu, base=MAIN, pieces=(1, 31)):
    """A TailSparseIndex holding the host CSR, appended in pieces (then the rest, then nothing)."""
    from audio_rag_amd.retrieval.device import TailSparseIndex

    n = len(csr[0]) - 1
    t = TailSparseIndex(base, gpu, vocab=VOCAB)
    at = 0
    for size in (*pieces, n, 0):
        hi = min(at + size, n)
        t.append(*(_dev(a, gpu) for a in _rows(csr, at, hi)))
        at = hi
    assert t.n_rows == n and not t.general_built
    return t


def _both_paths(monkeypatch, tail, q, k, main, mask=None):
    monkeypatch.delenv("ARMI_TAIL_PASS", raising=False)
    built = tail.general_built
    fused = _np(tail.tail_topk(*q, k, main, row_mask=mask))
    assert tail.general_built == built  # the fused pass builds no native index over the tail
    monkeypatch.setenv("ARMI_TAIL_PASS", "general")
    general = _np(tail.tail_topk(*q, k, main, row_mask=mask))
    monkeypatch.delenv("ARMI_TAIL_PASS")
    assert tail.general_built
    np.testing.assert_array_equal(fused["count"], general["count"])
    np.testing.assert_array_equal(fused["flags"], general["flags"])
    for b, c in enumerate(fused["count"]):
        for f in ("ids", "scores"):
            np.testing.assert_array_equal(fused[f][b, :c], general[f][b, :c], err_msg=f"{f} {b}")
    np.testing.assert_array_equal(fused["flags"], _np(main)["flags"])
    return fused


@pytest.fixture(scope="module")
def seg(gpu, oracle_mod):
    """(corpus CSR of main + the largest tail, 70 queries, the main SparseIndex)."""
    from audio_rag_amd.retrieval.device import SparseIndex

    csr = oracle_mod.sparse_corpus(MAIN + 1000, seed=301)
    qs = oracle_mod.sparse_queries(70, seed=302)
    main = SparseIndex(*(_dev(a, gpu) for a in _rows(csr, 0, MAIN)), VOCAB)
    return csr, qs, main


_refs = {}


def _ref(oracle_mod, seg, tail_n, k):
    if (tail_n, k) not in _refs:
        csr, qs, _ = seg
        _refs[(tail_n, k)] = oracle_mod.sparse_topk(*_rows(csr, 0, MAIN + tail_n), *qs, k)
    return _refs[(tail_n, k)]


def _strong_row(qs, b):
    """A row holding exactly query b's terms with value 1.0: it outscores every corpus row (values
    <= 0.40) for that query."""
    qi, qx, _ = qs
    ix = qx[qi[b]:qi[b + 1]]
    return ix.copy(), np.ones(len(ix), dtype=np.float32)


# ----------------------------------------------------------------------------- 1. concatenation

@pytest.mark.parametrize("tail_n,nq,k", [(t, b, k) for t in (1, 33, 1000) for b in (1, 64, 70)
                                         for k in (5, 40, 240)])
def test_tail_pass_matches_oracle_over_the_concatenation(gpu, oracle_mod, seg, monkeypatch,
                                                         tail_n, nq, k):
    csr, qs, main_idx = seg
    _, q = _first(qs, nq, gpu)
    tail = _tail(_rows(csr, MAIN, MAIN + tail_n), gpu)
    got = _both_paths(monkeypatch, tail, q, k, main_idx.topk(*q, k))
    _assert_same(got, _ref(oracle_mod, seg, tail_n, k), nq)


# ------------------------------------------------------------------------------------ 2. masks

def test_tail_pass_with_row_masks_on_both_segments(gpu, oracle_mod, seg, monkeypatch):
    csr, qs, main_idx = seg
    rng = np.random.default_rng(5)
    _, q = _first(qs, 70, gpu)
    for tail_n in (33, 1000):  # both leave a partial last mask word (33 and 1000 % 64 = 40 bits)
        ok = rng.random(MAIN + tail_n) < 0.5
        m_main, m_tail = (_dev(_bits(x).view(np.int64), gpu) for x in (ok[:MAIN], ok[MAIN:]))
        tail = _tail(_rows(csr, MAIN, MAIN + tail_n), gpu)
        for k in (5, 240):
            got = _both_paths(monkeypatch, tail, q, k, main_idx.topk(*q, k, row_mask=m_main), m_tail)
            _assert_same(got, oracle_mod.sparse_topk(*_rows(csr, 0, MAIN + tail_n), *qs, k,
                                                     row_mask=_bits(ok)))


# ------------------------------------------------------------------- 3. main list shorter than k

@pytest.mark.parametrize("main_left", [3, 0])
def test_main_list_shorter_than_k(gpu, oracle_mod, seg, monkeypatch, main_left):
    """A main mask leaving three rows (that share a term with query 0) or none: the main list has no
    k-th score, so every tail result survives. One tail row is masked."""
    csr, qs, main_idx = seg
    ip, ix, _ = csr
    q0 = set(qs[1][qs[0][0]:qs[0][1]].tolist())
    sharing = [r for r in range(MAIN) if q0 & set(ix[ip[r]:ip[r + 1]].tolist())]
    ok = np.zeros(MAIN + 33, dtype=bool)
    ok[sharing[:main_left]] = True
    ok[MAIN:] = True
    ok[MAIN + 4] = False
    m_main, m_tail = (_dev(_bits(x).view(np.int64), gpu) for x in (ok[:MAIN], ok[MAIN:]))
    host, q = _first(qs, 8, gpu)
    tail = _tail(_rows(csr, MAIN, MAIN + 33), gpu)
    for k in (5, 40):
        main = main_idx.topk(*q, k, row_mask=m_main)
        got = _both_paths(monkeypatch, tail, q, k, main, m_tail)
        ref = oracle_mod.sparse_topk(*_rows(csr, 0, MAIN + 33), *host, k, row_mask=_bits(ok))
        _assert_same(got, ref)
        assert got["count"][0] >= min(k, main_left)
        assert not (got["ids"] == MAIN + 4).any()


def test_empty_query_and_terms_of_one_segment_only(gpu, oracle_mod, seg, monkeypatch):
    """An empty query (count 0), a query whose only term occurs in no tail row (answer == the main
    list) and one whose only term occurs in no main row (answer from the tail alone, count < k)."""
    csr, qs, main_idx = seg
    ip, ix, _ = csr
    tail_n = 33
    in_main = np.unique(ix[:ip[MAIN]])
    t_terms, t_rows = np.unique(ix[ip[MAIN]:ip[MAIN + tail_n]], return_counts=True)
    main_only = int(np.setdiff1d(in_main, t_terms)[0])
    tail_only = int(np.setdiff1d(t_terms, in_main)[0])
    n_tail_only = int(t_rows[t_terms == tail_only][0])
    host, q = _queries([_to_lists((qs[0].astype(np.int64), qs[1], qs[2]))[0], ([], []),
                        ([main_only], [0.3]), ([tail_only], [0.3])], gpu)
    tail = _tail(_rows(csr, MAIN, MAIN + tail_n), gpu)
    for k in (5, 40):
        main = main_idx.topk(*q, k)
        got = _both_paths(monkeypatch, tail, q, k, main)
        _assert_same(got, oracle_mod.sparse_topk(*_rows(csr, 0, MAIN + tail_n), *host, k))
        m = _np(main)
        assert got["count"][1] == 0
        assert m["count"][2] > 0
        np.testing.assert_array_equal(got["ids"][2], m["ids"][2])
        np.testing.assert_array_equal(got["scores"][2], m["scores"][2])
        assert m["count"][3] == 0 and got["count"][3] == n_tail_only < k
        assert (got["ids"][3, :n_tail_only] >= MAIN).all()


# ---------------------------------------------------------------------- 4. ties, ordinal order

def test_same_row_in_main_and_tail_main_first(gpu, oracle_mod, seg, monkeypatch):
    from audio_rag_amd.retrieval.device import SparseIndex

    csr, qs, _ = seg
    rows = _to_lists(_rows(csr, 0, MAIN + 33))
    rows[7] = rows[MAIN] = rows[MAIN + 20] = _strong_row(qs, 0)
    whole = _from_lists(rows)
    main_idx = SparseIndex(*(_dev(a, gpu) for a in _rows(whole, 0, MAIN)), VOCAB)
    host, q = _first(qs, 3, gpu)
    tail = _tail(_rows(whole, MAIN, MAIN + 33), gpu)
    got = _both_paths(monkeypatch, tail, q, 5, main_idx.topk(*q, 5))
    _assert_same(got, oracle_mod.sparse_topk(*whole, *host, 5))
    assert got["ids"][0, :3].tolist() == [7, MAIN, MAIN + 20]
    assert got["scores"][0, 0] == got["scores"][0, 1] == got["scores"][0, 2]


def test_more_ties_than_a_chunk_list_keeps(gpu, oracle_mod, seg, monkeypatch):
    """240 + 64 copies of one row that outscores every main row: all tie, every scan workgroup holds
    more of them than it may keep, and they come out by ascending ordinal."""
    csr, qs, main_idx = seg
    n = 240 + 64
    trows = _from_lists([_strong_row(qs, 0)] * n)
    host, q = _first(qs, 2, gpu)
    tail = _tail(trows, gpu)
    for k in (5, 240):
        got = _both_paths(monkeypatch, tail, q, k, main_idx.topk(*q, k))
        _assert_same(got, oracle_mod.sparse_topk(*_cat(_rows(csr, 0, MAIN), trows), *host, k))
        np.testing.assert_array_equal(got["ids"][0], MAIN + np.arange(k))


# -------------------------------------------------------------------------- 5. summation order

T3 = (1000, 100000, 200000)  # query 0's terms; query 1's only term:
T_LAST = 240000


def _order_row(positions, length):
    """`length` postings, ascending ids, query 0's three terms at `positions` with values
    (1e8, 1, -1e8): 0.0 when added in ascending term order, 1.0 in any order that cancels first."""
    ids, vals, nxt = [], [], 4
    for p in range(length):
        if p in positions:
            t = T3[positions.index(p)]
            ids.append(t)
            vals.append((1e8, 1.0, -1e8)[positions.index(p)])
            nxt = t + 1
        else:
            ids.append(nxt)
            vals.append(0.25)
            nxt += 1
    assert ids == sorted(set(ids)) and T_LAST not in ids
    return ids, vals


def _last_only_row(length):
    return list(range(4, 4 + length - 1)) + [T_LAST], [0.25] * (length - 1) + [0.5]


def test_summation_order_within_and_across_rounds(gpu, oracle_mod, seg, monkeypatch):
    """fp32 sums whose bits depend on the order: the three shared terms inside one 64-posting round,
    across the 64, 128 and 256 boundaries of a row (up to three rounds of the scan), and rows of
    exactly 64, 65 and 256 postings whose last posting is the only shared term."""
    csr, _, main_idx = seg
    shapes = [((0, 1, 2), 3), ((60, 61, 62), 63), ((62, 63, 64), 65), ((63, 64, 128), 129),
              ((10, 100, 199), 200), ((127, 128, 129), 200), ((0, 64, 191), 192),
              # three 128-posting rounds: the prefetched round and both reloaded ones hold a term
              ((0, 130, 299), 300), ((127, 255, 256), 257)]
    assert all(3 <= n <= 300 for _, n in shapes)
    trows = _from_lists([_order_row(p, n) for p, n in shapes] +
                        [_last_only_row(n) for n in (64, 65, 256)])
    host, q = _queries([(T3, (1.0, 1.0, 1.0)), ([T_LAST], [1.0])], gpu)
    none = _dev(_bits(np.zeros(MAIN, dtype=bool)).view(np.int64), gpu)
    ok = np.concatenate([np.zeros(MAIN, dtype=bool), np.ones(len(shapes) + 3, dtype=bool)])
    tail = _tail(trows, gpu)
    got = _both_paths(monkeypatch, tail, q, 40, main_idx.topk(*q, 40, row_mask=none))
    ref = oracle_mod.sparse_topk(*_cat(_rows(csr, 0, MAIN), trows), *host, 40, row_mask=_bits(ok))
    _assert_same(got, ref)
    n = len(shapes)
    assert ref.count.tolist() == [n, 3]
    np.testing.assert_array_equal(got["ids"][0, :n], MAIN + np.arange(n))
    assert (got["scores"][0, :n] == 0.0).all() and not np.signbit(got["scores"][0, :n]).any()
    np.testing.assert_array_equal(got["ids"][1, :3], MAIN + n + np.arange(3))
    assert (got["scores"][1, :3] == 0.5).all()


# ---------------------------------------------------------------------- 6. sign and zero cases

def test_zero_and_negative_scores_are_results(gpu, oracle_mod, seg, monkeypatch):
    csr, _, main_idx = seg
    trows = _from_lists([
        ([5000, 6000], [1.0, 1.0]),    # 0.5 - 0.5: cancels to 0.0
        ([7000], [-0.0]),              # the only shared product is -0.0
        ([6000], [2.0]),               # -1.0
        ([5000], [-3.0]),              # -1.5
        ([], []),                      # no postings
        ([8000], [1.0]),               # no shared term: not a result
        ([5000], [1.0]),               # 0.5
        ([], []),
    ])
    host, q = _queries([([5000, 6000, 7000], [0.5, -0.5, 0.25])], gpu)
    whole = _cat(_rows(csr, 0, MAIN), trows)
    tail = _tail(trows, gpu, pieces=(5,))
    none = np.zeros(MAIN, dtype=bool)
    for main_ok, k in ((none, 40), (None, 240)):
        ok = None if main_ok is None else np.concatenate([main_ok, np.ones(8, dtype=bool)])
        m_main = None if main_ok is None else _dev(_bits(main_ok).view(np.int64), gpu)
        ref = oracle_mod.sparse_topk(*whole, *host, k, row_mask=None if ok is None else _bits(ok))
        # not vacuous: the expected answer holds zero- and negative-score tail rows
        c = ref.count[0]
        in_tail = ref.ids[0, :c] >= MAIN
        assert (in_tail & (ref.scores[0, :c] == 0.0)).sum() >= 2
        assert (in_tail & (ref.scores[0, :c] < 0.0)).sum() >= 2
        got = _both_paths(monkeypatch, tail, q, k, main_idx.topk(*q, k, row_mask=m_main))
        _assert_same(got, ref)
        if main_ok is not None:
            assert got["ids"][0, :5].tolist() == [MAIN + 6, MAIN, MAIN + 1, MAIN + 2, MAIN + 3]
            assert got["count"][0] == 5


# ------------------------------------------------------------------------- 7. chunk boundaries

def test_tail_of_more_than_two_scan_chunks(gpu, oracle_mod, seg, monkeypatch):
    """A tail of 2c + 70 rows (c = the rows one scan workgroup covers): the chunk lists go through the
    finish kernel; copies of two queries' best rows sit on both sides of every chunk boundary."""
    from audio_rag_amd import synthetic
    from audio_rag_amd.retrieval.device import TailSparseIndex

    csr, qs, main_idx = seg
    c = TailSparseIndex.chunk_rows()
    assert c > 0
    n = 2 * c + 70
    rows = _to_lists(tuple(t.cpu().numpy() for t in synthetic.make_sparse_rows(0, n, gpu, seed=9)))
    at0, at1 = [c - 1, c, 2 * c - 1, 2 * c + 69], [0, c + 1, 2 * c]
    for r in at0:
        rows[r] = _strong_row(qs, 0)
    for r in at1:
        rows[r] = _strong_row(qs, 1)
    trows = _from_lists(rows)
    host, q = _first(qs, 5, gpu)
    tail = _tail(trows, gpu, pieces=(c - 1, 2))
    whole = _cat(_rows(csr, 0, MAIN), trows)
    for k in (5, 40):
        got = _both_paths(monkeypatch, tail, q, k, main_idx.topk(*q, k))
        _assert_same(got, oracle_mod.sparse_topk(*whole, *host, k))
        assert got["ids"][0, :4].tolist() == [MAIN + r for r in at0]
        assert got["ids"][1, :3].tolist() == [MAIN + r for r in at1]


# ------------------------------------------------------------------------------- 8. long query

def test_query_of_300_terms_is_scored_on_its_first_256(gpu, oracle_mod, seg, monkeypatch):
    csr, qs, main_idx = seg
    ip, ix, _ = csr
    terms, freq = np.unique(ix[:ip[MAIN + 1000]], return_counts=True)
    long_terms = np.sort(terms[np.argsort(-freq, kind="stable")[:300]])
    w = np.random.default_rng(8).uniform(0.05, 0.35, size=300).astype(np.float32)
    host, q = _queries([(long_terms, w), _to_lists((qs[0].astype(np.int64), qs[1], qs[2]))[1]], gpu)
    cut, _ = _queries([(long_terms[:256], w[:256]),
                       _to_lists((qs[0].astype(np.int64), qs[1], qs[2]))[1]], gpu)
    tail = _tail(_rows(csr, MAIN, MAIN + 1000), gpu)
    got = _both_paths(monkeypatch, tail, q, 40, main_idx.topk(*q, 40))
    ref = oracle_mod.sparse_topk(*csr, *cut, 40)
    _assert_same(got, ref)
    assert (ref.ids[0, :40] >= MAIN).any()  # the tail contributes to the long query's answer


# ---------------------------------------------------------------------------- 9. graph capture

def test_main_and_tail_pass_replay_from_one_graph(gpu, oracle_mod, seg):
    csr, qs, main_idx = seg
    nq, k, cap = 8, 40, 8 * 32
    tail = _tail(_rows(csr, MAIN, MAIN + 1000), gpu)
    qi = torch.zeros(nq + 1, dtype=torch.int32, device=gpu)
    qx = torch.zeros(cap, dtype=torch.int32, device=gpu)
    qv = torch.zeros(cap, dtype=torch.float32, device=gpu)

    def fill(host):
        qi.copy_(_dev(host[0], gpu))
        qx[:len(host[1])].copy_(_dev(host[1], gpu))
        qv[:len(host[2])].copy_(_dev(host[2], gpu))

    def run():
        return tail.tail_topk(qi, qx, qv, k, main_idx.topk(qi, qx, qv, k))

    batches = [_first(qs, nq, gpu)[0],
               _first(oracle_mod.sparse_queries(nq, seed=303), nq, gpu)[0]]
    fill(batches[0])
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for host in (batches[1], batches[0]):
        fill(host)
        graph.replay()
        replayed = _np(out)
        eager = _np(run())
        for f in ("ids", "scores", "count", "flags"):
            np.testing.assert_array_equal(replayed[f], eager[f], err_msg=f)
        _assert_same(replayed, oracle_mod.sparse_topk(*csr, *host, k))
    assert not tail.general_built


# ------------------------------------------------------------------ 10. argument validation

def test_arguments_are_validated_before_any_device_work(gpu, seg):
    from audio_rag_amd import _armi
    from audio_rag_amd._armi import ptr
    from audio_rag_amd.retrieval.device import TailSparseIndex

    _, qs, main_idx = seg
    _, q = _first(qs, 2, gpu)
    k = 5
    main = main_idx.topk(*q, k)
    o_s = torch.full((2, k), 7.0, dtype=torch.float32, device=gpu)
    o_i = torch.full((2, k), 7, dtype=torch.int64, device=gpu)
    o_c = torch.full((2,), 7, dtype=torch.int32, device=gpu)
    o_f = torch.full((2,), 7, dtype=torch.int32, device=gpu)
    ip = torch.zeros(1000, dtype=torch.int64, device=gpu)
    c = TailSparseIndex.chunk_rows()

    def call(tail_rows=0, kk=k, outs=(o_s, o_i, o_c), ws=None, ws_bytes=0):
        return _armi.call("armi_sparse_tail_topk", ptr(ip), None, None, tail_rows, MAIN, ptr(q[0]),
                          ptr(q[1]), ptr(q[2]), 2, kk, None, ptr(main.scores), ptr(main.ids),
                          ptr(main.count), ptr(main.flags), ptr(outs[0]), ptr(outs[1]),
                          ptr(outs[2]), ptr(o_f), ws, ws_bytes, _armi.stream_handle())

    for bad in (dict(kk=0), dict(kk=241), dict(tail_rows=-1), dict(outs=(None, o_i, o_c)),
                dict(outs=(o_s, None, o_c)), dict(outs=(o_s, o_i, None)),
                dict(tail_rows=2 * c + 1, ws=None, ws_bytes=0),
                dict(outs=(main.scores, o_i, o_c))):
        with pytest.raises(_armi.ArmiError, match="armi_sparse_tail_topk"):
            call(**bad)
    torch.cuda.synchronize()
    assert (o_c == 7).all() and (o_i == 7).all()  # nothing ran
    # a tail of one chunk needs no workspace: null pointer, size 0 (rows without postings here)
    assert _armi.query("armi_sparse_tail_workspace_bytes", c, 2, k) == 0
    call(tail_rows=c)
    torch.cuda.synchronize()
    assert torch.equal(o_s, main.scores) and torch.equal(o_i, main.ids)
    assert torch.equal(o_c, main.count) and torch.equal(o_f, main.flags)
    o_c.fill_(7)
    # an empty tail copies the main list through
    call(tail_rows=0)
    torch.cuda.synchronize()
    assert torch.equal(o_s, main.scores) and torch.equal(o_i, main.ids)
    assert torch.equal(o_c, main.count) and torch.equal(o_f, main.flags)


def test_tail_topk_refuses_a_main_list_of_another_shape_type_or_device(gpu, seg):
    from audio_rag_amd.retrieval.device import TopK

    csr, qs, main_idx = seg
    _, q = _first(qs, 2, gpu)
    tail = _tail(_rows(csr, MAIN, MAIN + 33), gpu)
    main = main_idx.topk(*q, 5)

    def variant(**kw):
        f = dict(scores=main.scores, ids=main.ids, count=main.count, flags=main.flags)
        f.update(kw)
        return TopK(**f)

    bad = [main_idx.topk(*q, 6),                                   # another k
           variant(scores=main.scores[:, :4]), variant(scores=main.scores.double()),
           variant(count=main.count.long()), variant(count=main.count[:1]),
           variant(flags=main.flags.long()), variant(ids=main.ids.cpu()),
           variant(scores=main.scores.cpu())]
    for m in bad:
        with pytest.raises(ValueError, match="main must be"):
            tail.tail_topk(*q, 5, m)
    words = torch.full((4,), -1, dtype=torch.int64, device=gpu)
    for mask in (words[::2], words.to(torch.int32), words.cpu(), words[:0]):
        with pytest.raises(ValueError, match="row_mask"):
            tail.tail_topk(*q, 5, main, row_mask=mask)
    with pytest.raises(ValueError, match="k must be"):
        tail.tail_topk(*q, 241, main)
    got = _np(tail.tail_topk(*q, 5, variant(flags=None), row_mask=words))
    assert (got["flags"] == 0).all() and (got["count"] == 5).all()
    assert not tail.general_built
