"""armi_sparse_topk_qmask (SparseIndex.topk_masks): a sparse top-k in which every query carries its
own row mask, in the launches of one armi_sparse_topk call. The answer of query q must be bit for
bit armi_sparse_topk's with row_mask = that query's mask (ids, fp32 scores, count, padding), on
the MFMA filter path and on the exact scan, in every pass of 64 queries. The reference is the CPU
oracle (oracle/armi_oracle.c) run once per mask, and where stated one SparseIndex.topk(row_mask=)
per mask on the same index.
Reference: src/audio_rag/api/v1/query.py:41 and src/audio_rag/retrieval/qdrant.py:263-269 (one
payload filter per request, for every search type)."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sparse_adversarial as adv  # noqa: E402

pytestmark = pytest.mark.gpu

CERTIFIED, FALLBACK, FILTERED, QMASK = 1, 2, 4, 16
VOCAB = 250002


def _t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _index(csr, gpu, base=0):
    from audio_rag_amd.retrieval.device import SparseIndex

    return SparseIndex(*(_t(a, gpu) for a in csr), VOCAB, base)


def _bits(ok: np.ndarray, words: int | None = None) -> np.ndarray:
    out = np.zeros(words or (len(ok) + 63) // 64, dtype=np.uint64)
    for r in np.nonzero(ok)[0]:
        out[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return out


def _masks(n: int, count: int, seed: int, density: float = 0.3) -> list:
    return [_bits(np.random.default_rng(seed + m).random(n) < density) for m in range(count)]


def _stack(masks: list, n: int, gpu, stride: int | None = None) -> torch.Tensor:
    words = stride or (n + 63) // 64
    a = np.zeros((len(masks), words), dtype=np.uint64)
    for m, bits in enumerate(masks):
        a[m, :bits.size] = bits
    return _t(a.view(np.int64).reshape(len(masks), words), gpu)


def _q_mask(nq: int, n_masks: int) -> list:
    """-1 and repeated masks mixed, so that the queries of one wave and of one pass differ."""
    return [-1 if q % 5 == 2 else (q * 7 + q // 3) % n_masks for q in range(nq)]


def _sub(q, sel):
    qi, qx, qv = q
    lists = [(qx[qi[b]:qi[b + 1]], qv[qi[b]:qi[b + 1]]) for b in sel]
    ni = np.zeros(len(lists) + 1, np.int32)
    ni[1:] = np.cumsum([t.size for t, _ in lists])
    return (ni, np.concatenate([t for t, _ in lists] + [np.zeros(0, np.int32)]).astype(np.int32),
            np.concatenate([w for _, w in lists] + [np.zeros(0, np.float32)]).astype(np.float32))


def _oracle(oracle_mod, csr, q, k, masks, q_mask, base=0) -> dict:
    """The oracle's lists of every query under its own mask: one oracle run per distinct mask."""
    nq = q[0].size - 1
    ids = np.full((nq, k), -1, np.int64)
    scores = np.full((nq, k), -np.inf, np.float32)
    count = np.zeros(nq, np.int32)
    for m in sorted(set(q_mask)):
        sel = [b for b in range(nq) if q_mask[b] == m]
        ref = oracle_mod.sparse_topk(*csr, *_sub(q, sel), k, ordinal_base=base,
                                     row_mask=None if m < 0 else masks[m])
        for j, b in enumerate(sel):
            c = int(ref.count[j])
            count[b] = c
            ids[b, :c] = ref.ids[j, :c]
            scores[b, :c] = ref.scores[j, :c]
    return {"ids": ids, "scores": scores, "count": count}


def _run(idx, q, k, stacked, q_mask, gpu, workspace=None) -> dict:
    qm = q_mask if isinstance(q_mask, torch.Tensor) else _t(np.asarray(q_mask, np.int32), gpu)
    out = idx.topk_masks(*(_t(a, gpu) for a in q), k, stacked, qm, workspace=workspace)
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "count", "flags")}


def _same(got: dict, ref: dict, msg=""):
    np.testing.assert_array_equal(got["count"], ref["count"], err_msg=msg)
    for b in range(ref["count"].shape[0]):
        c = ref["count"][b]
        np.testing.assert_array_equal(got["ids"][b, :c], ref["ids"][b, :c], err_msg=f"{msg} query {b}")
        np.testing.assert_array_equal(got["scores"][b, :c], ref["scores"][b, :c],
                                      err_msg=f"{msg} query {b}")
        assert (got["ids"][b, c:] == -1).all(), f"{msg} query {b}"


def _flags_ok(got: dict, filtered_allowed=True):
    f = got["flags"]
    assert ((f & QMASK) != 0).all(), f
    assert (((f & CERTIFIED) != 0) ^ ((f & FALLBACK) != 0)).all(), f
    assert not (f & ~np.uint32(CERTIFIED | FALLBACK | FILTERED | QMASK)).any(), f
    if not filtered_allowed:
        assert not (f & FILTERED).any(), f


def _synthetic(n, b, gpu, seed):
    from audio_rag_amd import synthetic

    csr = tuple(a.cpu().numpy() for a in synthetic.make_sparse_rows(0, n, gpu, seed=seed))
    q = tuple(a.cpu().numpy() for a in synthetic.make_sparse_queries(b, gpu, seed=seed + 1))
    return csr, q


_STORES: dict = {}


def _store(gpu, n):
    """(csr, 150 queries, 5 masks) of an n-row corpus, built once per n."""
    if n not in _STORES:
        csr, q = _synthetic(n, 150, gpu, seed=61 + n % 7)
        _STORES[n] = (csr, q, _masks(n, 5, seed=700 + n % 11))
    return _STORES[n]


# ------------------------------------------------------------------------------------- 1. shapes

@pytest.mark.parametrize("filt", [True, False])
@pytest.mark.parametrize("nq", [1, 64, 65, 150])
@pytest.mark.parametrize("n", [3 * 1024 + 5, 40_000])
def test_shapes_match_oracle(gpu, oracle_mod, n, nq, filt):
    """A partial last tile of both tile sizes (256 and 1024 rows), several row ranges, and the
    second and third pass of 64 queries (the q0 offset into q_mask)."""
    csr, q150, masks = _store(gpu, n)
    q = _sub(q150, range(nq))
    qm = _q_mask(nq, len(masks))
    idx = _index(csr, gpu)
    idx.set_filter(filt)
    stacked = _stack(masks, n, gpu)
    for k in (5, 40):
        got = _run(idx, q, k, stacked, qm, gpu)
        _same(got, _oracle(oracle_mod, csr, q, k, masks, qm), f"k={k}")
        _flags_ok(got, filtered_allowed=filt)


# -------------------------------------------------------------- 2. the filter path really runs

def test_filter_path_runs_and_equals_one_topk_per_mask(gpu, oracle_mod):
    n, nq, k = 120_000, 64, 40
    csr, q = _synthetic(n, nq, gpu, seed=43)
    masks = _masks(n, 8, seed=900)
    qm = [b % 8 for b in range(nq)]
    idx = _index(csr, gpu)
    assert idx.set_filter(True)
    got = _run(idx, q, k, _stack(masks, n, gpu), qm, gpu)
    # the parent path: one masked topk per mask over that mask's queries
    per = {"ids": np.zeros((nq, k), np.int64), "scores": np.zeros((nq, k), np.float32),
           "count": np.zeros(nq, np.int32), "flags": np.zeros(nq, np.uint32)}
    for m in range(8):
        sel = [b for b in range(nq) if qm[b] == m]
        out = idx.topk(*(_t(a, gpu) for a in _sub(q, sel)), k,
                       row_mask=_t(masks[m].view(np.int64), gpu))
        torch.cuda.synchronize()
        for f in per:
            per[f][sel] = getattr(out, f).cpu().numpy()
    share_masks = ((got["flags"] & FILTERED) != 0).mean()
    share_per = ((per["flags"] & FILTERED) != 0).mean()
    assert share_per > 0 and share_masks >= 0.9 * share_per, (share_masks, share_per)
    _flags_ok(got)
    for f in ("ids", "scores", "count"):
        np.testing.assert_array_equal(got[f], per[f], err_msg=f)
    _same(got, _oracle(oracle_mod, csr, q, k, masks, qm))


# -------------------------------------------------- 3. a query is filtered by its own mask only

@pytest.mark.parametrize("filt", [True, False])
@pytest.mark.parametrize("step", [1, 4, 32])
def test_a_query_is_filtered_by_its_own_mask(gpu, oracle_mod, step, filt):
    """Identical terms in columns q and q + step (the same wave of the exact scan, neighbouring
    waves, the two query halves of the filter scan) under complementary masks."""
    n, nq, k = 40_000, 64, 40
    csr, q150, _ = _store(gpu, n)
    rng = np.random.default_rng(17)
    on = rng.random(n) < 0.5
    masks = [_bits(on), _bits(~on)]
    q = _sub(q150, [b if (b // step) % 2 == 0 else b - step for b in range(nq)])
    qm = [0 if (b // step) % 2 == 0 else 1 for b in range(nq)]
    idx = _index(csr, gpu)
    idx.set_filter(filt)
    got = _run(idx, q, k, _stack(masks, n, gpu), qm, gpu)
    for b in range(nq):
        ids = got["ids"][b, :got["count"][b]]
        assert got["count"][b] > 0
        assert (on[ids] == (qm[b] == 0)).all(), f"query {b} returned rows outside its mask"
    _same(got, _oracle(oracle_mod, csr, q, k, masks, qm))
    _flags_ok(got, filtered_allowed=filt)


# ------------------------------------------------------------------- 4. edge masks in one call

@pytest.mark.parametrize("filt", [True, False])
def test_edge_masks_in_one_call(gpu, oracle_mod, filt):
    n, k = 3 * 1024 + 5, 5
    csr, q150, _ = _store(gpu, n)
    need = (n + 63) // 64
    stride = need + 3
    row = np.arange(n)
    garbage = np.zeros(stride, np.uint64)
    garbage[:need] = _bits(np.random.default_rng(3).random(n) < 0.3)
    garbage[need - 1] |= ~np.uint64(0) << np.uint64(n & 63)   # bits past the last row
    garbage[need:] = ~np.uint64(0)
    clean = garbage[:need].copy()
    clean[need - 1] &= (np.uint64(1) << np.uint64(n & 63)) - np.uint64(1)
    masks = [_bits(np.zeros(n, bool)), _bits(np.ones(n, bool)), _bits(row == 1234),
             _bits(row == n - 1), _bits(row >= 3 * 1024), garbage]
    as_oracle = masks[:5] + [clean]
    nq = 14
    q = _sub(q150, range(nq))
    qm = [0, 1, -1, 2, 3, 4, 5, 6, -2, 2**31 - 1, 1, 0, 5, 4]
    stated = [m if -1 <= m < 6 else -1 for m in qm]
    idx = _index(csr, gpu)
    idx.set_filter(filt)
    got = _run(idx, q, k, _stack(masks, n, gpu, stride), _t(np.asarray(qm, np.int32), gpu), gpu)
    ref = _oracle(oracle_mod, csr, q, k, as_oracle, stated)
    _same(got, ref)
    _flags_ok(got, filtered_allowed=filt)
    assert got["count"][0] == 0 and got["count"][11] == 0                 # the empty mask
    # a full mask, -1 and the out-of-range entries: the unfiltered answer bit for bit
    plain = idx.topk(*(_t(a, gpu) for a in q), k)
    torch.cuda.synchronize()
    for b in (1, 2, 7, 8, 9, 10):
        for f in ("ids", "scores", "count"):
            np.testing.assert_array_equal(got[f][b], getattr(plain, f).cpu().numpy()[b])
    # n_masks = 0 with a null row_masks
    empty = torch.empty((0, need), dtype=torch.int64, device=gpu)
    got = _run(idx, q, k, empty, _t(np.asarray([-1, 0, 3] + [-1] * 11, np.int32), gpu), gpu)
    _same(got, _oracle(oracle_mod, csr, q, k, [], [-1] * nq))
    _flags_ok(got, filtered_allowed=filt)


# --------------------------------------------------------- 5. duplicate pile under three masks

@pytest.mark.parametrize("pile", [300, 5000])
def test_duplicate_pile_under_three_masks(gpu, oracle_mod, pile):
    """test_filter_ties_at_the_boundary_take_the_exact_scan's construction: `pile` consecutive
    identical rows above every other row for query 0's terms. 300 rows overflow the lane and
    workgroup lists (the collect list answers), 5000 overflow the collect list of 4096 (the helper
    workgroups answer, and test each row against the query's own mask). Each mask enables a
    different third of the pile."""
    n = 60_000
    csr, q = _synthetic(n, 8, gpu, seed=45)
    ip, ix, iv = csr
    qi, qx, qv = q
    terms = qx[qi[0]:qi[1]]
    dup = (np.sort(terms), np.full(terms.size, 0.4, np.float32))
    rows = [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(n)]
    for j in range(pile):
        rows[1000 + j] = dup
    nip = np.zeros(n + 1, np.int64)
    nip[1:] = np.cumsum([r[0].size for r in rows])
    csr2 = (nip, np.concatenate([r[0] for r in rows]).astype(np.int32),
            np.concatenate([r[1] for r in rows]).astype(np.float32))
    row = np.arange(n)
    in_pile = (row >= 1000) & (row < 1000 + pile)
    rng = np.random.default_rng(23)
    masks = [_bits(np.where(in_pile, (row - 1000) % 3 == m, rng.random(n) < 0.3))
             for m in range(3)]
    # query 0's terms in columns 0, 1, 2, one per mask; the rest ordinary
    q3 = _sub(q, [0, 0, 0, 3, 4, 5, 6, 7])
    qm = [0, 1, 2, 0, 1, 2, -1, 0]
    idx = _index(csr2, gpu)
    got = _run(idx, q3, 5, _stack(masks, n, gpu), qm, gpu)
    assert not (got["flags"][0] & FILTERED), got["flags"]
    _flags_ok(got)
    ref = _oracle(oracle_mod, csr2, q3, 5, masks, qm)
    _same(got, ref)
    for m in range(3):  # the five lowest pile rows of the query's own third
        want = 1000 + np.nonzero((np.arange(pile) % 3) == m)[0][:5]
        np.testing.assert_array_equal(got["ids"][m], want)


# ------------------------------------------------------------------ 6. special rows and weights

def test_adversarial_rows_under_two_masks(gpu, oracle_mod):
    csr, terms, lab = adv.corpus(adv.N, adv.SEED)
    q, kinds = adv.queries(terms, adv.N_ORDINARY, adv.SEED)
    nq = q[0].size - 1
    ok = adv.keep_half(lab, adv.SEED)
    masks = [adv.bits(ok), adv.bits(~ok)]
    qm = [b % 3 - 1 for b in range(nq)]          # -1, 0, 1 in turn: every kind under several
    idx = _index(csr, gpu, base=adv.BASE)
    stacked = _stack(masks, adv.N, gpu)
    for filt in (True, False):
        idx.set_filter(filt)
        for k in (5, 20, 240):
            got = _run(idx, q, k, stacked, qm, gpu)
            _same(got, _oracle(oracle_mod, csr, q, k, masks, qm, base=adv.BASE), f"k={k} filter={filt}")
            _flags_ok(got, filtered_allowed=filt)


def test_negative_and_zero_weights_under_their_own_masks(gpu, oracle_mod):
    n = 40_000
    csr, q150, masks = _store(gpu, n)
    q = _sub(q150, range(16))
    qv = q[2].copy()
    qv[q[0][3]] = -0.25        # query 3: a negative weight
    qv[q[0][9] + 1] = 0.0      # query 9: a +0.0 weight
    q2 = (q[0], q[1], qv)
    qm = _q_mask(16, 5)
    qm[3], qm[9] = 1, 4
    idx = _index(csr, gpu)
    got = _run(idx, q2, 20, _stack(masks, n, gpu), qm, gpu)
    assert not (got["flags"][3] & FILTERED) and not (got["flags"][9] & FILTERED)
    _flags_ok(got)
    _same(got, _oracle(oracle_mod, csr, q2, 20, masks, qm))


# ---------------------------------------------------------------------- 7. workspace and graph

def test_caller_workspace_graph_replay_and_ordinal_base(gpu, oracle_mod):
    from audio_rag_amd._armi import call, ptr, stream_handle
    from audio_rag_amd.retrieval.device import TopK

    n, nq, k = 40_000, 65, 5
    csr, q150, masks = _store(gpu, n)
    q = _sub(q150, range(nq))
    idx = _index(csr, gpu, base=3)
    ws = torch.empty(idx.workspace_bytes(nq, k), dtype=torch.uint8, device=gpu)
    stacked = _stack(masks[:3], n, gpu)
    qm = _q_mask(nq, 3)
    qm_dev = _t(np.asarray(qm, np.int32), gpu)
    got = _run(idx, q, k, stacked, qm_dev, gpu, workspace=ws)
    _same(got, _oracle(oracle_mod, csr, q, k, masks[:3], qm, base=3), "caller workspace")
    _flags_ok(got)

    qd = tuple(_t(a, gpu) for a in q)
    out = TopK.empty(nq, k, gpu, rank=False)

    def launch():
        call("armi_sparse_topk_qmask", idx.handle, ptr(qd[0]), ptr(qd[1]), ptr(qd[2]), nq, k,
             ptr(stacked), int(stacked.shape[1]), ptr(qm_dev), 3, ptr(out.scores), ptr(out.ids),
             ptr(out.count), ptr(out.flags), ptr(ws), ws.numel(), stream_handle())

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for masks_now, qm_now in ((masks[:3], qm), (masks[2:5], [(m + 1) % 3 if m >= 0 else 0 for m in qm])):
        stacked.copy_(_stack(masks_now, n, gpu))
        qm_dev.copy_(_t(np.asarray(qm_now, np.int32), gpu))
        graph.replay()
        torch.cuda.synchronize()
        got = {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "count", "flags")}
        _same(got, _oracle(oracle_mod, csr, q, k, masks_now, qm_now, base=3), "replay")
        _flags_ok(got)


def test_argument_errors_before_any_device_work(gpu):
    from audio_rag_amd import _armi
    from audio_rag_amd._armi import call, ptr, stream_handle
    from audio_rag_amd.retrieval.device import TopK

    n = 3 * 1024 + 5
    csr, q150, masks = _store(gpu, n)
    idx = _index(csr, gpu)
    qd = tuple(_t(a, gpu) for a in _sub(q150, range(4)))
    stacked = _stack(masks[:2], n, gpu)
    qm = _t(np.asarray([0, 1, -1, 0], np.int32), gpu)
    out = TopK.empty(4, 5, gpu, rank=False)
    ws = torch.empty(idx.workspace_bytes(4, 5), dtype=torch.uint8, device=gpu)

    def launch(k=5, stride=(n + 63) // 64, n_masks=2, q_mask=qm, ws_bytes=ws.numel()):
        call("armi_sparse_topk_qmask", idx.handle, ptr(qd[0]), ptr(qd[1]), ptr(qd[2]), 4, k,
             ptr(stacked), stride, ptr(q_mask) if q_mask is not None else None, n_masks,
             ptr(out.scores), ptr(out.ids), ptr(out.count), ptr(out.flags), ptr(ws), ws_bytes,
             stream_handle())

    for kw, text in (({"stride": (n + 63) // 64 - 1}, "mask_stride_words"),
                     ({"n_masks": -1}, "n_masks < 0"), ({"k": 0}, "k must be"),
                     ({"k": 241}, "k must be"), ({"q_mask": None}, "null pointer"),
                     ({"ws_bytes": 16}, "workspace too small")):
        with pytest.raises(_armi.ArmiError, match=text) as e:
            launch(**kw)
        assert e.value.code == _armi.ARMI_ERR_INVALID, kw
    # the Python layer's own checks
    with pytest.raises(ValueError, match="words"):
        idx.topk_masks(*qd, 5, stacked[:, :-1].contiguous(), qm)
    with pytest.raises(ValueError, match="4 queries"):
        idx.topk_masks(*qd, 5, stacked, qm[:3])
    with pytest.raises(ValueError, match=r"in \[-1, 2\)"):
        idx.topk_masks(*qd, 5, stacked, torch.tensor([0, 1, 2, -1], dtype=torch.int32))
