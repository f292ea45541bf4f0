"""armi_dense_tail_topk_qmask (TailIndex.tail_topk_masks): the fused tail pass in which every query
carries its own mask over the tail's rows.

Every answer must be bit-identical (ids, float64 rank keys, fp32 scores, counts, the -1 / -inf
padding) to two references: oracle.dense_topk over main + tail with the query's combined mask, and
TailIndex.tail_topk(row_mask=...) called once per distinct mask with the same main lists. The main
lists come from DenseIndex.topk_masks (k <= 64) or one DenseIndex.topk(row_mask=...) per mask
(k = 240, which the int8 qmask form does not serve). An oracle list is computed once per (tail
size, query, mask) at k = 240; its prefixes serve the smaller k."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAIN = 4096
KMAX = 240
TAILS = (1, 33, 65, 257, 1000)   # one row; second tile (upper half of a mask word); second uint64
#                                  word; second scan workgroup (256 rows each); a larger tail


def _bits(on: np.ndarray, words: int | None = None) -> np.ndarray:
    """bool [n] -> uint64 bitmask words (bit r of word r // 64), at least one word."""
    n = on.shape[0]
    w = np.zeros(words or max((n + 63) // 64, 1), dtype=np.uint64)
    idx = np.flatnonzero(on)
    np.bitwise_or.at(w, idx >> 6, np.left_shift(np.uint64(1), (idx & 63).astype(np.uint64)))
    return w


def _dev(a: np.ndarray, gpu) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _f16(a: np.ndarray, gpu) -> torch.Tensor:
    return _dev(a.view(np.float16), gpu)


def _arrays(out) -> dict:
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "rank", "count", "flags")}


def _tail(rows_u16, gpu, base=MAIN):
    from audio_rag_amd.retrieval.device import TailIndex

    t = TailIndex(rows_u16.shape[1], max(len(rows_u16), 1), base, gpu)
    t.append(_f16(rows_u16, gpu))
    return t


def _tail_stack(oks: list, tail_n: int, gpu) -> torch.Tensor:
    """The tail halves of the masks as int64 [n_masks, words + 1] on the device. Every bit past the
    last tail row is SET, in the last word and in a spare word behind it: they must be ignored."""
    words = (tail_n + 63) // 64
    out = np.full((len(oks), words + 1), ~np.uint64(0), dtype=np.uint64)
    for i, ok in enumerate(oks):
        out[i, :words] = _bits(ok[MAIN:])
        if tail_n % 64:
            out[i, words - 1] |= ~np.uint64(0) << np.uint64(tail_n % 64)
    return _dev(out.view(np.int64), gpu)


def _main_stack(oks: list, gpu) -> torch.Tensor:
    return _dev(np.stack([_bits(ok[:MAIN]) for ok in oks]).view(np.int64), gpu)


def _masks(tail_n: int) -> list:
    """The masks of one call as bool [MAIN + tail_n]: 0 a random half (shared by two queries),
    1 all-zero, 2 tail bits only, 3 main bits only, 4 a random 30 %, 5 three main rows and all but
    one tail row (a main list shorter than any k here, so thr = -inf)."""
    rng = np.random.default_rng(tail_n)
    n = MAIN + tail_n
    oks = [rng.random(n) < 0.5, np.zeros(n, dtype=bool), np.arange(n) >= MAIN, np.arange(n) < MAIN,
           rng.random(n) < 0.3, np.zeros(n, dtype=bool)]
    oks[5][[5, 700, 4000]] = True
    oks[5][MAIN:] = True
    oks[5][MAIN + tail_n // 2] = False
    return oks


def _q_mask(nq: int, n_masks: int) -> list:
    """Per query: its mask, -1, or an entry out of range (n_masks and -7: unfiltered)."""
    pattern = [0, -1, 0, 1, 2, 3, 4, 5, n_masks, -7]
    return [pattern[q % len(pattern)] for q in range(nq)]


def _eff(m: int, n_masks: int) -> int:
    return m if 0 <= m < n_masks else -1


@pytest.fixture(scope="module")
def segs(gpu, oracle_mod):
    """dim -> (rows of main + the largest tail, 70 queries, the main DenseIndex)."""
    from audio_rag_amd.retrieval.device import DenseIndex

    out = {}
    for dim in (1024, 256):
        rows = oracle_mod.unit_fp16(MAIN + 1100, dim, seed=190 + dim)
        qs = oracle_mod.unit_fp16(70, dim, seed=191 + dim)
        out[dim] = (rows, qs, DenseIndex(_f16(rows[:MAIN], gpu)))
    return out


_oracle: dict = {}


def _oracle_lists(oracle_mod, rows, qs, oks, q_mask, key) -> dict:
    """oracle.dense_topk at KMAX of every query under its own combined mask (cached per query and
    mask under `key`)."""
    b = len(q_mask)
    ref = {"ids": np.empty((b, KMAX), np.int64), "rank": np.empty((b, KMAX), np.float64),
           "scores": np.empty((b, KMAX), np.float32), "count": np.empty(b, np.int32)}
    eff = [_eff(m, len(oks)) for m in q_mask]
    for m in sorted(set(eff)):
        todo = [q for q in range(b) if eff[q] == m and (key, q, m) not in _oracle]
        if todo:
            r = oracle_mod.dense_topk(rows, qs[todo], KMAX,
                                      row_mask=None if m < 0 else _bits(oks[m]))
            for j, q in enumerate(todo):
                _oracle[(key, q, m)] = (r.ids[j], r.rank[j], r.scores[j], r.count[j])
        for q in range(b):
            if eff[q] == m:
                ref["ids"][q], ref["rank"][q], ref["scores"][q], ref["count"][q] = \
                    _oracle[(key, q, m)]
    return ref


def _assert_oracle(got: dict, ref: dict, k: int, msg=""):
    count = np.minimum(ref["count"], k)
    np.testing.assert_array_equal(got["count"], count, err_msg=msg)
    for b, c in enumerate(count):
        for f in ("ids", "rank", "scores"):
            np.testing.assert_array_equal(got[f][b, :c], ref[f][b, :c], err_msg=f"{msg} {f} q{b}")
        assert (got["ids"][b, c:] == -1).all(), f"{msg} ids past the count, query {b}"
        assert np.isneginf(got["scores"][b, c:]).all(), f"{msg} scores past the count, query {b}"


def _main_lists(main_idx, q, k, mstack, oks, q_mask, gpu):
    """The main index's list of every query under its own mask."""
    from audio_rag_amd.retrieval.device import TopK

    nq = len(q_mask)
    if k <= 64:
        return main_idx.topk_masks(q, k, mstack, _dev(np.asarray(q_mask, np.int32), gpu))
    out = TopK.empty(nq, k, gpu, rank=True)
    eff = [_eff(m, len(oks)) for m in q_mask]
    for m in sorted(set(eff)):
        it = torch.tensor([i for i in range(nq) if eff[i] == m], device=gpu)
        part = main_idx.topk(q[it].contiguous(), k, row_mask=None if m < 0 else mstack[m])
        for f in ("scores", "ids", "rank", "count", "flags"):
            getattr(out, f).index_copy_(0, it, getattr(part, f))
    return out


def _assert_per_mask(tail, q, k, main, tstack, q_mask, got, n_masks, qmask_bit):
    """tail_topk(row_mask=...) once per distinct mask over the same main lists: the queries of
    that mask must agree in every output word, the flags up to the QMASK bit."""
    eff = [_eff(m, n_masks) for m in q_mask]
    for m in sorted(set(eff)):
        one = _arrays(tail.tail_topk(q, k, main, row_mask=None if m < 0 else tstack[m]))
        sel = [i for i in range(len(q_mask)) if eff[i] == m]
        for f in ("ids", "rank", "scores", "count"):
            np.testing.assert_array_equal(got[f][sel], one[f][sel], err_msg=f"mask {m} {f}")
        np.testing.assert_array_equal(got["flags"][sel], one["flags"][sel] | qmask_bit)


CASES = [(t, 70, k, 1024) for t in TAILS for k in (5, 64, 240)] + \
        [(t, b, k, 1024) for t in (33, 257) for b in (1, 65) for k in (5, 240)] + \
        [(65, 70, 64, 256), (257, 65, 5, 256)]


@pytest.mark.parametrize("tail_n,nq,k,dim", CASES)
def test_matches_the_oracle_and_one_call_per_mask(gpu, oracle_mod, segs, tail_n, nq, k, dim):
    from audio_rag_amd import _armi

    rows, qs, main_idx = segs[dim]
    oks = _masks(tail_n)
    q_mask = _q_mask(nq, len(oks))
    q = _f16(qs[:nq], gpu)
    tail = _tail(rows[MAIN:MAIN + tail_n], gpu)
    mstack, tstack = _main_stack(oks, gpu), _tail_stack(oks, tail_n, gpu)
    main = _main_lists(main_idx, q, k, mstack, oks, q_mask, gpu)
    # q_mask holds exactly nq entries, on the device (the second 64-query block is partly filled)
    qm = _dev(np.asarray(q_mask, np.int32), gpu)
    assert qm.numel() == nq
    got = _arrays(tail.tail_topk_masks(q, k, main, tstack, qm))
    ref = _oracle_lists(oracle_mod, rows[:MAIN + tail_n], qs, oks, q_mask, (dim, tail_n))
    _assert_oracle(got, ref, k)
    _assert_per_mask(tail, q, k, main, tstack, q_mask, got, len(oks), _armi.ARMI_FLAG_QMASK)
    assert ((got["flags"] & _armi.ARMI_FLAG_QMASK) != 0).all()
    # mask 5's main list is short, so every enabled tail row survives; none of these tails passes
    # the list capacity, so nothing may fall back
    assert ((got["flags"] & ~_armi.ARMI_FLAG_QMASK) == _armi.ARMI_FLAG_CERTIFIED).all()
    unf = [i for i, m in enumerate(q_mask) if _eff(m, len(oks)) < 0]
    if len(unf) > 1:  # -1, n_masks and -7 are all the unfiltered answer
        plain = _arrays(tail.tail_topk(q, k, main))
        for f in ("ids", "rank", "scores", "count"):
            np.testing.assert_array_equal(got[f][unf], plain[f][unf])


def test_no_masks_at_all(gpu, oracle_mod, segs):
    """n_masks = 0 with a null stack: every query is unfiltered."""
    rows, qs, main_idx = segs[1024]
    q = _f16(qs[:9], gpu)
    tail = _tail(rows[MAIN:MAIN + 65], gpu)
    main = main_idx.topk(q, 5)
    empty = torch.empty((0, 2), dtype=torch.int64, device=gpu)
    got = _arrays(tail.tail_topk_masks(q, 5, main, empty, _dev(np.full(9, -1, np.int32), gpu)))
    want = _arrays(tail.tail_topk(q, 5, main))
    for f in ("ids", "rank", "scores", "count"):
        np.testing.assert_array_equal(got[f], want[f])


def test_overflowed_query_filters_by_its_own_mask(gpu, oracle_mod, segs):
    """A short main list over a 1100-row tail under a mask that enables more rows than the
    survivor list holds: that query takes the exhaustive pass under its own mask; its neighbour in
    the block, under a sparse mask, stays certified."""
    from audio_rag_amd import _armi
    from audio_rag_amd.retrieval.device import TailIndex

    rows, qs, main_idx = segs[1024]
    tail_n, cap = 1100, TailIndex.list_cap()
    rng = np.random.default_rng(11)
    wide = np.zeros(MAIN + tail_n, dtype=bool)
    wide[[9, 1234]] = True                        # two main rows: no k-th key, thr = -inf
    wide[MAIN:] = True
    wide[MAIN + rng.choice(tail_n, 40, replace=False)] = False
    assert wide[MAIN:].sum() > cap
    thin = rng.random(MAIN + tail_n) < 0.05
    oks = [wide, thin]
    q_mask = [1, 0, 1, -1]
    q = _f16(qs[:4], gpu)
    tail = _tail(rows[MAIN:MAIN + tail_n], gpu)
    mstack, tstack = _main_stack(oks, gpu), _tail_stack(oks, tail_n, gpu)
    for k in (5, 64):
        main = _main_lists(main_idx, q, k, mstack, oks, q_mask, gpu)
        got = _arrays(tail.tail_topk_masks(q, k, main, tstack, _dev(np.asarray(q_mask, np.int32), gpu)))
        ref = _oracle_lists(oracle_mod, rows[:MAIN + tail_n], qs, oks, q_mask, "overflow")
        _assert_oracle(got, ref, k)
        ids = got["ids"][1]
        assert wide[ids[ids >= 0]].all()
        assert got["flags"][1] == _armi.ARMI_FLAG_FALLBACK | _armi.ARMI_FLAG_QMASK
        for b in (0, 2, 3):
            assert got["flags"][b] == _armi.ARMI_FLAG_CERTIFIED | _armi.ARMI_FLAG_QMASK
        _assert_per_mask(tail, q, k, main, tstack, q_mask, got, 2, _armi.ARMI_FLAG_QMASK)


def test_invalid_appended_row_under_a_set_bit_is_never_returned(gpu, oracle_mod):
    from audio_rag_amd.retrieval.device import DenseIndex

    rows = oracle_mod.unit_fp16(MAIN + 40, 256, seed=280).copy()
    rows[MAIN + 17, 3] = 0x7C00  # +inf
    qs = oracle_mod.unit_fp16(6, 256, seed=281)
    main_idx = DenseIndex(_f16(rows[:MAIN], gpu))
    tail = _tail(rows[MAIN:], gpu)
    assert tail.invalid_rows() == 1
    rng = np.random.default_rng(3)
    oks = [rng.random(MAIN + 40) < 0.5, np.arange(MAIN + 40) >= MAIN]
    for ok in oks:
        ok[MAIN + 17] = True
    q_mask = [0, 1, -1, 0, 1, -1]
    q = _f16(qs, gpu)
    mstack, tstack = _main_stack(oks, gpu), _tail_stack(oks, 40, gpu)
    valid = np.ones(MAIN + 40, dtype=bool)
    valid[MAIN + 17] = False
    for k in (5, 64):
        main = _main_lists(main_idx, q, k, mstack, oks, q_mask, gpu)
        got = _arrays(tail.tail_topk_masks(q, k, main, tstack, _dev(np.asarray(q_mask, np.int32), gpu)))
        assert not (got["ids"] == MAIN + 17).any()
        # (the oracle does not know invalid rows: the row's bit is cleared in its masks)
        ref = _oracle_lists(oracle_mod, rows, qs, [ok & valid for ok in oks] + [valid],
                            [2 if m < 0 else m for m in q_mask], "invalid")
        _assert_oracle(got, ref, k)
    assert got["count"][1] == 39 and got["count"][4] == 39  # k = 64 over the tail's 39 valid rows


def test_graph_capture_and_replay_equal_the_eager_run(gpu, oracle_mod, segs):
    rows, qs, main_idx = segs[1024]
    tail_n, nq, k = 257, 70, 5
    oks = _masks(tail_n)
    q_mask = _q_mask(nq, len(oks))
    q = _f16(qs[:nq], gpu)
    tail = _tail(rows[MAIN:MAIN + tail_n], gpu)
    mstack, tstack = _main_stack(oks, gpu), _tail_stack(oks, tail_n, gpu)
    qm = _dev(np.asarray(q_mask, np.int32), gpu)
    ws_m = torch.empty(main_idx.qmask_workspace_bytes(nq, k, len(oks)), dtype=torch.uint8, device=gpu)
    ws_t = torch.empty(max(tail.tail_workspace_bytes(nq, k), 1), dtype=torch.uint8, device=gpu)

    def run():
        main = main_idx.topk_masks(q, k, mstack, qm, workspace=ws_m)
        return tail.tail_topk_masks(q, k, main, tstack, qm, workspace=ws_t)

    eager = _arrays(run())
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for f in ("ids", "scores", "rank", "count", "flags"):
        getattr(out, f).zero_()
    graph.replay()
    replayed = _arrays(out)
    for f in ("ids", "scores", "rank", "count", "flags"):
        np.testing.assert_array_equal(replayed[f], eager[f], err_msg=f)


def test_python_argument_checks(gpu, oracle_mod, segs):
    rows, qs, main_idx = segs[1024]
    q = _f16(qs[:4], gpu)
    tail = _tail(rows[MAIN:MAIN + 129], gpu)
    main = main_idx.topk(q, 5)
    qm = _dev(np.zeros(4, np.int32), gpu)
    with pytest.raises(ValueError, match="words"):       # 129 rows need three words
        tail.tail_topk_masks(q, 5, main, torch.zeros((1, 2), dtype=torch.int64, device=gpu), qm)
    ok = torch.zeros((1, 3), dtype=torch.int64, device=gpu)
    with pytest.raises(ValueError, match="q_mask"):
        tail.tail_topk_masks(q, 5, main, ok, qm[:3].contiguous())
    with pytest.raises(ValueError, match="q_mask entries"):
        tail.tail_topk_masks(q, 5, main, ok, torch.tensor([0, 1, 0, 0], dtype=torch.int32))
    with pytest.raises(ValueError, match="main"):
        tail.tail_topk_masks(q, 5, main_idx.topk(q, 6), ok, qm)
