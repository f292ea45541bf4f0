"""The end of a first-pass dense scan: each wave folds its lane lists into the workgroup's running
list as its tile loop ends (scan_wave_fold in dense.hip), for dense_scan_kernel (k > 64), the int8
scan (k <= 64) and its per-query-mask form, single and two-block calls.

Every answer must be bit-identical (ids, rank keys, scores, counts) to oracle.dense_topk. The
shapes are the smallest at which the fold can go wrong: fewer tiles than waves (waves fold empty
lists), exactly one tile per wave, a workgroup with more tiles than waves, ragged last tiles, a
pile of equal best rows larger than the list (cut in the lane lists, or only in the fold), filters
that leave whole waves without a row. A reference is computed once per store at the largest k and
its prefixes serve the smaller k.

How rows meet waves: a workgroup owns a range of 32-row tiles and its 8 waves take them in order,
one each before any takes a second. The plan gives a range at most 8 tiles until the store has
more than 8 tiles per CU, so the 9-, 10- and 18-tile stores are dealt to two or three workgroups
(5 + 4, 5 + 5, 6 + 6 + 6 tiles: again waves without a tile); `test_a_wave_with_a_second_tile`
is the store large enough for 9-tile ranges. The fp16 scan's tile t holds ordinals 32 t ..; the
int8 image is scattered (armi_index.h): ordinal i sits in image tile (i % T) * perm_mul % T at
row i / T, T the number of tiles."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = 3       # ordinal_base of every index here
KMAX = 65      # k = 65 takes the fp16 scan; every smaller k here the int8 scan
KS = (1, 5, 16, 17, 40, 65)


def _bits(on: np.ndarray) -> np.ndarray:
    """bool [n] -> uint64 bitmask words (bit r of word r // 64)."""
    w = np.zeros((on.shape[0] + 63) // 64, dtype=np.uint64)
    idx = np.flatnonzero(on)
    np.bitwise_or.at(w, idx >> 6, np.left_shift(np.uint64(1), (idx & 63).astype(np.uint64)))
    return w


def _f16(a: np.ndarray, gpu) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float16)).to(gpu)


def _mask(words: np.ndarray, gpu) -> torch.Tensor:
    return torch.from_numpy(words.view(np.int64)).to(gpu)


def _arrays(out) -> dict:
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in ("ids", "scores", "rank", "count", "flags")}


def _assert_same(got: dict, ref, k: int, msg=""):
    """got == the first k of the reference lists (computed at some k' >= k)."""
    count = np.minimum(ref.count, k)
    np.testing.assert_array_equal(got["count"], count, err_msg=msg)
    for b, c in enumerate(count):
        for f in ("ids", "rank", "scores"):
            np.testing.assert_array_equal(got[f][b, :c], getattr(ref, f)[b, :c],
                                          err_msg=f"{msg} {f} query {b}")
        assert (got["ids"][b, c:] == -1).all(), f"{msg} ids past the count, query {b}"


def _image_tile(i: np.ndarray, n: int) -> np.ndarray:
    """Image tile of ordinal i in the int8 image of an n-row store (armi_index.h)."""
    t = (n + 31) // 32
    if t == 1:
        return np.zeros_like(i)
    p = max(1, int(t * 0.6180339887498949))
    while math.gcd(p, t) != 1:
        p += 1
    return (i % t) * (p % t) % t


def _tile_ordinals(tile: int, n: int) -> np.ndarray:
    """Ordinals of image tile `tile`, by image row."""
    i = np.arange(n)
    return i[_image_tile(i, n) == tile]            # ascending ordinal = ascending image row


_stores: dict = {}


def _store(oracle_mod, gpu, n, dim):
    """(index, rows, 128 queries, reference at KMAX for the 128) of one (n, dim)."""
    from audio_rag_amd.retrieval.device import DenseIndex

    if (n, dim) not in _stores:
        rows = oracle_mod.unit_fp16(n, dim, seed=2000 + n + dim)
        qs = oracle_mod.unit_fp16(128, dim, seed=2001 + n + dim)
        idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
        ref = oracle_mod.dense_topk(rows, qs, KMAX, ordinal_base=BASE)
        _stores[(n, dim)] = (idx, rows, qs, ref)
    return _stores[(n, dim)]


def _head(ref, nq):
    """The reference lists of the first nq queries."""
    class R:
        pass
    r = R()
    for f in ("ids", "rank", "scores", "count"):
        setattr(r, f, getattr(ref, f)[:nq])
    return r


# --------------------------------------------------------------------------------- row counts

@pytest.mark.parametrize("dim", [1024, 256])
@pytest.mark.parametrize("tiles", [1, 7, 8, 9, 17])
def test_row_counts_match_oracle(gpu, oracle_mod, tiles, dim):
    """32 * tiles + 5 rows: 2 tiles (six waves fold empty lists), 8 (one tile per wave), 9, 10 and
    18 (two and three workgroups, each with waves that have no tile); the last tile has 5 rows.
    64 queries fill every lane of the fold, 37 leave lanes without a query."""
    from audio_rag_amd import _armi

    n = 32 * tiles + 5
    idx, rows, qs, ref = _store(oracle_mod, gpu, n, dim)
    for nq in (64, 37):
        q = _f16(qs[:nq], gpu)
        for k in KS:
            want_form = _armi.SCAN_FP16 if k > 64 else _armi.SCAN_INT8_FILTER
            assert idx.scan_form(nq, k) == want_form
            got = _arrays(idx.topk(q, k))
            _assert_same(got, _head(ref, nq), k, f"n={n} dim={dim} nq={nq} k={k}")
            assert set(np.unique(got["flags"])) <= {1, 2}


def test_a_wave_with_a_second_tile(gpu, oracle_mod):
    """More than 8 tiles per CU, so that a range has 9 tiles and one wave of every workgroup takes
    a second one from the workgroup's counter (dim 256 keeps the store at 34 MB)."""
    from audio_rag_amd.retrieval.device import DenseIndex

    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = 32 * (8 * min(cus, 256) + 1) + 5
    rows = oracle_mod.unit_fp16(n, 256, seed=2100)
    qs = oracle_mod.unit_fp16(64, 256, seed=2101)
    idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
    ref = oracle_mod.dense_topk(rows, qs, KMAX, ordinal_base=BASE)
    q = _f16(qs, gpu)
    for k in (5, 40, 65):
        _assert_same(_arrays(idx.topk(q, k)), ref, k, f"k={k}")


# ---------------------------------------------------------------------------------- multi-block

@pytest.mark.parametrize("dim", [1024, 256])
@pytest.mark.parametrize("nq", [65, 128])
def test_two_query_blocks(gpu, oracle_mod, nq, dim):
    """65 and 128 queries: the grid of (range, block) workgroups, each block's lists at its own
    out_base; both scans (k = 65: dense_scan_kernel over two blocks)."""
    idx, rows, qs, ref = _store(oracle_mod, gpu, 32 * 17 + 5, dim)
    q = _f16(qs[:nq], gpu)
    for k in (5, 17, 65):
        _assert_same(_arrays(idx.topk(q, k)), _head(ref, nq), k, f"nq={nq} dim={dim} k={k}")


# ---------------------------------------------------------------------------- truncation piles

PILE_N = 32 * 31 + 5        # 32 tiles: four workgroups of 8 tiles, one tile per wave
PILE = 40


def _pile_store(oracle_mod, gpu, pile_ords):
    """Random unit rows with one vector repeated at pile_ords; that vector asked at queries 0 and
    33 (columns r and 32 + r of the fold) among random queries."""
    from audio_rag_amd.retrieval.device import DenseIndex

    rows = oracle_mod.unit_fp16(PILE_N, 1024, seed=2200).copy()
    v = oracle_mod.unit_fp16(1, 1024, seed=2201)
    rows[pile_ords] = v
    qs = oracle_mod.unit_fp16(64, 1024, seed=2202).copy()
    qs[[0, 33]] = v
    return DenseIndex(_f16(rows, gpu), ordinal_base=BASE), rows, qs


def _check_pile(oracle_mod, gpu, pile_ords):
    from audio_rag_amd import _armi

    assert len(pile_ords) == PILE and len(set(pile_ords.tolist())) == PILE
    tiles = _image_tile(pile_ords, PILE_N)
    assert tiles.min() >= 8 and tiles.max() < 16      # inside the second workgroup's range
    idx, rows, qs = _pile_store(oracle_mod, gpu, pile_ords)
    got = _arrays(idx.topk(_f16(qs, gpu), 5))
    _assert_same(got, oracle_mod.dense_topk(rows, qs, 5, ordinal_base=BASE), 5)
    lowest = [BASE + int(o) for o in np.sort(pile_ords)[:5]]
    for p in (0, 33):
        # 16 of the 40 equal keys fit the workgroup's list: the other 24 are the bound, which then
        # equals the k-th key, so nothing certifies the list and the collect pass answers
        assert not got["flags"][p] & _armi.ARMI_FLAG_CERTIFIED, got["flags"]
        assert got["flags"][p] & _armi.ARMI_FLAG_FALLBACK
        assert list(got["ids"][p]) == lowest
    # the same store through the fp16 scan (all 40 in its top-65)
    _assert_same(_arrays(idx.topk(_f16(qs, gpu), 65)),
                 oracle_mod.dense_topk(rows, qs, 65, ordinal_base=BASE), 65)


def test_pile_in_two_tiles(gpu, oracle_mod):
    """40 identical best rows in two image tiles of one workgroup (20 each): the lane lists keep 4
    of the 12 and of the 8 a lane half sees, and the two waves' 16 survivors fill the list."""
    ords = np.concatenate([_tile_ordinals(t, PILE_N)[:20] for t in (9, 10)])
    _check_pile(oracle_mod, gpu, ords)


def test_pile_split_across_waves(gpu, oracle_mod):
    """The same pile, 5 rows in each of the workgroup's 8 tiles, i.e. per wave, at image rows 0-2
    (lane half 0) and 4-5 (lane half 1): no lane list discards any, 40 reach the fold and it drops
    24 of them."""
    ords = np.concatenate([_tile_ordinals(t, PILE_N)[[0, 1, 2, 4, 5]] for t in range(8, 16)])
    _check_pile(oracle_mod, gpu, ords)


# ---------------------------------------------------------------------------------------- masks

def _wave_emptying_masks(n: int) -> list:
    """Two filters over an n-row store: one keeps the rows of every eighth IMAGE tile (int8 scan),
    one the rows of every eighth 32-row tile of the store (fp16 scan), so that in each form most
    waves of a workgroup see no enabled row, under the other filter every wave only a few."""
    i = np.arange(n)
    return [_bits(_image_tile(i, n) % 8 == 2), _bits((i // 32) % 8 == 5)]


@pytest.mark.parametrize("dim", [1024, 256])
def test_row_mask_that_empties_whole_waves(gpu, oracle_mod, dim):
    n = 32 * 17 + 5
    idx, rows, qs, _ = _store(oracle_mod, gpu, n, dim)
    q = _f16(qs[:64], gpu)
    for m, words in enumerate(_wave_emptying_masks(n)):
        ref = oracle_mod.dense_topk(rows, qs[:64], KMAX, ordinal_base=BASE, row_mask=words)
        assert 0 < ref.count.max() <= 96
        for k in (5, 40, 65):
            got = _arrays(idx.topk(q, k, row_mask=_mask(words, gpu)))
            _assert_same(got, ref, k, f"dim={dim} mask={m} k={k}")


def test_two_masks_in_one_qmask_call(gpu, oracle_mod):
    """armi_dense_topk_qmask: the two filters above in one call of 65 queries (both blocks), every
    third query unfiltered."""
    from audio_rag_amd import _armi

    n = 32 * 17 + 5
    idx, rows, qs, plain = _store(oracle_mod, gpu, n, 1024)
    nq = 65
    masks = _wave_emptying_masks(n)
    qm = np.array([-1 if q % 3 == 0 else q % 2 for q in range(nq)], dtype=np.int32)
    refs = {-1: _head(plain, nq)}
    for m in (0, 1):
        refs[m] = oracle_mod.dense_topk(rows, qs[:nq], KMAX, ordinal_base=BASE, row_mask=masks[m])
    stacked = torch.from_numpy(np.stack(masks).view(np.int64)).to(gpu)
    for k in (5, 40):
        got = _arrays(idx.topk_masks(_f16(qs[:nq], gpu), k, stacked, torch.from_numpy(qm).to(gpu)))
        assert ((got["flags"] & _armi.ARMI_FLAG_QMASK) != 0).all()
        for q in range(nq):
            ref = refs[int(qm[q])]
            c = min(int(ref.count[q]), k)
            assert got["count"][q] == c, f"k={k} query {q}"
            for f in ("ids", "rank", "scores"):
                np.testing.assert_array_equal(got[f][q, :c], getattr(ref, f)[q, :c],
                                              err_msg=f"k={k} {f} query {q}")


# ------------------------------------------------------------------------------- certification

def test_plain_data_is_all_certified(gpu, oracle_mod):
    """Random unit rows, 20k x 1024, 64 queries, top-5: every query is answered by the first pass
    and its certificate (the lists' bounds are no looser than the barrier merge's, which
    certified all of them at this shape), so a wrong list cannot hide behind the collect pass."""
    from audio_rag_amd import _armi
    from audio_rag_amd.retrieval.device import DenseIndex

    rows = oracle_mod.unit_fp16(20000, 1024, seed=2300)
    qs = oracle_mod.unit_fp16(64, 1024, seed=2301)
    idx = DenseIndex(_f16(rows, gpu), ordinal_base=BASE)
    got = _arrays(idx.topk(_f16(qs, gpu), 5))
    assert (got["flags"] == _armi.ARMI_FLAG_CERTIFIED).all(), got["flags"]
    _assert_same(got, oracle_mod.dense_topk(rows, qs, 5, ordinal_base=BASE), 5)
