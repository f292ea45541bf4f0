"""The oracle on the adversarial rows of tests/adversarial.py (subnormal rows, power-of-two
multiples, spikes, zero rows, one-ulp neighbours, invalid rows), pinned against a plain numpy int64
restatement of its arithmetic before the GPU tests lean on it:

  fixed = int(x * 2^24) (exact for every fp16 x with |x| < 2; |fixed| < 2^25, so a 1024-term sum of
  products stays below 2^60: no int64 overflow), norm2 = sum fixed^2, dot = sum q_fixed * x_fixed,
  key = float64(dot) * (1 / sqrt(float64(norm2))), order (key desc, ordinal asc),
  score = float32(key * (1 / sqrt(float64(q_norm2)))).

Everything is compared bit for bit (the sign of a zero key included).
"""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adversarial as adv  # noqa: E402

N, NQ, K, BASE, SEED = 850, 10, 240, 1000, 5


def _fixed(u16: np.ndarray) -> np.ndarray:
    x = u16.view(np.float16).astype(np.float64) * 2.0 ** 24
    ok = np.isfinite(x)
    out = np.where(ok, x, 0.0).astype(np.int64)
    assert (out[ok] == x[ok]).all()  # every finite fp16 is an integer multiple of 2^-24
    return out


def _inv_sqrt(n2: np.ndarray) -> np.ndarray:
    inv = np.zeros(n2.shape, dtype=np.float64)
    inv[n2 > 0] = 1.0 / np.sqrt(n2[n2 > 0].astype(np.float64))
    return inv


def _numpy_reference(rows, qs):
    """(norm2 with -1 for invalid rows, inv_norm, keys float64 [nq, n], inv_q)."""
    valid = adv.valid_rows(rows)
    xf, qf = _fixed(rows), _fixed(qs)
    norm2 = np.where(valid, (xf * xf).sum(axis=1), -1)
    inv = _inv_sqrt(norm2)
    dot = qf @ xf.T
    assert dot.dtype == np.int64
    return norm2, inv, dot.astype(np.float64) * inv[None, :], _inv_sqrt((qf * qf).sum(axis=1))


@pytest.fixture(scope="module", params=[256, 1024])
def case(request, oracle_mod):
    dim = request.param
    rows = adv.corpus(dim, N, SEED)
    qs = adv.queries(dim, NQ, rows, SEED)
    return dim, rows, qs, adv.labels(dim, N, SEED)


def test_corpus_is_deterministic_and_holds_every_class(case):
    dim, rows, qs, lab = case
    np.testing.assert_array_equal(rows, adv.corpus(dim, N, SEED))
    np.testing.assert_array_equal(qs, adv.queries(dim, NQ, rows, SEED))
    np.testing.assert_array_equal(adv.queries(dim, 37, rows, SEED)[:NQ], qs)
    want = dict(A=256, B=256, C1=64, C2=64, L=64, D=64, E=8, G=64, F=4, fill=N - adv.BLOCK_ROWS)
    for name, count in want.items():
        assert (lab == adv.LABELS.index(name)).sum() == count, name
    assert sorted(adv.query_kinds(NQ).tolist()) == list(range(len(adv.KINDS)))
    exp = (rows >> 10) & 31
    c2 = rows[lab == adv.LABELS.index("C2")]
    assert (((c2 >> 10) & 31) == 0).all() and ((c2 & 0x3FF) != 0).all()
    c1 = exp[lab == adv.LABELS.index("C1")]
    assert (c1 == 0).mean() > 0.5  # mostly subnormal
    # every 32-row tile of the block-sized corpus mixes classes
    for t in range(0, N - 31, 32):
        assert len(np.unique(lab[t:t + 32])) >= 3
    assert ((((qs >> 10) & 31) <= 15).all())  # queries stay in the row domain


def test_row_norms_match_numpy_and_flag_the_invalid_rows(case, oracle_mod):
    dim, rows, qs, lab = case
    norm2, inv, _, _ = _numpy_reference(rows, qs)
    o2, oinv = oracle_mod.row_norms(rows, dim)
    np.testing.assert_array_equal(o2, norm2)
    np.testing.assert_array_equal(oinv.view(np.uint64), inv.view(np.uint64))
    np.testing.assert_array_equal(np.nonzero(o2 < 0)[0], np.nonzero(lab == adv.LABELS.index("F"))[0])
    assert (o2 < 0).sum() == 4
    np.testing.assert_array_equal(np.nonzero(o2 == 0)[0], np.nonzero(lab == adv.LABELS.index("E"))[0])
    assert (o2 == 0).sum() == 8 and (oinv[o2 == 0] == 0).all()


def test_dense_topk_matches_numpy_bitwise(case, oracle_mod):
    dim, rows, qs, lab = case
    norm2, _, keys, inv_q = _numpy_reference(rows, qs)
    ref = oracle_mod.dense_topk(rows, qs, K, ordinal_base=BASE)
    live = np.nonzero(norm2 >= 0)[0]
    assert (ref.count == K).all()
    for b in range(NQ):
        kb = keys[b, live]
        order = np.lexsort((live, -kb))[:K]  # key descending, then ordinal ascending
        np.testing.assert_array_equal(ref.ids[b], BASE + live[order], err_msg=f"query {b}")
        np.testing.assert_array_equal(ref.rank[b].view(np.uint64), kb[order].view(np.uint64),
                                      err_msg=f"query {b}")
        score = (kb[order] * inv_q[b]).astype(np.float32)
        np.testing.assert_array_equal(ref.scores[b].view(np.uint32), score.view(np.uint32),
                                      err_msg=f"query {b}")
    assert not np.isin(ref.ids - BASE, np.nonzero(lab == adv.LABELS.index("F"))[0]).any()


def test_power_of_two_multiples_tie_bitwise(case, oracle_mod):
    """The tie premise of class B: for every query, each multiple's key has the bits of its 2^0
    original's key, through the oracle's own key routine and through numpy."""
    dim, rows, qs, lab = case
    block_rows, _ = adv.block(dim, SEED)
    where = np.argsort(adv.permutation(N, SEED))  # block row j sits at corpus row where[j]
    np.testing.assert_array_equal(rows[where[:adv.BLOCK_ROWS]], block_rows)
    _, _, keys, _ = _numpy_reference(rows, qs)
    originals = where[256 + 3 * 64:256 + 4 * 64]  # the 2^0 copies
    np.testing.assert_array_equal(rows[originals], rows[where[:64]])
    for b in range(NQ):
        want, _ = oracle_mod.dense_keys(rows, qs[b], originals)
        np.testing.assert_array_equal(want.view(np.uint64), keys[b, originals].view(np.uint64))
        for m in range(3):
            mult = where[256 + m * 64:256 + (m + 1) * 64]
            assert (rows[mult] != rows[originals]).any(axis=1).all()
            got, _ = oracle_mod.dense_keys(rows, qs[b], mult)
            np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64),
                                          err_msg=f"query {b} multiple {m}")
            np.testing.assert_array_equal(keys[b, mult].view(np.uint64), want.view(np.uint64))


def test_top_lists_hold_exact_ties_in_ordinal_order(case, oracle_mod):
    """What the GPU tests rely on: the top 240 of every non-zero query holds exact key ties, and the
    zero queries tie everywhere (ascending ordinals)."""
    dim, rows, qs, lab = case
    ref = oracle_mod.dense_topk(rows, qs, K)
    kinds = adv.query_kinds(NQ)
    for b in range(NQ):
        tied = ref.rank[b, 1:] == ref.rank[b, :-1]
        assert (ref.ids[b, 1:][tied] > ref.ids[b, :-1][tied]).all()
        if adv.KINDS[kinds[b]] in ("zero", "neg_zero"):
            assert tied.all() and (ref.rank[b] == 0).all()
        else:
            assert tied.sum() >= 20, (b, tied.sum())
