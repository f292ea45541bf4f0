"""The oracle on the adversarial sparse corpus of tests/sparse_adversarial.py (rows that share an
index with the query and score exactly 0: zero and -0.0 values, zero and -0.0 weights, a term whose
every posting is zero, products that underflow), before the GPU tests lean on it:

  * the expected answers are not vacuous: at k = 5 the zero query's answer is all positive, at
    k = 20 it mixes positive and zero-score rows, from k = 64 up it is shorter than k and holds
    rows of every zero-score class, the zero-score block in ascending ordinal order;
  * the C oracle equals a numpy merge join of the documented rule (include/armi.h: a row is a result
    when it shares an index, fp32 products added in ascending index order from +0.0f, order
    (score desc, ordinal asc)).

Scores are compared as bit patterns: the sums start from +0.0f, so a -0.0 would be a difference.
"""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sparse_adversarial as sadv  # noqa: E402

N, SEED, BASE, KS = sadv.N, sadv.SEED, sadv.BASE, sadv.KS
ZERO_CLASSES = ("ZV", "NZ", "ZW", "AZ", "UF")


@pytest.fixture(scope="module")
def case(oracle_mod):
    csr, terms, lab = sadv.corpus(N, SEED)
    q, kinds = sadv.queries(terms, sadv.N_ORDINARY, SEED)
    return csr, terms, lab, q, kinds, sadv.keep_half(lab, SEED)


_refs = {}


def _ref(oracle_mod, case, k, masked):
    if (k, masked) not in _refs:
        csr, _, _, q, _, ok = case
        _refs[(k, masked)] = oracle_mod.sparse_topk(
            *csr, *q, k, row_mask=sadv.bits(ok) if masked else None, ordinal_base=BASE)
    return _refs[(k, masked)]


def test_corpus_is_deterministic_and_holds_every_class(case):
    csr, terms, lab, q, kinds, ok = case
    again, terms2, lab2 = sadv.corpus(N, SEED)
    for a, b in zip(csr, again):
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b)
    assert terms == terms2 and (lab == lab2).all()
    base = sadv.oracle.sparse_corpus(N, seed=SEED)
    assert not np.isin(list(terms.values()), base[1]).any()  # fresh ids
    assert sorted(terms.values()) == [terms[t] for t in sadv.TERM_NAMES]
    assert min(terms.values()) >= sadv.FIRST_FRESH and max(terms.values()) < sadv.oracle.VOCAB
    ip, ix, iv = csr
    assert (np.diff(ix)[np.diff(np.repeat(np.arange(N), np.diff(ip))) == 0] > 0).all()  # ascending
    assert (iv >= 0).all()  # (-0.0 >= 0: no negative value, so the MFMA filter stays usable)
    for name, count in sadv.CLASSES:
        rows = sadv.rows_of(lab, name)
        assert rows.size == count, name
        kept = ok[rows].sum()
        assert kept == (count + 1) // 2 and kept < count, name  # the mask splits every class
        # rows of every class on both sides of the main / tail and the shard cuts
        assert (rows < 1500).any() and (rows >= 2000).any(), name
        assert (rows[ok[rows]] < 2000).any(), name
    assert np.signbit(iv).sum() == 6 and ((iv == 0).sum() == 12 + 6 + 6)
    az = iv[ix == terms["az"]]
    assert az.size == 6 and (az == 0).all()  # the all-zero term
    # row ranges of 64 rows: the class rows spread over many of them
    assert np.unique(np.nonzero(lab < len(sadv.CLASSES))[0] // 64).size >= 25
    tw = sadv.twin(csr)
    assert (tw[2] > 0).all() and tw[2].size == iv.size - 24 and len(tw[0]) == N + 1
    assert kinds.tolist() == [0, 1, 2, 3] + [4] * sadv.N_ORDINARY
    qi, qx, qv = q
    assert np.signbit(qv[qi[1]:qi[2]]).sum() == 1 and (qv[qi[0]:qi[1]] == 0).sum() == 1
    assert (qv[qi[3]:qi[4]] > 0).all() and qv[qi[3]:qi[4]].max() < 1e-37
    assert len(qi) - 1 <= 64  # one pass: the tiny query shares it with ordinary queries


def test_zero_query_answers_are_not_vacuous(case, oracle_mod):
    csr, terms, lab, q, kinds, ok = case
    for masked in (False, True):
        wide = _ref(oracle_mod, case, 240, masked)
        for b in (0, 1):  # zero, zero_negw
            c = wide.count[b]
            assert c < 64
            positives = int((wide.scores[b, :c] > 0).sum())
            live = ok if masked else np.ones(N, dtype=bool)
            n_uf = int(live[sadv.rows_of(lab, "UF")].sum())
            # (the wrong-ids case needs k = 20 inside the zero block with more zero rows behind it;
            # the short-count case needs fewer than 64 rows with a positive key)
            if not masked:
                assert positives + n_uf >= 20 and positives + n_uf < 64
            assert positives < 20 < c
            r5 = _ref(oracle_mod, case, 5, masked)
            assert r5.count[b] == 5 and (r5.scores[b] > 0).all()
            r20 = _ref(oracle_mod, case, 20, masked)
            assert r20.count[b] == 20
            assert (r20.scores[b] == 0).sum() >= 2 and (r20.scores[b] > 0).sum() >= 2
            for k in (64, 128, 240):
                r = _ref(oracle_mod, case, k, masked)
                assert r.count[b] == c < k
                got = r.ids[b, :c] - BASE
                assert (r.ids[b, c:] == -1).all()
                for name in ZERO_CLASSES:
                    assert np.isin(sadv.rows_of(lab, name), got).any(), (name, k, masked)
                zero = got[r.scores[b, :c] == 0]
                assert zero.size == c - positives and (np.diff(zero) > 0).all()
                assert (r.scores[b, :c].view(np.uint32) >> 31 == 0).all()  # no -0.0, no negative


def test_hot_only_query_returns_more_than_its_positive_rows(case, oracle_mod):
    """Only P, PL, ZV and NZ rows share the hot term: 11 positive rows and 18 with score +0.0."""
    csr, terms, lab, q, kinds, ok = case
    r = _ref(oracle_mod, case, 64, False)
    c = r.count[2]
    assert c == 7 + 4 + 12 + 6 and (r.scores[2, :c] > 0).sum() == 11
    np.testing.assert_array_equal(
        np.sort(r.ids[2, :c] - BASE),
        np.sort(np.concatenate([sadv.rows_of(lab, n) for n in ("P", "PL", "ZV", "NZ")])))


def test_ordinary_queries_have_full_positive_lists(case, oracle_mod):
    """What the GPU tests' filter-coverage condition selects on."""
    kinds = case[4]
    for k in KS:
        r = _ref(oracle_mod, case, k, False)
        full = (r.count == k) & (r.scores[:, -1] > 0) & (kinds == 4)
        assert full.sum() >= 15, (k, full.sum())


@pytest.mark.parametrize("masked", [False, True])
def test_oracle_matches_numpy_merge_join_bitwise(case, oracle_mod, masked):
    csr, terms, lab, q, kinds, ok = case
    want = sadv.numpy_topk(csr, q, 240, ok if masked else None, BASE)
    ref = _ref(oracle_mod, case, 240, masked)
    for b, (ids, scores) in enumerate(want):
        c = ref.count[b]
        assert c == ids.size, b
        np.testing.assert_array_equal(ref.ids[b, :c], ids, err_msg=f"query {b}")
        np.testing.assert_array_equal(ref.scores[b, :c].view(np.uint32), scores.view(np.uint32),
                                      err_msg=f"query {b}")
    # the twin corpus (zero postings removed) loses exactly the rows whose every shared posting
    # was zero; the rows it keeps score the same
    tw = sadv.numpy_topk(sadv.twin(csr), q, 240, ok if masked else None, BASE)
    for b in (0, 2):
        gone = np.setdiff1d(want[b][0], tw[b][0]) - BASE
        assert gone.size and np.isin(lab[gone], [sadv.LABELS.index(n) for n in ("ZV", "NZ", "AZ")]).all()
