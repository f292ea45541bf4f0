"""Every sparse search path on the adversarial corpus of tests/sparse_adversarial.py (rows that
share an index with the query and score exactly 0), against the CPU oracle: the MFMA filter at its
default (on), the exact scan alone, row lists, the live tail on both of its passes, two shards
merged, and the sorted term numbering of a large vocabulary.

include/armi.h's rule is one ranking whichever kernel answers: a row is a result when it shares an
index with the query, also with score 0, ordered (score desc, ordinal asc). So on every path ids,
counts and score BIT PATTERNS (the sums start from +0.0f: a returned -0.0 is a difference) equal
oracle.sparse_topk, and the ids past the count are -1. k = 5 answers with positive rows only, k = 20
ends inside the block of zero-score rows, k = 64 and 128 want more rows than share an index, k = 240
is above the filter's limit; each with and without a row mask that keeps half of every class.
test_sparse_adversarial_cpu.py pins those expectations.

Two conditions keep the filter honest rather than absent: whenever a query is flagged FILTERED its
answer equals the oracle's (asserted per query), and the ordinary queries whose top-k is full and
positive are FILTERED on this index at least as often as on its twin without the zero postings.
"""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sparse_adversarial as sadv  # noqa: E402

pytestmark = pytest.mark.gpu

N, SEED, BASE, KS = sadv.N, sadv.SEED, sadv.BASE, sadv.KS
FILTER_KS = tuple(k for k in KS if k <= 128)  # the filter's k limit
VOCAB, BIG_VOCAB = 250002, 1 << 20
MAIN, SHARD = 2000, 1500
FILTERED = 4
CASES = [(k, m) for k in KS for m in (False, True)]


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _np(out, fields=("ids", "scores", "count", "flags")):
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in fields if getattr(out, f) is not None}


def _mask(ok, gpu):
    return _dev(sadv.bits(ok).view(np.int64), gpu)


class Case:
    def __init__(self, gpu, oracle_mod):
        from audio_rag_amd.retrieval.device import SparseIndex

        self.gpu, self.oracle = gpu, oracle_mod
        self.csr, self.terms, self.lab = sadv.corpus(N, SEED)
        self.q, self.kinds = sadv.queries(self.terms, sadv.N_ORDINARY, SEED)
        self.ok = sadv.keep_half(self.lab, SEED)
        self.dq = tuple(_dev(a, gpu) for a in self.q)
        self.nq = len(self.q[0]) - 1
        self.index = lambda csr, base, vocab=VOCAB: SparseIndex(*(_dev(a, gpu) for a in csr), vocab, base)
        self.idx = self.index(self.csr, BASE)
        self._refs, self._on = {}, {}

    def ref(self, k, masked):
        if (k, masked) not in self._refs:
            self._refs[(k, masked)] = self.oracle.sparse_topk(
                *self.csr, *self.q, k, row_mask=sadv.bits(self.ok) if masked else None,
                ordinal_base=BASE)
        return self._refs[(k, masked)]

    def run(self, idx, k, ok=None):
        return _np(idx.topk(*self.dq, k, row_mask=None if ok is None else _mask(ok, self.gpu)))

    def filter_on(self, k, masked):
        if (k, masked) not in self._on:
            assert self.idx.set_filter(True)  # usable: -0.0 is no negative value
            self._on[(k, masked)] = self.run(self.idx, k, self.ok if masked else None)
        return self._on[(k, masked)]


@pytest.fixture(scope="module")
def case(gpu, oracle_mod):
    return Case(gpu, oracle_mod)


def _same(got, ref, kinds, what):
    """ids, counts and score bits of every query equal the oracle's; -1 past the count."""
    flags = got.get("flags")
    for b in range(ref.count.shape[0]):
        c = int(ref.count[b])
        msg = (f"{what}: query {b} ({sadv.KINDS[kinds[b]]})"
               + ("" if flags is None else f", flags {int(flags[b])}"
                  f"{' FILTERED' if flags[b] & FILTERED else ''}"))
        assert int(got["count"][b]) == c, f"{msg}: count {int(got['count'][b])}, oracle {c}"
        np.testing.assert_array_equal(got["ids"][b, :c], ref.ids[b, :c], err_msg=msg)
        np.testing.assert_array_equal(got["scores"][b, :c].view(np.uint32),
                                      ref.scores[b, :c].view(np.uint32), err_msg=msg)
        assert (got["ids"][b, c:] == -1).all(), msg


# ------------------------------------------------------------------------- the filter, on and off

@pytest.mark.parametrize("k,masked", CASES)
def test_filter_on_equals_oracle(case, k, masked):
    """SparseIndex.topk as it comes (the MFMA filter on). A query flagged FILTERED was answered by
    the filter's certificate: _same names the flag of any query that differs."""
    got = case.filter_on(k, masked)
    ref = case.ref(k, masked)
    _same(got, ref, case.kinds, f"filter on, k {k}, mask {masked}")
    if k > 128:
        assert not (got["flags"] & FILTERED).any()
    if k == 64 and not masked:  # hot_only: more results than positive rows (not vacuous)
        assert got["count"][2] > (ref.scores[2, :ref.count[2]] > 0).sum() > 0


@pytest.mark.parametrize("k,masked", CASES)
def test_filter_off_equals_oracle_and_filter_on(case, k, masked):
    on = case.filter_on(k, masked)
    try:
        case.idx.set_filter(False)
        off = case.run(case.idx, k, case.ok if masked else None)
    finally:
        case.idx.set_filter(True)
    assert not (off["flags"] & FILTERED).any()
    _same(off, case.ref(k, masked), case.kinds, f"filter off, k {k}, mask {masked}")
    for f in ("count", "ids"):
        np.testing.assert_array_equal(on[f], off[f], err_msg=f)
    np.testing.assert_array_equal(on["scores"].view(np.uint32), off["scores"].view(np.uint32))


@pytest.mark.parametrize("k,masked", [(k, m) for k in FILTER_KS for m in (False, True)])
def test_sorted_term_numbering_equals_oracle(case, k, masked):
    """vocab = 2^20: the pass numbers its terms by sorting instead of the bitmap. The special ids
    sit above 2^18 after an order-preserving move, which leaves every sum's order, and so the
    oracle's answer, unchanged."""
    if not hasattr(case, "big"):
        ip, ix, iv = case.csr
        case.big = case.index((ip, sadv.move_terms(ix), iv), BASE, BIG_VOCAB)
        case.big_q = (case.dq[0], _dev(sadv.move_terms(case.q[1]), case.gpu), case.dq[2])
        assert min(case.terms.values()) + 300000 >= 1 << 18
    assert case.big.set_filter(True)
    m = _mask(case.ok, case.gpu) if masked else None
    got = _np(case.big.topk(*case.big_q, k, row_mask=m))
    _same(got, case.ref(k, masked), case.kinds, f"vocab 2^20, k {k}, mask {masked}")


def test_filter_still_answers_where_it_can(case):
    """The ordinary queries whose oracle top-k is full and all positive need no zero-score row: the
    filter must certify them on this index at least as often as on the twin index (the same rows
    without the zero-valued postings), same queries, same pass. The twin's answers for them are the
    same lists. No fraction is fixed in advance, but the twin must certify some query at k = 5 (an
    index without zeros and positive weights is what the filter was built for), or the comparison
    would be empty."""
    twin = case.index(sadv.twin(case.csr), BASE)
    assert twin.set_filter(True)
    for k in FILTER_KS:
        for masked in (False, True):
            ref = case.ref(k, masked)
            sel = np.nonzero((case.kinds == sadv.KINDS.index("ordinary")) & (ref.count == k)
                             & (ref.scores[:, -1] > 0))[0]
            assert sel.size >= 10, (k, masked, sel.size)
            adv = case.filter_on(k, masked)
            tw = case.run(twin, k, case.ok if masked else None)
            for b in sel:
                np.testing.assert_array_equal(tw["ids"][b], ref.ids[b], err_msg=f"twin, query {b}")
                np.testing.assert_array_equal(tw["scores"][b].view(np.uint32),
                                              ref.scores[b].view(np.uint32))
            f_adv = ((adv["flags"][sel] & FILTERED) != 0).mean()
            f_twin = ((tw["flags"][sel] & FILTERED) != 0).mean()
            print(f"k {k} mask {masked}: FILTERED {f_adv:.2f} of {sel.size} queries, twin {f_twin:.2f}")
            assert f_adv >= f_twin, (k, masked, f_adv, f_twin)
            if k == 5 and not masked:
                assert f_twin > 0
    twin.close()


# -------------------------------------------------------------------------------- row lists

@pytest.mark.parametrize("k", KS)
def test_row_lists_equal_oracle(case, k):
    """topk_rows with a list of every row the mask enables and a list of all rows."""
    lists = [np.nonzero(case.ok)[0].astype(np.int32), np.arange(N, dtype=np.int32)]
    ptr = _dev(np.array([0, len(lists[0]), len(lists[0]) + N], np.int64), case.gpu)
    rows = _dev(np.concatenate(lists), case.gpu)
    for l, masked in ((0, True), (1, False)):
        got = _np(case.idx.topk_rows(*case.dq, k, ptr, rows,
                                     _dev(np.full(case.nq, l, np.int32), case.gpu), N))
        _same(got, case.ref(k, masked), case.kinds, f"row list of {len(lists[l])} rows, k {k}")


# -------------------------------------------------------------------------------- live tail

@pytest.mark.parametrize("k,masked", CASES)
def test_live_tail_equals_oracle_over_the_whole_corpus(case, monkeypatch, k, masked):
    """Main segment = rows [0, 2000) (SparseIndex, filter on), tail = rows [2000, 3000) appended in
    two pieces; both segments hold rows of every class. The fused pass and ARMI_TAIL_PASS=general."""
    from audio_rag_amd.retrieval.device import TailSparseIndex

    if not hasattr(case, "main"):
        case.main = case.index(sadv.rows_range(case.csr, 0, MAIN), BASE)
        case.tail = TailSparseIndex(BASE + MAIN, case.gpu, vocab=VOCAB)
        for lo, hi in ((MAIN, MAIN + 300), (MAIN + 300, N)):
            case.tail.append(*(_dev(a, case.gpu) for a in sadv.rows_range(case.csr, lo, hi)))
        for name, _ in sadv.CLASSES:
            r = sadv.rows_of(case.lab, name)
            assert (r < MAIN).any() and (r >= MAIN).any(), name
    assert case.tail.n_rows == N - MAIN
    m_main = _mask(case.ok[:MAIN], case.gpu) if masked else None
    m_tail = _mask(case.ok[MAIN:], case.gpu) if masked else None
    main = case.main.topk(*case.dq, k, row_mask=m_main)
    for setting in (None, "general"):
        if setting is None:
            monkeypatch.delenv("ARMI_TAIL_PASS", raising=False)
        else:
            monkeypatch.setenv("ARMI_TAIL_PASS", setting)
        got = _np(case.tail.tail_topk(*case.dq, k, main, row_mask=m_tail))
        _same(got, case.ref(k, masked), case.kinds,
              f"tail pass {setting or 'fused'}, k {k}, mask {masked}")


# ----------------------------------------------------------------------------------- shards

@pytest.mark.parametrize("k,masked", CASES)
def test_two_shards_merged_equal_oracle(case, k, masked):
    from audio_rag_amd.retrieval.device import merge_shards

    if not hasattr(case, "shards"):
        case.shards = [case.index(sadv.rows_range(case.csr, lo, lo + SHARD), BASE + lo)
                       for lo in (0, SHARD)]
    outs = []
    for s, lo in zip(case.shards, (0, SHARD)):
        m = _mask(case.ok[lo:lo + SHARD], case.gpu) if masked else None
        outs.append(s.topk(*case.dq, k, row_mask=m))
    scores = torch.stack([o.scores for o in outs])
    merged = merge_shards(scores.double(), scores, torch.stack([o.ids for o in outs]),
                          torch.stack([o.count for o in outs]), k)
    _same(_np(merged), case.ref(k, masked), case.kinds, f"two shards, k {k}, mask {masked}")
