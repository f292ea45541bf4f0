"""Every dense search path on adversarial rows (tests/adversarial.py: subnormal rows, exact
power-of-two multiples, spikes that quantise to a one-hot int8 image, zero rows, one-ulp neighbours,
invalid rows) at all four dims the kernels are instantiated for, against the CPU oracle.

Parity bar, as everywhere in the dense suite: counts, ids, fp64 rank keys and fp32 scores equal
oracle.dense_topk bit for bit, ids past the count are -1, no invalid ordinal is ever returned.
Every cell asserts the scan form it names first. Each cell also appends the fraction of queries it
answered CERTIFIED (unit-kind queries and the others apart) to bench_out/dense_adversarial_cert.txt
(the ignored directory the tools/ scripts write their output to):
a report, not an assertion (the zero queries and the tie piles take the exact second pass by design).

Measured on an MI355X (certified unit-kind queries, certified others; the same at every dim unless
noted; a range spans the dims; except at k = 240 the uncertified "others" are mostly the zero queries):
  INT8_FILTER (7,5) 1/1 4/6, (64,64) 21-22/22 39-40/42, (100,40) 36-37/37 61/63; masked (16,5) 4/4 10/12
  FP16 (16,65) 4/4 10/12, (64,65) 22/22 40/42, (70,128) 25/25 41-43/45, (70,240) 17-18/25 22-30/45
  TILED_FP16 (130,5) 49/49 78-79/81 (masked too), TILED_INT8 (130, 1 and 5) 49/49 79/81
  tail fused pass (7,5) (7,240) 1/1 4/6, (70,5) (70,240) 25/25 43/45
  FP16 (16,240) and TILED_FP16 (300,100): no query certifies. 4099 rows give 17 workgroup lists (33
  row ranges) of 16 candidates, whose 17th-best bounds lie above the global k-th key: these two cells
  test the exact second pass only; the fp16 scan's own k = 240 answer is tested by FP16 (70,240).
"""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adversarial as adv  # noqa: E402

pytestmark = pytest.mark.gpu

N, BASE, SEED, NQ_MAX = 4099, 1000, 5, 300   # 129 tiles of 32 rows, the last one partial
DIMS = (256, 512, 768, 1024)
MAIN = 3000                                  # live tail: rows [MAIN, N) are appended
REPORT = Path(__file__).resolve().parent.parent / "bench_out" / "dense_adversarial_cert.txt"


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _np(out, fields=("ids", "scores", "rank", "count", "flags")):
    torch.cuda.synchronize()
    return {f: getattr(out, f).cpu().numpy() for f in fields}


def _assert_same(got, ref, invalid=()):
    np.testing.assert_array_equal(got["count"], ref.count)
    for b in range(ref.count.shape[0]):
        c = ref.count[b]
        np.testing.assert_array_equal(got["ids"][b, :c], ref.ids[b, :c], err_msg=f"query {b}")
        # bit patterns, so that the sign of a zero key (a zero row under a negative dot) counts too
        np.testing.assert_array_equal(got["rank"][b, :c].view(np.uint64),
                                      ref.rank[b, :c].view(np.uint64), err_msg=f"rank, query {b}")
        np.testing.assert_array_equal(got["scores"][b, :c].view(np.uint32),
                                      ref.scores[b, :c].view(np.uint32), err_msg=f"scores, query {b}")
        assert (got["ids"][b, c:] == -1).all()
    assert not np.isin(got["ids"], invalid).any()


def _report(dim, form, nq, k, flags, kinds, bit=None):
    """One line per cell: the fraction of queries flagged CERTIFIED (or `bit`), unit kind / rest."""
    from audio_rag_amd import _armi

    bit = _armi.ARMI_FLAG_CERTIFIED if bit is None else bit
    hit = (flags & bit) != 0
    unit = kinds[:nq] == adv.UNIT_KIND
    REPORT.parent.mkdir(exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(f"dim={dim} form={form} nq={nq} k={k} certified_unit={hit[unit].mean():.3f} "
                f"({int(hit[unit].sum())}/{int(unit.sum())}) certified_other={hit[~unit].mean():.3f} "
                f"({int(hit[~unit].sum())}/{int((~unit).sum())})\n")


def _assert_answered(flags):
    from audio_rag_amd import _armi

    assert ((flags & (_armi.ARMI_FLAG_CERTIFIED | _armi.ARMI_FLAG_FALLBACK)) != 0).all(), flags


class _Ctx:
    def __init__(self, dim, gpu, oracle_mod):
        from audio_rag_amd.retrieval.device import DenseIndex

        self.dim, self.gpu, self.oracle = dim, gpu, oracle_mod
        self.rows = adv.corpus(dim, N, SEED)
        self.lab = adv.labels(dim, N, SEED)
        self.qs = adv.queries(dim, NQ_MAX, self.rows, SEED, among=self.lab != adv.LABELS.index("fill"))
        self.kinds = adv.query_kinds(NQ_MAX)
        self.invalid = BASE + np.nonzero(self.lab == adv.LABELS.index("F"))[0]
        self.idx = DenseIndex(_dev(self.rows.view(np.float16), gpu), ordinal_base=BASE)
        self.keep = np.random.default_rng(3).random(N) < 0.4
        self.mask = adv.mask_words(self.keep)
        self.mask_dev = _dev(self.mask.view(np.int64), gpu)
        self._refs = {}

    def q(self, nq):
        return _dev(self.qs[:nq].view(np.float16), self.gpu)

    def ref(self, nq, k, masked=False):
        """The oracle's answer, computed once per (nq, k, masked) and shared."""
        key = (nq, k, masked)
        if key not in self._refs:
            self._refs[key] = self.oracle.dense_topk(self.rows, self.qs[:nq], k, ordinal_base=BASE,
                                                     row_mask=self.mask if masked else None)
        return self._refs[key]


_ctxs = {}


@pytest.fixture(scope="module")
def ctx(gpu, oracle_mod):
    def get(dim):
        if dim not in _ctxs:
            _ctxs[dim] = _Ctx(dim, gpu, oracle_mod)
        return _ctxs[dim]

    yield get
    for c in _ctxs.values():
        c.idx.close()
    _ctxs.clear()


def _forms():
    from audio_rag_amd import _armi

    return {"INT8_FILTER": _armi.SCAN_INT8_FILTER, "FP16": _armi.SCAN_FP16,
            "TILED_FP16": _armi.SCAN_TILED_FP16, "TILED_INT8": _armi.SCAN_TILED_INT8}


# ------------------------------------------------------------------------------ index build

@pytest.mark.parametrize("dim", DIMS)
def test_norms_and_invalid_rows(ctx, oracle_mod, dim):
    """row_norm_kernel on subnormal, zero, spike and invalid rows: norm2 / inv_norm / inv_norm32
    equal the oracle's, 4 rows are counted invalid, the 8 zero rows have inv_norm 0."""
    c = ctx(dim)
    assert c.idx.invalid_rows() == 4
    n2, inv, inv32 = (t.cpu().numpy() for t in c.idx.norms())
    o2, oinv = oracle_mod.row_norms(c.rows, dim)
    ok = o2 >= 0
    assert (~ok).sum() == 4 and (o2 == 0).sum() == 8
    np.testing.assert_array_equal(n2 >= 0, ok)
    np.testing.assert_array_equal(n2[ok], o2[ok])
    np.testing.assert_array_equal(inv[ok], oinv[ok])
    np.testing.assert_array_equal(inv32[ok], (oinv[ok] * 2.0 ** 24).astype(np.float32))
    assert (inv[o2 == 0] == 0).all()


# ------------------------------------------------------------------------------- scan forms

CELLS = [("INT8_FILTER", 7, 5), ("INT8_FILTER", 64, 64), ("INT8_FILTER", 100, 40),
         ("FP16", 16, 65), ("FP16", 16, 240), ("TILED_FP16", 130, 5), ("TILED_FP16", 300, 100),
         # the fp16 scan with a full 64-query block (the XCD-grouped two-block form at nq = 70): at
         # dim 256 its workgroup merge scratch is larger than the query image it overlays
         ("FP16", 64, 65), ("FP16", 70, 128), ("FP16", 70, 240)]


@pytest.mark.parametrize("form,nq,k", CELLS)
@pytest.mark.parametrize("dim", DIMS)
def test_scan_form_matches_oracle(ctx, dim, form, nq, k):
    c = ctx(dim)
    assert c.idx.scan_form(nq, k) == _forms()[form]
    ref = c.ref(nq, k)
    for _ in range(2):  # consecutive calls scan in opposite directions
        got = _np(c.idx.topk(c.q(nq), k))
        _assert_same(got, ref, c.invalid)
        _assert_answered(got["flags"])
    _report(dim, form, nq, k, got["flags"], c.kinds)


@pytest.mark.parametrize("dim", DIMS)
def test_exact_entry_point_matches_oracle(ctx, dim):
    c = ctx(dim)
    got = _np(c.idx.topk(c.q(16), 33, exact=True))
    _assert_same(got, c.ref(16, 33), c.invalid)
    _assert_answered(got["flags"])
    _report(dim, "EXACT", 16, 33, got["flags"], c.kinds)


MASKED = [("INT8_FILTER", 16, 5, False), ("FP16", 16, 65, False), ("TILED_FP16", 130, 5, False),
          ("EXACT", 16, 5, True), ("EXACT", 130, 5, True),
          # two 64-query blocks: the XCD-grouped workgroup mapping together with the row mask
          ("INT8_FILTER", 100, 40, False), ("FP16", 70, 128, False)]


@pytest.mark.parametrize("form,nq,k,exact", MASKED)
@pytest.mark.parametrize("dim", DIMS)
def test_row_mask_matches_oracle(ctx, dim, form, nq, k, exact):
    """A 40 % random row filter on every scan form and on the exact entry point."""
    c = ctx(dim)
    if not exact:
        assert c.idx.scan_form(nq, k) == _forms()[form]
    got = _np(c.idx.topk(c.q(nq), k, row_mask=c.mask_dev, exact=exact))
    _assert_same(got, c.ref(nq, k, masked=True), c.invalid)
    _assert_answered(got["flags"])
    ids = got["ids"][got["ids"] >= 0] - BASE
    assert c.keep[ids].all()
    _report(dim, form + "+mask", nq, k, got["flags"], c.kinds)


# -------------------------------------------------------------------------------- row lists

@pytest.mark.parametrize("k", [5, 240])
@pytest.mark.parametrize("dim", DIMS)
def test_row_lists_match_oracle(ctx, oracle_mod, gpu, dim, k):
    """topk_rows over an empty list, a 37-row list and a 1500-row list (three 512-row chunks: the
    merge kernel runs); the long list holds every invalid and every zero row."""
    from audio_rag_amd import _armi

    c = ctx(dim)
    rng = np.random.default_rng(11)
    special = np.nonzero(np.isin(c.lab, [adv.LABELS.index("F"), adv.LABELS.index("E")]))[0]
    long = np.unique(np.concatenate([rng.choice(N, size=1500 - len(special), replace=False), special]))
    long = np.unique(np.concatenate([long, rng.choice(np.setdiff1d(np.arange(N), long),
                                                      size=1500 - len(long), replace=False)]))
    lists = [np.zeros(0, dtype=np.int64), np.sort(rng.choice(N, size=37, replace=False)), long]
    assert [len(x) for x in lists] == [0, 37, 1500]
    ptr = np.zeros(4, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    nq = 16
    q_list = (np.arange(nq) % 3).astype(np.int32)
    got = _np(c.idx.topk_rows(c.q(nq), k, _dev(ptr, gpu),
                              _dev(np.concatenate(lists).astype(np.int32), gpu), _dev(q_list, gpu), 1500))
    assert (got["flags"] == _armi.ARMI_FLAG_ROWLIST).all()
    for l, rows_l in enumerate(lists):
        sel = np.nonzero(q_list == l)[0]
        ok = np.zeros(N, dtype=bool)
        ok[rows_l] = True
        ref = oracle_mod.dense_topk(c.rows, c.qs[sel], k, row_mask=adv.mask_words(ok),
                                    ordinal_base=BASE)
        assert (ref.count == min(k, int((ok & (c.lab != adv.LABELS.index("F"))).sum()))).all()
        _assert_same({f: got[f][sel] for f in ("ids", "scores", "rank", "count")}, ref, c.invalid)
    _report(dim, "ROWLIST", nq, k, got["flags"], c.kinds, bit=_armi.ARMI_FLAG_ROWLIST)


# -------------------------------------------------------------------------------- live tail

@pytest.fixture(scope="module")
def tails(ctx, gpu):
    """dim -> (DenseIndex over rows [0, MAIN), TailIndex holding rows [MAIN, N) appended in pieces of
    1, 31, 33 and the rest)."""
    from audio_rag_amd.retrieval.device import DenseIndex, TailIndex

    made = {}

    def get(dim):
        if dim not in made:
            c = ctx(dim)
            main = DenseIndex(_dev(c.rows[:MAIN].view(np.float16), gpu), ordinal_base=BASE)
            tail = TailIndex(dim, N - MAIN, BASE + MAIN, gpu)
            at = MAIN
            for piece in (1, 31, 33, N - MAIN - 65):
                tail.append(_dev(c.rows[at:at + piece].view(np.float16), gpu))
                at += piece
            assert at == N and tail.n_rows == N - MAIN
            assert main.invalid_rows() + tail.invalid_rows() == 4
            made[dim] = (main, tail)
        return made[dim]

    yield get
    for main, tail in made.values():
        main.close()
        tail.close()


def _both_paths(monkeypatch, tail, q, k, main):
    monkeypatch.delenv("ARMI_TAIL_PASS", raising=False)
    fused = _np(tail.tail_topk(q, k, main))
    monkeypatch.setenv("ARMI_TAIL_PASS", "general")
    general = _np(tail.tail_topk(q, k, main))
    monkeypatch.delenv("ARMI_TAIL_PASS")
    return fused, general


@pytest.mark.parametrize("nq,k", [(7, 5), (7, 240), (70, 5), (70, 240)])
@pytest.mark.parametrize("dim", DIMS)
def test_live_tail_matches_oracle_over_all_rows(ctx, tails, monkeypatch, dim, nq, k):
    """The fused tail pass (dense_tail_scan_kernel / dense_tail_finish_kernel) and the general pass
    extend the main index's list by the appended rows: both equal the oracle over all 4099 rows."""
    c = ctx(dim)
    main, tail = tails(dim)
    q = c.q(nq)
    fused, general = _both_paths(monkeypatch, tail, q, k, main.topk(q, k))
    ref = c.ref(nq, k)
    _assert_same(fused, ref, c.invalid)
    _assert_same(general, ref, c.invalid)
    _assert_answered(fused["flags"])
    _assert_answered(general["flags"])
    _report(dim, "TAIL_FUSED", nq, k, fused["flags"], c.kinds)
    _report(dim, "TAIL_GENERAL", nq, k, general["flags"], c.kinds)


# ------------------------------------------------------------------------------- tiled int8

BIG_N, BIG_NQ, BIG_BASE = 200_011, 130, 1_000_000
BIG_SAMPLE = [0, 2, 4, 5, 7, 9, 64, 129]


@pytest.fixture(scope="module", params=[256, 768])
def big(request, gpu):
    """The adversarial block and make_rows filler, scattered by adversarial.permutation, at the
    smallest size that takes the int8 x int8 tiled scan."""
    from audio_rag_amd.retrieval.device import DenseIndex
    from audio_rag_amd.synthetic import make_rows

    dim = request.param
    blk, lab = adv.block(dim, SEED)
    rows = torch.cat([_dev(blk.view(np.float16), gpu),
                      make_rows(0, BIG_N - adv.BLOCK_ROWS, dim, gpu, seed=7)])
    perm = adv.permutation(BIG_N, SEED)
    rows = rows[_dev(perm, gpu)].contiguous()
    idx = DenseIndex(rows, ordinal_base=BIG_BASE)
    assert idx.invalid_rows() == 4
    qs = adv.queries(dim, BIG_NQ, blk, SEED)  # row copies come from the block
    where = np.argsort(perm)[:adv.BLOCK_ROWS]
    invalid = BIG_BASE + where[lab == adv.LABELS.index("F")]
    torch.cuda.synchronize()
    yield dict(dim=dim, idx=idx, rows=rows, qs=qs, invalid=invalid)
    idx.close()
    del rows
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [1, 5])
def test_tiled_int8_equals_exact_and_oracle(big, oracle_mod, gpu, k):
    from audio_rag_amd import _armi

    idx, dim = big["idx"], big["dim"]
    assert idx.scan_form(BIG_NQ, k) == _armi.SCAN_TILED_INT8
    q = _dev(big["qs"].view(np.float16), gpu)
    fast = _np(idx.topk(q, k))
    exact = _np(idx.topk(q, k, exact=True))
    for f in ("count", "ids", "rank", "scores"):
        np.testing.assert_array_equal(fast[f], exact[f], err_msg=f)
    _assert_answered(fast["flags"])
    assert not np.isin(fast["ids"], big["invalid"]).any()
    rows_u16 = big["rows"].cpu().numpy().view(np.uint16)
    want = oracle_mod.dense_topk(rows_u16, big["qs"][BIG_SAMPLE], k, ordinal_base=BIG_BASE)
    _assert_same({f: fast[f][BIG_SAMPLE] for f in ("ids", "scores", "rank", "count")}, want)
    _report(dim, "TILED_INT8", BIG_NQ, k, fast["flags"], adv.query_kinds(BIG_NQ))


# ------------------------------------------------------------------------------ shard merge

@pytest.mark.parametrize("dim", DIMS)
def test_three_shard_merge_equals_global_oracle(ctx, gpu, dim):
    """Shards cut at rows 1000 and 2777, k = 240 each: 720 pooled entries per query with exact key
    ties (the power-of-two multiples) across shards."""
    from audio_rag_amd.retrieval.device import DenseIndex, merge_shards

    c = ctx(dim)
    nq, k = 16, 240
    q = c.q(nq)
    parts, shards = [], []
    for a, b in ((0, 1000), (1000, 2777), (2777, N)):
        shards.append(DenseIndex(_dev(c.rows[a:b].view(np.float16), gpu), ordinal_base=BASE + a))
        parts.append(shards[-1].topk(q, k))
    stack = lambda f: torch.stack([getattr(p, f) for p in parts])  # noqa: E731
    m = merge_shards(stack("rank"), stack("scores"), stack("ids"), stack("count"), k)
    _assert_same(_np(m, ("ids", "scores", "rank", "count")), c.ref(nq, k), c.invalid)
    for s in shards:
        s.close()


def test_merge_at_the_pool_limit(gpu):
    """17 shards x k_in 240 = 4080 pooled entries (pool2 = 4096: merge_lists_kernel's largest, 98 KB
    LDS instance), k_out 240, ragged counts including 0, few distinct keys so that most ties cross
    shards, slots past a list's count poisoned. Reference: numpy sort by (key desc, ordinal asc)."""
    from audio_rag_amd.retrieval.device import merge_shards

    S, B, K_IN, K_OUT = 17, 6, 240, 240
    rng = np.random.default_rng(21)
    rank = np.full((S, B, K_IN), 1e300)
    ids = np.full((S, B, K_IN), 7, dtype=np.int64)       # poison past count: a winning entry
    scores = np.full((S, B, K_IN), 9.0, dtype=np.float32)
    count = rng.choice([0, 1, 17, 100, 239, 240], size=(S, B)).astype(np.int32)
    count[:, 0] = 240                                    # query 0: the full pool
    count[:, 1] = 0                                      # query 1: nothing at all
    count[:, 2] = (np.arange(S) == 4) * 3                # query 2: fewer than k_out in total
    want = []
    for b in range(B):
        ords = rng.permutation(S * K_IN).astype(np.int64) + 1000
        keys = rng.integers(-3, 4, size=S * K_IN) / 8.0  # 7 distinct keys, 0.0 among them
        ent_k, ent_o, ent_s = [], [], []
        for s in range(S):
            n = count[s, b]
            kk, oo = keys[s * K_IN:s * K_IN + n], ords[s * K_IN:s * K_IN + n]
            order = np.lexsort((oo, -kk))
            rank[s, b, :n], ids[s, b, :n] = kk[order], oo[order]
            scores[s, b, :n] = (oo[order] % 4096).astype(np.float32)  # follows its entry
            ent_k.append(kk), ent_o.append(oo), ent_s.append((oo % 4096).astype(np.float32))
        ent_k, ent_o, ent_s = (np.concatenate(x) for x in (ent_k, ent_o, ent_s))
        order = np.lexsort((ent_o, -ent_k))[:K_OUT]
        want.append((ent_k[order], ent_o[order], ent_s[order]))
    m = merge_shards(_dev(rank, gpu), _dev(scores, gpu), _dev(ids, gpu), _dev(count, gpu), K_OUT)
    got = _np(m, ("ids", "scores", "rank", "count"))
    for b, (wk, wo, ws) in enumerate(want):
        n = len(wo)
        assert got["count"][b] == n == min(K_OUT, int(count[:, b].sum()))
        np.testing.assert_array_equal(got["ids"][b, :n], wo, err_msg=f"query {b}")
        np.testing.assert_array_equal(got["rank"][b, :n], wk, err_msg=f"query {b}")
        np.testing.assert_array_equal(got["scores"][b, :n], ws, err_msg=f"query {b}")
        assert (got["ids"][b, n:] == -1).all()
    assert got["count"].tolist()[:3] == [240, 0, 3]
