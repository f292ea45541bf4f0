"""Adversarial sparse rows and queries for the sparse search tests: rows that share an index with
the query and score exactly 0. include/armi.h makes them results on every path ("also when its
score is 0 or negative"), ranked (score desc, ordinal asc) behind the positive rows; a kernel that
ranks by an upper bound of the score cannot tell most of them from rows that share nothing.

corpus() is oracle.sparse_corpus(n) (values >= 0.01) with the postings of seven labelled classes
added to 59 of its rows, on five term ids the base corpus does not use (TERM_NAMES), scattered by
one seeded permutation:

  P    7  the hot term with a value in U(0.05, 0.4): positive scores.
  PL   4  the hot term with a value in U(0.01, 0.05): positive scores below P's. With them the
          rows of positive score and the UF rows together outnumber k = 20 (7 + 4 + 12 = 23), so
          a top 20 taken from the rows a positive upper bound can see ends inside the zero block.
  ZV  12  the hot term with value +0.0.
  NZ   6  the hot term with value -0.0 (w * -0.0 = -0.0, and +0.0 + -0.0 = +0.0).
  ZW  12  value 0.3 on a term the query carries with weight 0.
  AZ   6  value 0.0 on a term whose every posting is zero (its largest value, and so any scale
          derived from it, is 0).
  UF  12  value 1e-30 on a term the query carries with weight 1e-30: the product underflows to
          +0, so the exact score is 0 although both factors are positive.

Every class row also holds the fifth term ("co", value 0.2), which only the class rows hold and no
special query carries: in twin(), the same corpus with every zero-valued posting removed, the ZV, NZ
and AZ rows keep a posting of their own and the set of stored terms differs by "az" alone.

queries() is one batch (one 64-query pass) of every KIND: the special queries first, then ordinary
oracle.sparse_queries, so the tiny query shares its pass with queries of ordinary magnitude.
"""

import numpy as np

from oracle import oracle

CLASSES = (("P", 7), ("PL", 4), ("ZV", 12), ("NZ", 6), ("ZW", 12), ("AZ", 6), ("UF", 12))
LABELS = tuple(c for c, _ in CLASSES) + ("base",)
CLASS_ROWS = sum(n for _, n in CLASSES)
TERM_NAMES = ("zw", "az", "hot", "co", "uf")      # ascending ids: zero products on both sides of hot
KINDS = ("zero", "zero_negw", "hot_only", "tiny", "ordinary")
N_SPECIAL = 4                                     # queries 0..3 are zero, zero_negw, hot_only, tiny
FIRST_FRESH = 200000                              # the fresh ids are taken from here up
# the case both test modules use: 3,000 rows are 47 row ranges of 64 rows on an MI355X, so the
# classes spread over many scan workgroups; k = 240 is above the MFMA filter's limit of 128
N, SEED, BASE, N_ORDINARY, KS = 3000, 7, 1000, 20, (5, 20, 64, 128, 240)
_F32 = np.float32


def fresh_terms(base_indices: np.ndarray) -> dict:
    """Five ids in [FIRST_FRESH, oracle.VOCAB) that the base corpus does not use, spread out."""
    used = np.zeros(oracle.VOCAB, dtype=bool)
    used[base_indices] = True
    ids, t = [], FIRST_FRESH
    for _ in TERM_NAMES:
        while used[t]:
            t += 1
        ids.append(t)
        t += 9973
    assert ids[-1] < oracle.VOCAB and not used[ids].any()
    return dict(zip(TERM_NAMES, ids))


def permutation(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed + 1000).permutation(n)


def labels(n: int, seed: int) -> np.ndarray:
    """Class index (into LABELS) of every row; class rows are the first CLASS_ROWS entries of the
    permutation, class by class."""
    lab = np.full(n, len(LABELS) - 1, dtype=np.int64)
    where = permutation(n, seed)
    at = 0
    for c, (_, count) in enumerate(CLASSES):
        lab[where[at:at + count]] = c
        at += count
    return lab


def rows_of(lab: np.ndarray, name: str) -> np.ndarray:
    return np.nonzero(lab == LABELS.index(name))[0]


def _from_lists(rows):
    ip = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r[0]) for r in rows], out=ip[1:])
    return (ip, np.concatenate([r[0] for r in rows]).astype(np.int32),
            np.concatenate([r[1] for r in rows]).astype(_F32))


def _to_lists(csr):
    ip, ix, iv = csr
    return [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(len(ip) - 1)]


def corpus(n: int, seed: int):
    """(CSR, TERMS dict, labels)."""
    base = oracle.sparse_corpus(n, seed=seed)
    assert base[2].min() >= _F32(0.01) and base[1].max() <= oracle.VOCAB - 1
    terms = fresh_terms(base[1])
    lab = labels(n, seed)
    rng = np.random.default_rng(seed + 2000)
    posting = {"P": lambda: ("hot", _F32(rng.uniform(0.05, 0.4))),
               "PL": lambda: ("hot", _F32(rng.uniform(0.01, 0.05))), "ZV": lambda: ("hot", _F32(0.0)),
               "NZ": lambda: ("hot", _F32(-0.0)), "ZW": lambda: ("zw", _F32(0.3)),
               "AZ": lambda: ("az", _F32(0.0)), "UF": lambda: ("uf", _F32(1e-30))}
    rows = _to_lists(base)
    for r in np.nonzero(lab < len(CLASSES))[0]:
        name, value = posting[LABELS[lab[r]]]()
        ix = np.concatenate([rows[r][0], [terms[name], terms["co"]]]).astype(np.int32)
        iv = np.concatenate([rows[r][1], [value, _F32(0.2)]]).astype(_F32)
        order = np.argsort(ix, kind="stable")
        rows[r] = (ix[order], iv[order])
    csr = _from_lists(rows)
    nz = csr[2][rows_of_value(csr, terms["hot"], lab, "NZ")]
    assert nz.size == 6 and np.signbit(nz).all() and (nz == 0).all()
    return csr, terms, lab


def rows_of_value(csr, term: int, lab: np.ndarray, name: str) -> np.ndarray:
    """Positions (into values) of `term`'s postings in the rows of class `name`."""
    ip, ix, _ = csr
    out = []
    for r in rows_of(lab, name):
        at = ip[r] + np.nonzero(ix[ip[r]:ip[r + 1]] == term)[0]
        assert at.size == 1
        out.append(int(at[0]))
    return np.array(out, dtype=np.int64)


def twin(csr):
    """The same rows with every zero-valued posting (+0.0 or -0.0) removed."""
    return _from_lists([(ix[iv != 0], iv[iv != 0]) for ix, iv in _to_lists(csr)])


def rows_range(csr, lo: int, hi: int):
    """Rows [lo, hi) as a CSR of their own."""
    ip, ix, iv = csr
    return ip[lo:hi + 1] - ip[lo], ix[ip[lo]:ip[hi]], iv[ip[lo]:ip[hi]]


def move_terms(a: np.ndarray, shift: int = 300000) -> np.ndarray:
    """An order-preserving move of the ids from FIRST_FRESH up (the special ids among them) beyond
    2^18, for an index of a larger vocabulary."""
    return np.where(a >= FIRST_FRESH, a + shift, a).astype(np.int32)


def bits(ok: np.ndarray) -> np.ndarray:
    words = np.zeros(max((len(ok) + 63) // 64, 1), dtype=np.uint64)
    for r in np.nonzero(ok)[0]:
        words[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return words


def keep_half(lab: np.ndarray, seed: int) -> np.ndarray:
    """bool per row: a seeded half (rounded up) of every class, the base rows included."""
    rng = np.random.default_rng(seed + 3000)
    ok = np.zeros(lab.size, dtype=bool)
    for c in range(len(LABELS)):
        rows = np.nonzero(lab == c)[0]
        ok[rng.permutation(rows)[:(rows.size + 1) // 2]] = True
    return ok


def _special(terms: dict, kind: str):
    if kind == "hot_only":
        return np.array([terms["hot"]], np.int32), np.array([0.25], _F32)
    zero = _F32(-0.0 if kind == "zero_negw" else 0.0)
    w = {"hot": _F32(0.25), "zw": zero, "uf": _F32(1e-30), "az": _F32(0.5)}
    names = sorted(w, key=lambda t: terms[t])
    return (np.array([terms[t] for t in names], np.int32), np.array([w[t] for t in names], _F32))


def queries(terms: dict, n_ordinary: int, seed: int):
    """(query CSR, kind index per query): zero, zero_negw, hot_only, tiny, then n_ordinary ordinary
    queries."""
    oi, ox, ov = oracle.sparse_queries(n_ordinary + 1, seed=seed + 4000)
    lists = [_special(terms, k) for k in KINDS[:3]]
    lists.append((ox[oi[0]:oi[1]], (ov[oi[0]:oi[1]] * _F32(1e-37)).astype(_F32)))
    lists += [(ox[oi[b]:oi[b + 1]], ov[oi[b]:oi[b + 1]]) for b in range(1, n_ordinary + 1)]
    qi = np.zeros(len(lists) + 1, dtype=np.int32)
    np.cumsum([len(t) for t, _ in lists], out=qi[1:])
    kinds = np.array([0, 1, 2, 3] + [4] * n_ordinary)
    assert (lists[3][1] > 0).all()  # tiny, not zero
    return (qi, np.concatenate([t for t, _ in lists]).astype(np.int32),
            np.concatenate([w for _, w in lists]).astype(_F32)), kinds


def numpy_topk(csr, q, k: int, ok: np.ndarray | None = None, base: int = 0):
    """The documented rule as a numpy merge join: fp32 products, added in ascending index order
    from +0.0f, a row a result when it shares an index, ranked (score desc, ordinal asc).
    Returns [(ids, scores)] per query."""
    ip, ix, iv = csr
    qi, qx, qv = q
    n = len(ip) - 1
    row = np.repeat(np.arange(n), np.diff(ip))
    out = []
    for b in range(len(qi) - 1):
        score, hit = np.zeros(n, dtype=_F32), np.zeros(n, dtype=bool)
        for t, w in zip(qx[qi[b]:qi[b + 1]], qv[qi[b]:qi[b + 1]]):  # ascending index
            at = np.nonzero(ix == t)[0]
            score[row[at]] = score[row[at]] + (_F32(w) * iv[at]).astype(_F32)
            hit[row[at]] = True
        live = np.nonzero(hit if ok is None else hit & ok)[0]
        order = live[np.lexsort((live, -score[live].astype(np.float64)))][:k]
        out.append((base + order, score[order]))
    return out
