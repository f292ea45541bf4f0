"""Adversarial fp16 rows and queries for the dense search tests: everything here is inside the
store's stated domain (every |x| < 2, oracle `fp16_in_domain`) except the four class-F rows, which
must be counted invalid and never returned.

Corpus classes (BLOCK_ROWS = 844 rows before the unit filler; LABELS names them):

  A      256  unit rows (oracle.unit_fp16). Rows 0..63 are snapped to the 2^-18 grid first (only
              components below 2^-8 move), so that the 2^-6 multiple of class B is exact in fp16.
  B    4 x 64 rows 0..63 of A times 2^-1, 2^-3, 2^-6, 2^0: a power-of-two multiple scales dot by
              2^-e and norm2 by 4^-e exactly, so its fp64 key is bit-identical to the original's
              (exact key ties across magnitudes, ordered by ordinal only).
  C1      64  unit rows x 2^-12 rounded to fp16 (mostly subnormal components).
  C2      64  every component a random subnormal (bits 0x0001..0x03FF) with a random sign.
  L       64  large norm: clip(unit * 40, +-1.999).
  D       64  spikes: one hot component from {1.5, -1.5, 2^-20, 0.37} at an index < 8; odd rows
              carry +-2^-20 in every other component (they quantise to a one-hot int8 image, so the
              filter's residual terms carry everything), even rows are zero elsewhere; every third
              row also gets a 2^-24 component. Rows share hot indices: one-hot queries tie on them.
  E        8  zero rows, half of them all -0.0 (0x8000): inv_norm = 0, key 0 for every query.
  G    2 x 32 unit rows and, later in the block, a copy with component 5 changed by one fp16 ulp:
              near ties that only the exact rescore can order.
  F        4  invalid rows: +inf, NaN, 2.0, -inf in one component.

corpus() appends unit filler rows and scatters everything with one seeded permutation, so every
32-row tile mixes classes. queries() cycles through the ten KINDS.
"""

import numpy as np

from oracle import oracle

BLOCK_ROWS = 844
LABELS = ("A", "B", "C1", "C2", "L", "D", "E", "G", "F", "fill")
KINDS = ("unit", "unit_2^-12", "subnormal", "large", "one_hot", "zero", "neg_zero", "row_copy",
         "row_negated", "c2_copy")
UNIT_KIND = 0
_F32, _F16, _U16 = np.float32, np.float16, np.uint16


def _f32(u16: np.ndarray) -> np.ndarray:
    return u16.view(_F16).astype(_F32)


def _u16(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x.astype(_F16)).view(_U16)


def _subnormals(rng: np.random.Generator, n: int, dim: int) -> np.ndarray:
    mag = rng.integers(1, 0x400, size=(n, dim), dtype=np.int64)
    sign = rng.integers(0, 2, size=(n, dim), dtype=np.int64) << 15
    return (mag | sign).astype(_U16)


def _spikes(rng: np.random.Generator, n: int, dim: int) -> np.ndarray:
    hot = (1.5, -1.5, 2.0 ** -20, 0.37)
    x = np.zeros((n, dim), dtype=_F32)
    for i in range(n):
        if i % 2:
            x[i] = rng.choice(np.array([-1.0, 1.0], dtype=_F32), size=dim) * _F32(2.0 ** -20)
        x[i, int(rng.integers(0, 8))] = hot[i % 4 if i < n // 2 else int(rng.integers(0, 4))]
        if i % 3 == 0:
            x[i, int(rng.integers(8, dim))] = 2.0 ** -24
    return _u16(x)


def block(dim: int, seed: int) -> tuple[np.ndarray, np.ndarray]:
    """(uint16 [BLOCK_ROWS, dim], int labels into LABELS) of the adversarial classes, unshuffled."""
    rng = np.random.default_rng([seed, dim, 1])
    base = _f32(oracle.unit_fp16(512, dim, seed=seed))
    base[:64] = np.round(base[:64] * _F32(2.0 ** 18)) * _F32(2.0 ** -18)
    near = oracle.unit_fp16(32, dim, seed=seed + 1)
    near_ulp = near.copy()
    near_ulp[:, 5] ^= 1
    bad = oracle.unit_fp16(4, dim, seed=seed + 2).copy()
    for r, (col, bits) in enumerate(((3, 0x7C00), (dim - 1, 0x7E00), (0, 0x4000), (dim // 2, 0xFC00))):
        bad[r, col] = bits
    zeros = np.zeros((8, dim), dtype=_U16)
    zeros[1::2] = 0x8000
    parts = [("A", _u16(base[:256]))]
    parts += [("B", _u16(base[:64] * _F32(2.0 ** e))) for e in (-1, -3, -6, 0)]
    parts += [("C1", _u16(base[64:128] * _F32(2.0 ** -12))),
              ("C2", _subnormals(rng, 64, dim)),
              ("L", _u16(np.clip(base[128:192] * _F32(40.0), -1.999, 1.999))),
              ("D", _spikes(rng, 64, dim)),
              ("E", zeros), ("G", near), ("G", near_ulp), ("F", bad)]
    rows = np.concatenate([p for _, p in parts])
    labels = np.concatenate([np.full(len(p), LABELS.index(name)) for name, p in parts])
    assert rows.shape == (BLOCK_ROWS, dim)
    return rows, labels


def permutation(n: int, seed: int) -> np.ndarray:
    """Row i of the scattered corpus is row permutation(n, seed)[i] of [block | filler]."""
    return np.random.default_rng([seed, n, 2]).permutation(n)


def labels(dim: int, n: int, seed: int) -> np.ndarray:
    lab = np.full(n, LABELS.index("fill"))
    lab[:BLOCK_ROWS] = block(dim, seed)[1]
    return lab[permutation(n, seed)]


def corpus(dim: int, n: int, seed: int) -> np.ndarray:
    """uint16 [n, dim]: the adversarial block, unit filler rows up to n, scattered by a seeded
    permutation. Deterministic in (dim, n, seed)."""
    assert n >= BLOCK_ROWS
    rows = block(dim, seed)[0]
    if n > BLOCK_ROWS:
        rows = np.concatenate([rows, oracle.unit_fp16(n - BLOCK_ROWS, dim, seed=seed + 3)])
    return np.ascontiguousarray(rows[permutation(n, seed)])


def valid_rows(rows: np.ndarray) -> np.ndarray:
    """bool [n]: every component inside the fp16 domain (exponent field <= 15)."""
    return (((rows >> 10) & 31) <= 15).all(axis=1)


def query_kinds(nq: int) -> np.ndarray:
    """Kind (index into KINDS) of each of queries()'s rows. After the first cycle the three kinds
    with only one possible vector (one-hot, zero, -0.0) would repeat it: they become unit queries."""
    kinds = np.arange(nq) % len(KINDS)
    fixed = np.isin(kinds, [KINDS.index(x) for x in ("one_hot", "zero", "neg_zero")])
    kinds[fixed & (np.arange(nq) >= len(KINDS))] = UNIT_KIND
    return kinds


def queries(dim: int, nq: int, rows: np.ndarray, seed: int, among=None) -> np.ndarray:
    """uint16 [nq, dim], every component in the row domain (|x| < 2): KINDS in turn, with fresh
    draws on every cycle. A prefix of a longer call is the shorter call. among: bool [n], the rows
    the row_copy / row_negated queries may copy (default: any valid non-zero row)."""
    unit = _f32(oracle.unit_fp16(nq, dim, seed=seed + 4))
    nonzero = valid_rows(rows) & ((rows & 0x7FFF) != 0).any(axis=1)
    any_row = np.nonzero(nonzero if among is None else nonzero & among)[0]
    all_sub = np.nonzero(nonzero & (((rows >> 10) & 31) == 0).all(axis=1))[0]
    out = np.zeros((nq, dim), dtype=_U16)
    for i, kind in enumerate(query_kinds(nq)):
        name = KINDS[kind]
        cycle = np.random.default_rng([seed, dim, 3, i // len(KINDS)])  # one stream per cycle
        copy_of = rows[cycle.choice(any_row)]
        if name == "unit":
            out[i] = _u16(unit[i])
        elif name == "unit_2^-12":
            out[i] = _u16(unit[i] * _F32(2.0 ** -12))
        elif name == "subnormal":
            out[i] = _subnormals(cycle, 1, dim)[0]
        elif name == "large":
            out[i] = _u16(np.clip(unit[i] * _F32(40.0), -1.999, 1.999))
        elif name == "one_hot":
            out[i, 2] = 0x3C00
        elif name == "neg_zero":
            out[i] = 0x8000
        elif name == "row_copy":
            out[i] = copy_of
        elif name == "row_negated":
            out[i] = copy_of ^ 0x8000  # of the row the cycle's row_copy query copies
        elif name == "c2_copy":
            out[i] = rows[cycle.choice(all_sub)]
    assert ((((out >> 10) & 31) <= 15).all())
    return out


def mask_words(ok: np.ndarray) -> np.ndarray:
    """uint64 row mask (bit r of word r // 64) of a bool array."""
    padded = np.zeros((len(ok) + 63) // 64 * 64, dtype=bool)
    padded[:len(ok)] = ok
    return np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64)
