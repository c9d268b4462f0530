"""Global / banded and fit alignment over alphabets of up to 32 symbols: the yardstick of the wide-alphabet tests.

Not a test file.  nw_scored_reference.nw_scored_reference and fit_reference.fit_reference index S by code already; only
their `codes()` stops at 8 symbols.  The references here are those two functions, called with the lookup replaced by
`codes32` (the same function with the limit at 32), so recurrence, borders, band rule, tie order, byte format, walk and
the returned dictionaries are theirs by construction.  test_wide_alphabet_host.py checks them against the 8-code
yardsticks key by key and against `gotoh_brute`, a plain-Python three-matrix DP that shares no code with them.
"""
from __future__ import annotations

import contextlib

import numpy as np

import fit_reference as FR
import nw_scored_reference as RS
from nw_reference import NEG, band_cols, band_width, cigar_of, to_band, walk_bytes  # noqa: F401

# 32 distinct bytes: code k is AL32[k]; the first 20 are the amino acids, then B Z X * and eight more letters
AL32 = b"ARNDCQEGHILKMFPSTWYVBZX*JOUabcde"
AL20 = AL32[:20]
assert len(set(AL32)) == 32


def codes32(seq: bytes, alphabet: bytes) -> np.ndarray:
    """nw_scored_reference.codes for alphabets of up to 32 symbols."""
    assert len(set(alphabet)) == len(alphabet) <= 32
    lut = np.full(256, -1, dtype=np.int64)
    lut[np.frombuffer(alphabet, dtype=np.uint8)] = np.arange(len(alphabet))
    c = lut[np.frombuffer(seq, dtype=np.uint8)]
    assert (c >= 0).all(), "a symbol outside the alphabet"
    return c


@contextlib.contextmanager
def _wide_lookup():
    """The 8-code yardsticks' symbol lookup replaced by codes32 for the duration of one call."""
    saved = (RS.codes, FR.codes)
    RS.codes = FR.codes = codes32
    try:
        yield
    finally:
        RS.codes, FR.codes = saved


def nw_reference32(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int, band: int = -1, walk=True) -> dict:
    """nw_scored_reference's dictionary (score, w, H, byte, efin, ffin, valid [, ops, stop]), up to 32 symbols."""
    with _wide_lookup():
        return RS.nw_scored_reference(A, B, alphabet, S, g, h, band, walk)


def fit_reference32(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int) -> dict:
    """fit_reference's dictionary (score, end_j, beg_j, w, H, byte, efin, ffin, valid, ops, stop), up to 32 symbols."""
    with _wide_lookup():
        return FR.fit_reference(A, B, alphabet, S, g, h)


def rescore32(A: bytes, B: bytes, ops: bytes, alphabet: bytes, S, g: int, h: int, band: int = -1) -> int:
    with _wide_lookup():
        return RS.rescore(A, B, ops, alphabet, S, g, h, band)


def fit_rescore32(A: bytes, B: bytes, beg: int, end: int, ops: bytes, alphabet: bytes, S, g: int, h: int) -> int:
    with _wide_lookup():
        return FR.rescore(A, B, beg, end, ops, alphabet, S, g, h)


def gotoh_brute(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int, fit=False):
    """(H, E, F) as (m+1) x (n+1) lists of Python ints (None = -inf) by the recurrence include/msa.h states, cell by
    cell: E(i,j) = max(H(i,j-1) - (g+h), E(i,j-1) - g), F(i,j) = max(H(i-1,j) - (g+h), F(i-1,j) - g), H(i,j) =
    max(H(i-1,j-1) + S[A_i][B_j], E, F); H(0,0) = 0, H(0,j) = -h - g j (fit: 0), H(i,0) = F(i,0) = -h - g i, no band."""
    a, b = codes32(A, alphabet).tolist(), codes32(B, alphabet).tolist()
    S = np.asarray(S).tolist()
    m, n = len(a), len(b)

    def mx(*v):
        v = [x for x in v if x is not None]
        return max(v) if v else None

    def sub(x, c):
        return None if x is None else x - c

    H = [[None] * (n + 1) for _ in range(m + 1)]
    E = [[None] * (n + 1) for _ in range(m + 1)]
    F = [[None] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, n + 1):
        H[0][j] = 0 if fit else -h - g * j
    for i in range(1, m + 1):
        H[i][0] = F[i][0] = -h - g * i
        for j in range(1, n + 1):
            E[i][j] = mx(sub(H[i][j - 1], g + h), sub(E[i][j - 1], g))
            F[i][j] = mx(sub(H[i - 1][j], g + h), sub(F[i - 1][j], g))
            H[i][j] = mx(H[i - 1][j - 1] + S[a[i - 1]][b[j - 1]], E[i][j], F[i][j])
    return H, E, F


# ---- tables and inputs of the wide-alphabet tests ---------------------------------------------------------------
def table32() -> np.ndarray:
    """A dense asymmetric 32 x 32 int8 table in [-11, 17]: S[a][b] = (7a + 13b) % 23 - 11 off the diagonal (a swapped
    index or a wrong 8-code group changes the score), 12 + a % 6 on it."""
    a = np.arange(32)
    S = (7 * a[:, None] + 13 * a[None, :]) % 23 - 11
    S[a, a] = 12 + a % 6
    return S.astype(np.int64)


def protein20() -> np.ndarray:
    """A symmetric 20 x 20 table shaped like a log-odds protein matrix: off the diagonal in [-4, 3], the diagonal in
    [4, 11] (seeded)."""
    rng = np.random.default_rng(62)
    off = rng.integers(-4, 4, size=(20, 20))
    S = np.triu(off, 1)
    S = S + S.T
    S[np.arange(20), np.arange(20)] = rng.integers(4, 12, size=20)
    return S.astype(np.int64)


def sub32(S) -> np.ndarray:
    """The plan's 32 x 32 int8 table of an n_sym x n_sym matrix (unused codes score 0)."""
    S = np.asarray(S)
    out = np.zeros((32, 32), dtype=np.int8)
    out[:S.shape[0], :S.shape[1]] = S
    return out


def rs32(rng, n: int, alphabet: bytes = AL32) -> bytes:
    """n random symbols of the alphabet."""
    return rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n).tobytes()


def mutated(rng, q: bytes, alphabet: bytes, frac=0.05) -> bytes:
    """q with about `frac` of its symbols replaced by another symbol of the alphabet (at least one)."""
    s = bytearray(q)
    for k in rng.choice(len(s), size=max(1, int(len(s) * frac)), replace=False):
        s[k] = alphabet[(alphabet.index(s[k]) + 1 + int(rng.integers(len(alphabet) - 1))) % len(alphabet)]
    return bytes(s)
