"""Banded global (Gotoh) alignment under a substitution matrix, restated in numpy: the yardstick of the NW_SCORED
tests.

Not a test file.  It is nw_reference.nw_reference with one change: the diagonal term's (b == a) is the lookup
S[code of A_i][code of B_j] (rows of S are A's symbol, columns B's; S need not be symmetric; a symbol's code is its
index in `alphabet`).  Recurrence, borders, band rule, tie order, byte format and walk are the ones include/msa.h
documents for msa_plan_traceback_nw, and every per-cell array is in nw_reference's band form.  The prefix-maximum
form of E holds for any S: it needs h >= 0 only.
"""
from __future__ import annotations

import numpy as np

from nw_reference import (BATCH_MS, BATCH_NS, BATCH_WIDE_BAND, BATCH_WIDE_MS, BATCH_WIDE_NS, CHUNKED,  # noqa: F401
                          NEG, NOBAND, SMALL, band_cols, band_width, batch_pairs, batch_wide_pairs, chunked_case,
                          cigar_of, to_band, walk_bytes)


def codes(seq: bytes, alphabet: bytes) -> np.ndarray:
    """The codes of seq's symbols (their indices in alphabet); every symbol must be in the alphabet."""
    assert len(set(alphabet)) == len(alphabet) <= 8
    lut = np.full(256, -1, dtype=np.int64)
    lut[np.frombuffer(alphabet, dtype=np.uint8)] = np.arange(len(alphabet))
    c = lut[np.frombuffer(seq, dtype=np.uint8)]
    assert (c >= 0).all(), "a symbol outside the alphabet"
    return c


def nw_scored_reference(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int, band: int = -1, walk=True) -> dict:
    """nw_reference's dictionary (score, w, H, byte, efin, ffin, valid [, ops, stop]) with f(i, j) = S[A_i][B_j]."""
    assert g >= 0 and h >= 0
    S = np.asarray(S, dtype=np.int64)
    a = codes(A, alphabet)
    b = codes(B, alphabet)
    m, n = len(a), len(b)
    w = band_width(m, n, band)
    assert abs(m - n) <= w
    op = g + h
    W = 2 * w + 1
    H = np.full((m + 1, W), NEG, dtype=np.int64)
    byte = np.zeros((m + 1, W), dtype=np.uint8)
    efin = np.zeros((m + 1, W), dtype=bool)
    ffin = np.zeros((m + 1, W), dtype=bool)
    # rows as absolute-column arrays (n + 1), -inf outside the row's band
    Hp = np.full(n + 1, NEG, dtype=np.int64)
    Fp = np.full(n + 1, NEG, dtype=np.int64)
    Hp[0] = 0
    jb = np.arange(1, min(n, w) + 1)
    Hp[jb] = -h - g * jb
    H[0, w - 0 + np.arange(0, min(n, w) + 1)] = Hp[:min(n, w) + 1]
    for i in range(1, m + 1):
        jlo, jhi = max(1, i - w), min(n, i + w)
        js = np.arange(jlo, jhi + 1)
        diag = Hp[js - 1] + S[a[i - 1], b[js - 1]]
        F = np.maximum(Hp[js] - op, Fp[js] - g)
        X = np.maximum(diag, F)
        # the left neighbour of the row's first cell: the border column 0 (rows <= band), else out of band
        left0 = -h - g * i if (jlo == 1 and i <= w) else NEG
        Y = np.concatenate(([left0 + g * (jlo - 1)], X[:-1] + g * js[:-1]))
        E = np.maximum.accumulate(Y) - op - g * (js - 1)
        Hc = np.maximum(X, E)
        Hl = np.concatenate(([left0], Hc[:-1]))  # H(i, j-1)
        for v in (diag, E, F, Hc, Hl):
            v[v < NEG // 2] = NEG
        lo = np.where(Hc == diag, 1, np.where(Hc == E, 2, 3)).astype(np.uint8)
        bt = lo | (((E == Hl - op) & (Hl > NEG // 2)).astype(np.uint8) << 2) | \
            (((F == Hp[js] - op) & (Hp[js] > NEG // 2)).astype(np.uint8) << 3)
        d = js - i + w
        H[i, d] = Hc
        byte[i, d] = bt
        efin[i, d] = E > NEG // 2
        ffin[i, d] = F > NEG // 2
        Hn = np.full(n + 1, NEG, dtype=np.int64)
        Fn = np.full(n + 1, NEG, dtype=np.int64)
        Hn[js] = Hc
        Fn[js] = F
        if i <= w:
            Hn[0] = -h - g * i
        Hp, Fp = Hn, Fn
    _, valid = band_cols(m, n, w)
    out = dict(score=int(H[m, n - m + w]), w=w, H=H, byte=byte, efin=efin, ffin=ffin, valid=valid)
    if walk:
        out["ops"], out["stop"] = walk_bytes(byte, m, n, w)
    return out


def rescore(A: bytes, B: bytes, ops: bytes, alphabet: bytes, S, g: int, h: int, band: int = -1) -> int:
    """Score of the alignment `ops` (end -> start) describes: S per 'M', h + g L per gap run of length L; asserts
    that it consumes exactly m and n and that every visited cell has |i - j| <= band."""
    S = np.asarray(S, dtype=np.int64)
    a = codes(A, alphabet)
    b = codes(B, alphabet)
    o = np.frombuffer(ops, dtype=np.uint8)[::-1]  # start -> end
    assert np.isin(o, np.frombuffer(b"MID", dtype=np.uint8)).all()
    isM, isI, isD = o == ord("M"), o == ord("I"), o == ord("D")
    i = np.cumsum(isM | isI)
    j = np.cumsum(isM | isD)
    assert (i[-1] if len(o) else 0) == len(a) and (j[-1] if len(o) else 0) == len(b), "ops do not consume (m, n)"
    if band >= 0:
        assert int(np.abs(i - j).max(initial=0)) <= band, "the path leaves the band"
    gap = ~isM
    runs = int((gap & np.concatenate(([True], o[1:] != o[:-1]))).sum())
    return int(S[a[i[isM] - 1], b[j[isM] - 1]].sum()) - g * int(gap.sum()) - h * runs


# ---- the score sets: name -> (alphabet, S, g, h), open = g + h -----------------------------------------------
def match_mismatch(alphabet: bytes, match: int, mismatch: int) -> np.ndarray:
    k = len(alphabet)
    S = np.full((k, k), mismatch, dtype=np.int64)
    np.fill_diagonal(S, match)
    return S


def _titv() -> np.ndarray:
    """ACGTN: match 1, transition (A<->G, C<->T) -1, transversion -2, N against anything 0."""
    S = np.full((5, 5), -2, dtype=np.int64)
    np.fill_diagonal(S, 1)
    for x, y in ((0, 2), (1, 3)):
        S[x, y] = S[y, x] = -1
    S[4, :] = 0
    S[:, 4] = 0
    return S


ASYM = np.array([[2, -3, -1, -4], [-2, 3, -5, 0], [-1, -1, 1, -2], [-6, -3, -2, 4]], dtype=np.int64)
SCORE_SETS = {
    "dna": (b"ACGT", match_mismatch(b"ACGT", 2, -3), 2, 3),
    "unit": (b"ACGT", match_mismatch(b"ACGT", 1, -1), 1, 0),
    "edit": (b"ACGT", match_mismatch(b"ACGT", 0, -1), 1, 0),
    "neg": (b"ACGT", match_mismatch(b"ACGT", 1, -4), 1, 0),
    "titv": (b"ACGTN", _titv(), 1, 2),
    "asym": (b"ACGT", ASYM, 1, 1),
}


def with_n(seq: bytes, seed: int, frac=0.05) -> bytes:
    """seq with about `frac` of its positions set to N by a seeded generator (the "titv" inputs)."""
    rng = np.random.default_rng(seed)
    s = bytearray(seq)
    for k in np.flatnonzero(rng.random(len(s)) < frac):
        s[k] = ord("N")
    return bytes(s)


def set_input(set_name: str, A: bytes, B: bytes):
    """The inputs a score set runs on: (A, B) themselves, or for "titv" with N at ~5% of the positions."""
    return (with_n(A, 101), with_n(B, 202)) if set_name == "titv" else (A, B)


def sub8(S) -> np.ndarray:
    """The plan's 8 x 8 int8 table of an n_sym x n_sym matrix (unused codes score 0)."""
    S = np.asarray(S)
    out = np.zeros((8, 8), dtype=np.int8)
    out[:S.shape[0], :S.shape[1]] = S
    return out
