"""Fit (query-in-reference) alignment with direction bytes, restated in numpy: the yardstick of the NW_FIT tests.

Not a test file.  It is nw_scored_reference.nw_scored_reference without a band and with two changes, the contract
include/msa.h documents at msa_fit_align: the top border is H(0, j) = 0 for every j (the reference's symbols before
the aligned substring are free), and the result is the first maximum of H(m, 1..n) (the symbols after it are free
too) instead of H(m, n).  Interior cells, the left border H(i, 0) = F(i, 0) = -h - g i, tie order and byte format
are unchanged, and the walk is msa_plan_traceback_nw's started at (m, end_j); of the border gap only i x 'I' is
appended.  Every per-cell array is in nw_reference's band form with w = max(m, n) (no band).
"""
from __future__ import annotations

import numpy as np

import alphabet8 as A8
from nw_reference import NEG, band_cols, rs
from nw_scored_reference import SCORE_SETS, cigar_of, codes, match_mismatch  # noqa: F401
from nw_scored_reference import rescore as _rescore_global


def fit_reference(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int) -> dict:
    """dict(score, end_j, beg_j, w, H, byte, efin, ffin, valid, ops, stop): score = max H(m, 1..n), end_j its first
    column; H int64, byte uint8, efin / ffin = "E / F is finite", valid = interior cells, all in band form with w =
    max(m, n); ops = the complete ops end -> start (the walk's from (m, end_j), then stop[0] x 'I'), stop = the
    border cell where the walk stopped, beg_j = stop[1].  The alignment is A against B[beg_j:end_j]."""
    assert g >= 0 and h >= 0
    S = np.asarray(S, dtype=np.int64)
    a = codes(A, alphabet)
    b = codes(B, alphabet)
    m, n = len(a), len(b)
    assert m >= 1 and n >= 1
    w = max(m, n)
    op = g + h
    W = 2 * w + 1
    H = np.full((m + 1, W), NEG, dtype=np.int64)
    byte = np.zeros((m + 1, W), dtype=np.uint8)
    efin = np.zeros((m + 1, W), dtype=bool)
    ffin = np.zeros((m + 1, W), dtype=bool)
    js = np.arange(1, n + 1)
    Hp = np.zeros(n + 1, dtype=np.int64)            # the zero top border
    Fp = np.full(n + 1, NEG, dtype=np.int64)
    H[0, w + np.arange(0, n + 1)] = 0
    for i in range(1, m + 1):
        diag = Hp[js - 1] + S[a[i - 1], b[js - 1]]
        F = np.maximum(Hp[js] - op, Fp[js] - g)
        X = np.maximum(diag, F)
        left0 = -h - g * i                          # H(i, 0)
        # E(i, j) = max_{k < j} (X(k) + g k) - op - g (j - 1), X(0) = the border (h >= 0: opening again never wins)
        Y = np.concatenate(([left0], X[:-1] + g * js[:-1]))
        E = np.maximum.accumulate(Y) - op - g * (js - 1)
        Hc = np.maximum(X, E)
        Hl = np.concatenate(([left0], Hc[:-1]))     # H(i, j-1)
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
        H[i, w - i] = left0
        Hn = np.empty(n + 1, dtype=np.int64)
        Fn = np.full(n + 1, NEG, dtype=np.int64)
        Hn[0] = left0
        Hn[js] = Hc
        Fn[js] = F
        Hp, Fp = Hn, Fn
    _, valid = band_cols(m, n, w)
    last = Hp[1:]
    end_j = int(np.argmax(last)) + 1                # argmax: the first maximum
    ops, stop = walk_fit(byte, m, end_j, w)
    return dict(score=int(last[end_j - 1]), end_j=end_j, beg_j=stop[1], w=w, H=H, byte=byte, efin=efin, ffin=ffin,
                valid=valid, ops=ops, stop=stop)


def walk_fit(byte: np.ndarray, m: int, end_j: int, w: int):
    """msa_plan_traceback_nw's walk over band-form bytes from (m, end_j) in state H: (ops end -> start completed
    by stop[0] x 'I' -- never a 'D' --, stop cell)."""
    i, j, st = m, end_j, 0
    ops = bytearray()
    while i > 0 and j > 0:
        v = int(byte[i, j - i + w])
        if st == 0:
            lo = v & 3
            assert lo != 0, (i, j)
            if lo == 1:
                ops.append(ord("M"))
                i -= 1
                j -= 1
            else:
                st = lo - 1  # 1: E, 2: F
        elif st == 1:
            ops.append(ord("D"))
            j -= 1
            st = 0 if v & 4 else 1
        else:
            ops.append(ord("I"))
            i -= 1
            st = 0 if v & 8 else 2
    stop = (i, j)
    ops += b"I" * i
    return bytes(ops), stop


def rescore(A: bytes, B: bytes, beg: int, end: int, ops: bytes, alphabet: bytes, S, g: int, h: int) -> int:
    """Score of the alignment `ops` (end -> start) describes between A and B[beg:end]: S per 'M', h + g L per gap
    run of length L; asserts that it consumes exactly m and end - beg."""
    assert 0 <= beg <= end <= len(B)
    return _rescore_global(A, B[beg:end], ops, alphabet, S, g, h)


# ---- the named shapes: name -> (A, B), run under "dna" (+2 / -3, g = 2, h = 3) unless a test says otherwise ------
def edited(rng, q: bytes, frac=0.03) -> bytes:
    """q with about `frac` of its symbols substituted by another one (at least one)."""
    s = bytearray(q)
    for k in rng.choice(len(s), size=max(1, int(len(s) * frac)), replace=False):
        s[k] = b"ACGT"[(b"ACGT".index(s[k]) + 1 + int(rng.integers(3))) % 4]
    return bytes(s)


def planted(seed: int, m: int, n: int, at: int):
    """A random query of m symbols; a random reference of n with an edited copy of the query at offset `at`."""
    rng = np.random.default_rng(seed)
    q = rs(rng, m)
    ref = bytearray(rs(rng, n))
    ref[at:at + m] = edited(rng, q)
    return q, bytes(ref)


def _rnd(seed, m, n):
    rng = np.random.default_rng(seed)
    return rs(rng, m), rs(rng, n)


def _tie_twice():
    q = rs(np.random.default_rng(5), 100)
    fl = rs(np.random.default_rng(6), 300)
    return q, fl[:70] + q + fl[70:200] + q + fl[200:]


def _end_at_n():
    ref = rs(np.random.default_rng(31), 300)
    return ref[-80:], ref


def _overhang():
    rng = np.random.default_rng(4025)
    X = rs(rng, 130)
    return X, X[25:] + rs(rng, 200)


SHAPES = {
    "q100_in_r700": lambda: planted(21, 100, 700, 333),        # row m = lane 35 of stripe 1
    "m64_r300": lambda: _rnd(22, 64, 300),                     # row m = the last lane of the only stripe
    "m65_r300": lambda: _rnd(23, 65, 300),                     # ... lane 0 of a second stripe
    "m1_r200": lambda: _rnd(24, 1, 200),                       # ... a single row
    "tie_twice": _tie_twice,                                   # two equal maxima on row m: the first wins
    "end_at_n": _end_at_n,                                     # the query is a suffix of the reference
    "end_at_1": lambda: (b"A" * 70, b"C" * 200),               # "dna": everything inserted at column 1
    "overhang_25I": _overhang,                                 # the query overhangs the reference's start
    "q130_r40": lambda: _rnd(25, 130, 40),                     # the query is longer than the reference
    "q100_r5000_late": lambda: planted(26, 100, 5000, 4700),   # many phases per stripe, the maximum in a late one
    "q1000_r3000": lambda: planted(27, 1000, 3000, 1234),      # one pair over many workgroups
}
# what the definition gives on the shapes whose answer is known in advance ("dna"): score, beg, end, CIGAR
KNOWN = {
    "tie_twice": (200, 70, 170, "100M"),
    "end_at_1": (-143, 1, 1, "70I"),
    "overhang_25I": (157, 0, 105, "25I105M"),
}
# "end_at_1"'s pair under +1 / 0, g = 1, h = 2
UNIT = (b"ACGT", match_mismatch(b"ACGT", 1, 0), 1, 2)
KNOWN_UNIT_END_AT_1 = (0, 0, 70, "70M")

# a batch for one plan: rows, columns (row m in a third stripe, a second, lane 12 of a second, the last lane, one row)
BATCH_MS, BATCH_NS = [200, 150, 77, 64, 1], [700, 200, 90, 300, 50]


def batch_pairs():
    rng = np.random.default_rng(28)
    out = []
    for m, n in zip(BATCH_MS, BATCH_NS):
        q = rs(rng, m)
        ref = bytearray(rs(rng, n))
        if n >= m + 20:
            ref[10:10 + m] = edited(rng, q)
        out.append((q, bytes(ref)))
    return out


def eight_symbols():
    """(A, B, alphabet, S, g, h): an 8-symbol alphabet under alphabet8's asymmetric dense table; an edited copy of
    the query sits at offset 90 of the reference, and code 7 occurs in both, inside the aligned part too."""
    rng = np.random.default_rng(29)
    q = bytearray(A8.rs8(rng, 150))
    q[40] = q[41] = q[100] = A8.AL8[7]
    ref = bytearray(A8.rs8(rng, 330))
    cp = bytearray(q)
    for k in range(3, 150, 6):  # (substitutions: the table's off-diagonal, asymmetric entries decide too)
        cp[k] = A8.AL8[(A8.AL8.index(cp[k]) + 3) % 8]
    ref[90:240] = cp
    return bytes(q), bytes(ref), A8.AL8, A8.TABLE8, A8.G8, A8.H8
