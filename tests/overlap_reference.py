"""Overlap (suffix-prefix, "dovetail") alignment with direction bytes, restated in numpy: the yardstick of the
NW_OVERLAP tests.

Not a test file.  It is fit_reference.fit_reference with two changes, the contract include/msa.h documents at
msa_overlap_align: the left border is H(i, 0) = 0 with E = F = -inf, like the top border (A's symbols before the
aligned part are free too), and the result is the better of two first maxima -- row m's over columns 1..n and column
n's over rows 1..m, the last row winning a tie -- or, when neither is positive, the empty overlap: score 0, end cell
(m, 0), no walk.  Interior cells, tie order and byte format are unchanged, and the walk is msa_plan_traceback_nw's
started at the end cell; nothing is appended where it stops.  Every per-cell array is in nw_reference's band form
with w = max(m, n) (no band).
"""
from __future__ import annotations

import numpy as np

import alphabet8 as A8
import wide_reference as WR
from fit_reference import UNIT, edited  # noqa: F401
from nw_reference import NEG, band_cols, rs
from nw_scored_reference import SCORE_SETS, cigar_of, match_mismatch  # noqa: F401
from nw_scored_reference import codes as _codes8
from nw_scored_reference import rescore as _rescore8


def codes(seq: bytes, alphabet: bytes) -> np.ndarray:
    """The codes of seq's symbols (their indices in alphabet): up to 8 symbols, or up to 32."""
    return WR.codes32(seq, alphabet) if len(alphabet) > 8 else _codes8(seq, alphabet)


def overlap_reference(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int) -> dict:
    """dict(score, end, beg, w, H, byte, efin, ffin, valid, ops, best_r, j_r, best_c, i_c): end = the end cell (end_i,
    end_j), beg = the cell where the walk stopped; H int64, byte uint8, efin / ffin = "E / F is finite", valid =
    interior cells, all in band form with w = max(m, n); ops = the walk's ops end -> start, nothing appended.  The
    alignment is A[beg[0]:end[0]] against B[beg[1]:end[1]]; the empty overlap is score 0, end = beg = (m, 0), ops
    b""."""
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
    col = np.empty(m, dtype=np.int64)               # H(i, n), i = 1..m
    left0 = 0                                       # H(i, 0): the zero left border (E = F = -inf there)
    for i in range(1, m + 1):
        diag = Hp[js - 1] + S[a[i - 1], b[js - 1]]
        F = np.maximum(Hp[js] - op, Fp[js] - g)
        X = np.maximum(diag, F)
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
        col[i - 1] = Hc[-1]
        Hn = np.empty(n + 1, dtype=np.int64)
        Fn = np.full(n + 1, NEG, dtype=np.int64)
        Hn[0] = left0
        Hn[js] = Hc
        Fn[js] = F
        Hp, Fp = Hn, Fn
    _, valid = band_cols(m, n, w)
    row = Hp[1:]
    j_r = int(np.argmax(row)) + 1                   # argmax: the first maximum
    i_c = int(np.argmax(col)) + 1
    best_r, best_c = int(row[j_r - 1]), int(col[i_c - 1])
    best = max(best_r, best_c)
    end = (m, j_r) if best_r >= best_c else (i_c, n)
    if best <= 0:
        best, end = 0, (m, 0)
    ops, beg = walk_overlap(byte, end, w)
    return dict(score=best, end=end, beg=beg, w=w, H=H, byte=byte, efin=efin, ffin=ffin, valid=valid, ops=ops,
                best_r=best_r, j_r=j_r, best_c=best_c, i_c=i_c)


def walk_overlap(byte: np.ndarray, end, w: int):
    """msa_plan_traceback_nw's walk over band-form bytes from the end cell in state H, to the first cell with i == 0
    or j == 0: (ops end -> start, that cell).  Nothing is appended; an end cell on the border is no walk."""
    i, j = end
    st = 0
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
    return bytes(ops), (i, j)


def rescore(A: bytes, B: bytes, beg, end, ops: bytes, alphabet: bytes, S, g: int, h: int) -> int:
    """Score of the alignment `ops` (end -> start) describes between A[beg[0]:end[0]] and B[beg[1]:end[1]]: S per
    'M', h + g L per gap run of length L; asserts that it consumes exactly both pieces.  No ops: 0."""
    assert 0 <= beg[0] <= end[0] <= len(A) and 0 <= beg[1] <= end[1] <= len(B)
    if not ops:
        assert beg == end
        return 0
    a, b = A[beg[0]:end[0]], B[beg[1]:end[1]]
    if len(alphabet) > 8:
        return WR.rescore32(a, b, ops, alphabet, S, g, h)
    return _rescore8(a, b, ops, alphabet, S, g, h)


def borders_ok(ref_or_res: dict, m: int, n: int) -> bool:
    """The four border conditions of a result with keys beg and end."""
    (bi, bj), (ei, ej) = ref_or_res["beg"], ref_or_res["end"]
    return (bi == 0 or bj == 0) and (ei == m or ej == n) and 0 <= bi <= ei <= m and 0 <= bj <= ej <= n


# ---- the named shapes: name -> (A, B), run under "dna" (+2 / -3, g = 2, h = 3) unless a test says otherwise ------
def _rnd(seed, m, n):
    rng = np.random.default_rng(seed)
    return rs(rng, m), rs(rng, n)


def _dovetail(swap=False):
    """A = P(120) + O(80), B = O + Q(120): A's last 80 symbols are B's first 80."""
    rng = np.random.default_rng(51)
    P, O, Q = rs(rng, 120), rs(rng, 80), rs(rng, 120)
    return (O + Q, P + O) if swap else (P + O, O + Q)


def _a_in_b(swap=False):
    rng = np.random.default_rng(52)
    big = rs(rng, 700)
    small = edited(rng, big[300:400])
    return (big, small) if swap else (small, big)


def _tie_row_col():
    """A = W2 + R1 + W1, B = W1 + R2 + W2: A's suffix W1 on B's prefix ends on the last row at (170, 60), A's prefix W2
    on B's suffix ends on the last column at (60, 190), both with score 120."""
    rng = np.random.default_rng(53)
    W1, W2, R1, R2 = rs(rng, 60), rs(rng, 60), rs(rng, 50), rs(rng, 70)
    return W2 + R1 + W1, W1 + R2 + W2


def _tie_col_twice():
    """B (90 symbols) occurs in A twice, ending at rows 130 (stripe 2) and 270 (stripe 4): H(130, 90) = H(270, 90) =
    180, the largest score a 90-column alignment can have."""
    rng = np.random.default_rng(54)
    Wd = rs(rng, 90)
    return rs(rng, 40) + Wd + rs(rng, 50) + Wd + rs(rng, 30), Wd


def _late_5000():
    rng = np.random.default_rng(55)
    ref = rs(rng, 5000)
    return edited(rng, ref[-60:]) + rs(rng, 40), ref


def _single_1000x3000():
    """A's first 700 symbols are an edited copy of B's last 700: the end cell (700, 3000) is a column candidate of
    stripe 10, in the third of the pair's four workgroups."""
    rng = np.random.default_rng(56)
    ref = rs(rng, 3000)
    return edited(rng, ref[-700:]) + rs(rng, 300), ref


SHAPES = {
    "dovetail_ab": _dovetail,                                  # end on the last row, stop on the left border
    "dovetail_ba": lambda: _dovetail(True),                    # end on the last column (stripe 1 of 4), stop on the top
    "a_in_b": _a_in_b,                                         # A inside B: row m, stop on the top border
    "b_in_a": lambda: _a_in_b(True),                           # B inside A: column n in a middle stripe, stop on the left
    "m64": lambda: _rnd(61, 64, 300),                          # row m = the last lane of the only stripe
    "m65": lambda: _rnd(62, 65, 300),                          # ... lane 0 of a second stripe
    "m1": lambda: _rnd(63, 1, 200),                            # ... a single row
    "n1": lambda: _rnd(64, 200, 1),                            # a single column: every row is a column candidate
    "corner": lambda: (rs(np.random.default_rng(65), 150),) * 2,   # (m, n) is a row and a column candidate
    "tie_row_col": _tie_row_col,                               # best_r == best_c at different cells: the last row wins
    "tie_col_twice": _tie_col_twice,                           # equal column candidates in two stripes: the smaller row
    "empty": lambda: (b"A" * 70, b"C" * 200),                  # nothing positive: the empty overlap
    "q130_n40": lambda: _rnd(66, 130, 40),                     # n < 64: column n in every lane's first phases
    "late_5000": _late_5000,                                   # many phases per stripe, column n in the last one
    "single_1000x3000": _single_1000x3000,                     # one pair over many workgroups
}
# what the definition gives on the shapes whose answer is known in advance ("dna"): score, beg, end, CIGAR
KNOWN = {
    "dovetail_ab": (160, (120, 0), (200, 80), "80M"),
    "dovetail_ba": (160, (0, 120), (80, 200), "80M"),
    "corner": (300, (0, 0), (150, 150), "150M"),
    "tie_row_col": (120, (110, 0), (170, 60), "60M"),
    "tie_col_twice": (180, (40, 0), (130, 90), "90M"),
    "empty": (0, (70, 0), (70, 0), ""),
}
# "empty"'s pair under +1 / 0, g = 1, h = 2 (fit_reference.UNIT): every candidate is 0, a zero-score tie -> still empty
KNOWN_UNIT_EMPTY = KNOWN["empty"]

# a batch for one plan: contained, dovetail on the last row, dovetail on the last column, empty, one row
BATCH_MS, BATCH_NS = [200, 150, 77, 64, 1], [700, 200, 90, 300, 50]


def batch_pairs():
    rng = np.random.default_rng(57)
    big = rs(rng, 700)
    ov1, ov2 = rs(rng, 60), rs(rng, 40)
    return [(edited(rng, big[10:210]), big),
            (rs(rng, 90) + ov1, ov1 + rs(rng, 140)),
            (ov2 + rs(rng, 37), rs(rng, 50) + ov2),
            (b"A" * 64, b"C" * 300),
            (rs(rng, 1), rs(rng, 50))]


def shared_b_batch():
    """(As, B): five reads against one 300-symbol B -- a dovetail over B's start, one over its end, a read inside it,
    one around it (the whole of B inside the read) and a random read."""
    rng = np.random.default_rng(58)
    ref = rs(rng, 300)
    return [rs(rng, 50) + ref[:70], ref[-80:] + rs(rng, 45), edited(rng, ref[100:190]),
            rs(rng, 30) + ref + rs(rng, 35), rs(rng, 40)], ref


def eight_symbols():
    """(A, B, alphabet, S, g, h): an 8-symbol alphabet under alphabet8's asymmetric dense table; A's last 150 symbols
    are, with substitutions, B's first 150, and code 7 occurs inside the overlap on both sides."""
    rng = np.random.default_rng(59)
    ov = bytearray(A8.rs8(rng, 150))
    ov[40] = ov[41] = ov[100] = A8.AL8[7]
    cp = bytearray(ov)
    for k in range(3, 150, 6):  # (substitutions: the table's off-diagonal, asymmetric entries decide too)
        cp[k] = A8.AL8[(A8.AL8.index(cp[k]) + 3) % 8]
    return A8.rs8(rng, 100) + bytes(ov), bytes(cp) + A8.rs8(rng, 180), A8.AL8, A8.TABLE8, A8.G8, A8.H8


AL24 = WR.AL32[:24]


def protein32(k: int = 0):
    """(A, B, alphabet, S, g, h): 24 symbols under wide_reference.table32's first 24 rows and columns; a 150 x 330
    dovetail -- A's last 80 symbols are, mutated, B's first 80 (k: the seed's offset, for a batch of such pairs)."""
    rng = np.random.default_rng(60 + k)
    ov = WR.rs32(rng, 80, AL24)
    A = WR.rs32(rng, 70, AL24) + ov
    B = WR.mutated(rng, ov, AL24) + WR.rs32(rng, 250, AL24)
    return A, B, AL24, WR.table32()[:24, :24], 2, 9
