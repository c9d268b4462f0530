"""Banded extension alignment with X-drop termination, restated in numpy: the yardstick of the X-drop tests.

Not a test file.  The contract is include/msa.h's at msa_extend_align_xdrop.  Everything is
extend_band_reference.extend_band_reference's on the clipped pair -- H, the bytes and their masks in band form, shape
(m' + 1, 2w + 1) --; on top of it: d = i + j, a(d) = the maximum of H over the in-band interior cells on anti-diagonal
d (-inf where d has none), best(d) = max(0, a(2), ..., a(d)); the fill stops after the first d in 2 .. m' + n' with
best(d) - max(a(d - 1), a(d)) > xdrop; D is that d, or m' + n'; xdrop < 0 never stops.  The result is the first
row-major maximum over the cells with i + j <= D, walked with extend_reference.walk_from.
"""
from __future__ import annotations

import numpy as np

import extend_band_reference as XB
import extend_reference as XR
from nw_reference import NEG, rs


def diagonal_maxima(ref: dict) -> np.ndarray:
    """a(d) for d = 0 .. m' + n' (NEG where d holds no in-band interior cell; a(0) = a(1) = NEG)."""
    me, ne, w = ref["m_eff"], ref["n_eff"], ref["w"]
    i = np.arange(me + 1)[:, None]
    d = 2 * i - w + np.arange(2 * w + 1)[None, :]  # i + j with j = i - w + column
    a = np.full(me + ne + 1, NEG, dtype=np.int64)
    v = ref["valid"]
    np.maximum.at(a, d[v], ref["H"][v])
    return a


def stop_diagonal(a: np.ndarray, xdrop: int):
    """(D, best(D) - max(a(D - 1), a(D)) or None when the rule never fired)."""
    last = len(a) - 1
    if xdrop < 0:
        return last, None
    best = 0
    for d in range(2, last + 1):
        best = max(best, int(a[d]))
        recent = max(int(a[d - 1]), int(a[d]))
        assert recent > NEG // 2, d  # two consecutive anti-diagonals always hold a cell
        if best - recent > xdrop:
            return d, best - recent
    return last, None


def xdrop_reference(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int, w: int, xdrop: int, band_ref=None) -> dict:
    """extend_band_reference's dictionary (its per-cell arrays unchanged, the same objects) with score, end, stop,
    global_score, best, walk_ops and ops under the stopping rule, and diagonals = D, dropped = D < m' + n', a = a(d),
    delta = best(D) - max(a(D - 1), a(D)) where the rule fired (else None), live = valid & (i + j <= D).  band_ref: the
    banded yardstick's dictionary of the same input, if the caller has it."""
    ref = band_ref if band_ref is not None else XB.extend_band_reference(A, B, alphabet, S, g, h, w)
    me, ne = ref["m_eff"], ref["n_eff"]
    a = diagonal_maxima(ref)
    D, delta = stop_diagonal(a, xdrop)
    i = np.arange(me + 1)[:, None]
    dd = 2 * i - w + np.arange(2 * w + 1)[None, :]
    live = ref["valid"] & (dd <= D)
    Hv = np.where(live, ref["H"], NEG)
    flat = int(np.argmax(Hv))  # the first maximum in row-major order
    bi, col = divmod(flat, Hv.shape[1])
    best = int(Hv[bi, col])
    end = (bi, col + bi - w)
    score = best
    if best <= 0:
        score, end = 0, (0, 0)
    walk_ops, stop = XR.walk_from(ref["byte"], end, w)
    dropped = D < me + ne
    gs = None if dropped else ref["global_score"]
    out = dict(ref)
    out.update(score=score, end=end, stop=stop, global_score=gs, best=best, walk_ops=walk_ops,
               ops=walk_ops + b"I" * stop[0] + b"D" * stop[1], diagonals=D, dropped=dropped, a=a, delta=delta, live=live,
               cells=int(live.sum()))
    return out


# ---- the prototype cases of the stopping rule: name -> (score set, band, (A, B), {xdrop: (score, end, D, dropped)}) ---
def _islands():
    rng = np.random.default_rng(5)
    P = rs(rng, 60)
    Q = rs(rng, 80)
    A = P + rs(rng, 25) + Q + rs(rng, 40)
    B = P + rs(rng, 25) + Q + rs(rng, 40)
    return A, B


STOPS = {
    "prefix40_w16": ("dna", 16, lambda: XR._prefix(7, 40, 300, 300),
                     {0: (80, (40, 40), 82, True), 3: (80, (40, 40), 84, True), 10: (80, (40, 40), 88, True),
                      50: (80, (40, 40), 114, True)}),
    "prefix30_w0": ("dna", 0, lambda: XR._prefix(7, 30, 90, 90),
                    {0: (60, (30, 30), 62, True), 3: (60, (30, 30), 64, True), 10: (60, (30, 30), 68, True),
                     50: (60, (30, 30), 94, True)}),
    "islands_w32": ("dna", 32, _islands,
                    {10: (124, (62, 62), 152, True), 30: (259, (165, 165), 408, True),
                     60: (259, (165, 165), 410, False), 1000: (259, (165, 165), 410, False),
                     -1: (259, (165, 165), 410, False)}),
}

_CACHE = {}


def stop_case(name):
    """(A, B, alphabet, S, g, h, w, banded reference) of a STOPS case, computed once and never modified."""
    if name not in _CACHE:
        sset, w, make, _ = STOPS[name]
        A, B = make()
        al, S, g, h = XB.score_set(sset)
        _CACHE[name] = (A, B, al, S, g, h, w, XB.extend_band_reference(A, B, al, S, g, h, w))
    return _CACHE[name]


def row_major_tie():
    """(A, B, alphabet, S, g, h, w, xdrop, (i1, j1), (i2, j2)): the smallest pair found by exhaustive search
    (test_xdrop_reference.py repeats the search) on which two live cells hold the maximum, the row-major first of them,
    (i1, j1), on the LATER anti-diagonal: i1 < i2 and i1 + j1 > i2 + j2."""
    al, S, g, h = XB.score_set("unit")
    return b"AACAG", b"CAGCA", al, S, g, h, 2, 100, (4, 5), (5, 3)
