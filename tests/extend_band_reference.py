"""Banded extension alignment with direction bytes, restated in numpy: the yardstick of the NW_EXTEND_BAND tests.

Not a test file.  The contract is include/msa.h's at msa_extend_align_banded.  The cells ARE the banded global
alignment's, on the CLIPPED pair: with m' = min(m, n + w) and n' = min(n, m + w) (rows past n + w and columns past
m + w hold no cell with |i - j| <= w), H, the bytes and their masks come from nw_scored_reference.nw_scored_reference
(wide_reference.nw_reference32 for more than 8 symbols) with band = w on A[:m'], B[:n'], unchanged.  On top of them:
the end cell is the first maximum of H over `valid` (the in-band interior) in row-major order; a maximum <= 0 is the
empty extension; the walk is extend_reference.walk_from's, completed by the global border gap; and the global score
H(m, n) exists only when nothing was clipped.
"""
from __future__ import annotations

import numpy as np

import extend_reference as XR
import nw_scored_reference as RS
import wide_reference as WR
from nw_reference import NEG, rs, similar  # noqa: F401
from nw_scored_reference import SCORE_SETS, cigar_of  # noqa: F401
from extend_reference import score_set  # noqa: F401


def clip(m: int, n: int, w: int):
    """(m', n') of the clip rule; |m' - n'| <= w always."""
    assert m >= 1 and n >= 1 and w >= 0
    return min(m, n + w), min(n, m + w)


def banded_global(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int, w: int, walk=False) -> dict:
    """The banded global yardstick's dictionary for up to 32 symbols (|m - n| <= w)."""
    fn = WR.nw_reference32 if len(alphabet) > 8 else RS.nw_scored_reference
    return fn(A, B, alphabet, S, g, h, w, walk)


def extend_band_reference(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int, w: int) -> dict:
    """dict(score, end, stop, global_score, best, w, m_eff, n_eff, H, byte, efin, ffin, valid, walk_ops, ops): as
    extend_reference's, for the band w; (m_eff, n_eff) = the clipped sizes the per-cell band-form arrays belong to;
    global_score = H(m, n), or None where the pair was clipped."""
    m, n = len(A), len(B)
    me, ne = clip(m, n, w)
    assert abs(me - ne) <= w
    glob = banded_global(A[:me], B[:ne], alphabet, S, g, h, w)
    assert glob["w"] == w
    Hv = np.where(glob["valid"], glob["H"], NEG)
    flat = int(np.argmax(Hv))  # the first maximum of the flattened band form: rows ascend, and within a row columns do
    i, d = divmod(flat, Hv.shape[1])
    best = int(Hv[i, d])
    end = (i, d + i - w)
    # (every row 1..m' has an in-band cell and its H is finite: row 1 of a band-0 pair is (1, 1) already)
    assert 1 <= end[0] <= me and 1 <= end[1] <= ne and abs(end[0] - end[1]) <= w and best > NEG // 2
    score = best
    if best <= 0:
        score, end = 0, (0, 0)
    walk_ops, stop = XR.walk_from(glob["byte"], end, w)
    assert stop[0] <= w and stop[1] <= w  # the walk never leaves the band, so neither does the border gap
    ops = walk_ops + b"I" * stop[0] + b"D" * stop[1]
    return dict(score=score, end=end, stop=stop, global_score=glob["score"] if (me, ne) == (m, n) else None, best=best,
                w=w, m_eff=me, n_eff=ne, H=glob["H"], byte=glob["byte"], efin=glob["efin"], ffin=glob["ffin"],
                valid=glob["valid"], walk_ops=walk_ops, ops=ops)


def rescore(A: bytes, B: bytes, end, ops: bytes, alphabet: bytes, S, g: int, h: int, band: int) -> int:
    """extend_reference.rescore between the prefixes A[:end[0]] and B[:end[1]], asserting too that every cell of the
    path has |i - j| <= band."""
    assert 0 <= end[0] <= len(A) and 0 <= end[1] <= len(B)
    if not ops:
        assert tuple(end) == (0, 0)
        return 0
    a, b = A[:end[0]], B[:end[1]]
    if len(alphabet) > 8:
        return WR.rescore32(a, b, ops, alphabet, S, g, h, band)
    return RS.rescore(a, b, ops, alphabet, S, g, h, band)


# ---- the named cases: name -> (score set, band, (A, B)) ------------------------------------------------------------
# Regular stripes (the v_writelane edge phases of the stripe kernel) need band >= 64, i0 - band > 1 and
# i0 + 63 + band < n for a stripe of rows i0 .. i0 + 63: with band 64 on 400 x 400 that is rows 129..192 alone.
def _P(seed, L):
    return rs(np.random.default_rng(seed), L)


def _upper_edge():
    """The end cell on the band's upper edge, j - i = 64, in row 160 of the regular stripe: B is A's first 160 symbols
    behind 64 'C's."""
    P = _P(301, 160)
    return P + b"A" * 240, b"C" * 64 + P + b"G" * 176


def _lower_edge():
    """The mirror, i - j = 64: A is B's first 120 symbols behind 64 'C's; the end cell is (184, 120)."""
    P = _P(302, 120)
    return b"C" * 64 + P + b"G" * 216, P + b"A" * 280


def _outside(nc):
    """After a common "GGG", B holds nc 'C's and then A's next 200 symbols: that diagonal is j - i = nc.  69 is outside
    a band of 64 (the unbanded extension takes it: 265 at (203, 272)); 64 is its edge."""
    P = b"T" + _P(303, 199)  # (its first symbol matches neither the 'C's nor the 'G's around it)
    return b"GGG" + P, b"GGG" + b"C" * nc + P + b"T" * 50


def _sim(seed, m):
    return similar(np.random.default_rng(seed), m)


def _rnd(seed, m, n):
    rng = np.random.default_rng(seed)
    return rs(rng, m), rs(rng, n)


def _prefix(seed, L, m, n):
    return XR._prefix(seed, L, m, n)


def _single_1000():
    """One pair over several workgroups: an edited copy of A's first 700 symbols, with a 30-symbol deletion at 400."""
    rng = np.random.default_rng(304)
    ref = rs(rng, 1000)
    b = bytearray(XR.edited(rng, ref[:700]))
    del b[400:430]
    return ref[:700] + b"A" * 300, bytes(b) + b"C" * (1000 - len(b))


CASES = {
    # 1. regular stripes, band 64, 400 x 400
    "upper_edge_w64": ("dna", 64, _upper_edge),
    "lower_edge_w64": ("dna", 64, _lower_edge),
    "random_400_w64": ("dna", 64, lambda: _rnd(305, 400, 400)),
    # 2. a better alignment just outside the band is ignored; on its edge it is taken
    "outside_69_w64": ("dna", 64, lambda: _outside(69)),
    "edge_64_w64": ("dna", 64, lambda: _outside(64)),
    # 3. body phases inside a band: band 128, 600 x 600 (stripes of rows 193..448 are regular and have unmasked phases)
    "similar_600_w128": ("dna", 128, lambda: tuple(s[:600] for s in _sim(306, 640))),
    "allA_600_w128_zero": ("zero", 128, lambda: (b"A" * 600, b"A" * 600)),
    # 5. clipping: m > n + w and n > m + w, a common prefix of 100; one pair clipped to a single stripe
    "clip_rows_400x150_w16": ("dna", 16, lambda: _prefix(307, 100, 400, 150)),
    "clip_cols_150x400_w16": ("dna", 16, lambda: _prefix(308, 100, 150, 400)),
    "clip_one_stripe_300x40_w8": ("dna", 8, lambda: _prefix(309, 30, 300, 40)),
    # 7. the empty extension
    "all_negative_w16": ("dna", 16, lambda: (b"A" * 70, b"C" * 80)),
    "best_zero_w8": ("unit", 8, lambda: (b"CA" + b"G" * 70, b"GA" + b"C" * 72)),
    "zero_borders_w16": ("zero", 16, lambda: (b"A" * 70, b"C" * 80)),
    # 8. one pair over several workgroups
    "single_1000_w100": ("dna", 100, _single_1000),
}
# 4. bands that never take the fast path, on a 150 x 150 and a 300 x 290 pair (|m - n| = 10: band 8 clips the second)
SLOW_BANDS = (0, 1, 8, 63, 65)
for _w in SLOW_BANDS:
    CASES[f"similar_150_w{_w}"] = ("dna", _w, lambda: tuple(s[:150] for s in _sim(310, 170)))
    CASES[f"random_300x290_w{_w}"] = ("dna", _w, lambda: _rnd(311, 300, 290))
CASES["equal_150_w0"] = ("dna", 0, lambda: (_P(312, 150),) * 2)          # band 0 on equal sequences: the diagonal
CASES["corner_on_edge_300x290_w10"] = ("dna", 10, lambda: (_P(313, 300), _P(313, 300)[:290]))  # |m - n| = w exactly

# what the contract gives where the answer is known in advance: score, end cell, CIGAR, global score (None: clipped;
# ...: not stated)
KNOWN = {
    "upper_edge_w64": (189, (160, 224), "64D160M", ...),
    "lower_edge_w64": (109, (184, 120), "64I120M", ...),
    "outside_69_w64": (6, (3, 3), "3M", None),
    "edge_64_w64": (275, (203, 267), "3M64D200M", None),
    "clip_rows_400x150_w16": (200, (100, 100), "100M", None),
    "clip_cols_150x400_w16": (200, (100, 100), "100M", None),
    "clip_one_stripe_300x40_w8": (60, (30, 30), "30M", None),
    "all_negative_w16": (0, (0, 0), "", ...),
    "best_zero_w8": (0, (0, 0), "", ...),
    "zero_borders_w16": (0, (0, 0), "", ...),
    "equal_150_w0": (300, (150, 150), "150M", 300),
    "allA_600_w128_zero": (600, (600, 600), "600M", 600),  # the longest common subsequence of two prefixes: min(i, j)
}
CLIPPED = {"outside_69_w64": (203, 267), "edge_64_w64": (203, 267), "clip_rows_400x150_w16": (166, 150),
           "clip_cols_150x400_w16": (150, 166), "clip_one_stripe_300x40_w8": (48, 40),
           "random_300x290_w0": (290, 290), "random_300x290_w1": (291, 290), "random_300x290_w8": (298, 290)}


_CACHE = {}


def case(name):
    """(A, B, alphabet, S, g, h, w, reference dict) of a named case, computed once and never modified."""
    if name not in _CACHE:
        sset, w, make = CASES[name]
        A, B = make()
        al, S, g, h = score_set(sset)
        _CACHE[name] = (A, B, al, S, g, h, w, extend_band_reference(A, B, al, S, g, h, w))
    return _CACHE[name]


# a mixed batch under one band (32): a long extension, a clipped pair, the empty extension, a full-length one, one row
BATCH_BAND = 32


def batch_pairs():
    rng = np.random.default_rng(314)
    ref = rs(rng, 700)
    same = rs(rng, 77)
    return [(XR.edited(rng, ref[:180]) + b"A" * 20, ref[:180] + b"C" * 40),
            _prefix(315, 40, 150, 400),
            (b"A" * 64, b"C" * 70),
            (same, same),
            (b"G", b"G" + rs(rng, 49))]


def shared_b_batch():
    """extend_reference.shared_b_batch: five reads against one 300-symbol B; under band 32 the short reads clip B."""
    return XR.shared_b_batch()
