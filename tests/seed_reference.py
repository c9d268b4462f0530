"""Seed extension, restated from the X-drop yardstick: the yardstick of the seed tests.

Not a test file.  The contract is include/msa.h's at msa_seed_align.  A seed is A[seed_a : seed_a + seed_len] against
B[seed_b : seed_b + seed_len].  Its right flank is xdrop_reference.xdrop_reference of A[seed_a + seed_len:] against
B[seed_b + seed_len:], its left flank the same function of the two REVERSED prefixes A[:seed_a][::-1] and
B[:seed_b][::-1], under the same band and xdrop; a flank with no symbols on one side is the empty extension (score 0, end
(0, 0), diagonals 0, not dropped, no ops).  Then score = left + the seed's column scores + right, beg = seed - left end,
end = seed + seed_len + right end, and the ops of the whole alignment, end -> start (the convention of every
``cigar_of`` here): the right flank's as walked, seed_len 'M', and the left flank's turned round -- its walk runs from its
far end to the seed, which is start -> end of the whole already.
"""
from __future__ import annotations

import numpy as np

import extend_reference as XR
import xdrop_reference as XD
from nw_scored_reference import cigar_of

EMPTY = dict(score=0, end=(0, 0), diagonals=0, dropped=False, ops=b"")


def flanks(A: bytes, B: bytes, seed_a: int, seed_b: int, seed_len: int):
    """((left A, left B), (right A, right B)): the byte strings each flank's extension is run on."""
    assert 0 <= seed_a and 0 <= seed_b and 0 <= seed_len and seed_a + seed_len <= len(A) and seed_b + seed_len <= len(B)
    return (A[:seed_a][::-1], B[:seed_b][::-1]), (A[seed_a + seed_len:], B[seed_b + seed_len:])


def flank_reference(a: bytes, b: bytes, alphabet: bytes, S, g: int, h: int, w: int, xdrop: int) -> dict:
    """xdrop_reference's score, end, diagonals, dropped and ops of one flank; EMPTY for a flank without symbols on a
    side."""
    if not a or not b:
        return dict(EMPTY)
    r = XD.xdrop_reference(a, b, alphabet, S, g, h, w, xdrop)
    return {k: r[k] for k in EMPTY}


def seed_score(A: bytes, B: bytes, seed_a: int, seed_b: int, seed_len: int, alphabet: bytes, S) -> int:
    ca, cb = XR.codes(A[seed_a:seed_a + seed_len], alphabet), XR.codes(B[seed_b:seed_b + seed_len], alphabet)
    return int(np.asarray(S)[ca, cb].sum()) if seed_len else 0


def seed_reference(A: bytes, B: bytes, seed_a: int, seed_b: int, seed_len: int, alphabet: bytes, S, g: int, h: int,
                   w: int, xdrop: int) -> dict:
    """dict(score, beg, end, seed_score, left, right, ops, cigar): left / right = flank_reference's dictionaries (in the
    flank's own coordinates), ops = the whole alignment end -> start, cigar = its run-length string start -> end."""
    (la, lb), (ra, rb) = flanks(A, B, seed_a, seed_b, seed_len)
    L = flank_reference(la, lb, alphabet, S, g, h, w, xdrop)
    R = flank_reference(ra, rb, alphabet, S, g, h, w, xdrop)
    mid = seed_score(A, B, seed_a, seed_b, seed_len, alphabet, S)
    ops = R["ops"] + b"M" * seed_len + L["ops"][::-1]
    return dict(score=L["score"] + mid + R["score"], beg=(seed_a - L["end"][0], seed_b - L["end"][1]),
                end=(seed_a + seed_len + R["end"][0], seed_b + seed_len + R["end"][1]), seed_score=mid, left=L, right=R,
                ops=ops, cigar=cigar_of(ops))


def want(ref: dict, traceback=True) -> dict:
    """api.seed_align's dictionary of a seed_reference result."""
    def flank(f):
        return dict(score=f["score"], a_end=f["end"][0], b_end=f["end"][1], diagonals=f["diagonals"],
                    dropped=f["dropped"])

    r = dict(score=ref["score"], a_beg=ref["beg"][0], b_beg=ref["beg"][1], a_end=ref["end"][0], b_end=ref["end"][1],
             seed_score=ref["seed_score"], left=flank(ref["left"]), right=flank(ref["right"]))
    if traceback:
        r["cigar"] = ref["cigar"]
    return r


def parse_cigar(cigar: str):
    """[(run, op)] of a CIGAR string."""
    out, run = [], ""
    for c in cigar:
        if c.isdigit():
            run += c
        else:
            out.append((int(run), c))
            run = ""
    assert run == ""
    return out


def rescore(cigar: str, A: bytes, B: bytes, beg, end, alphabet: bytes, S, g: int, h: int) -> int:
    """The score of the alignment `cigar` (start -> end; M a column of both, I consumes A, D consumes B) describes of
    A[beg[0]:end[0]] against B[beg[1]:end[1]]: S per 'M' column, h + g L per gap run of length L.  Asserts that it
    consumes exactly end - beg on each side and that no two neighbouring runs hold the same op (it is run-length encoded
    once over the whole)."""
    ca, cb = XR.codes(A, alphabet), XR.codes(B, alphabet)
    S = np.asarray(S)
    i, j = beg
    score, last = 0, ""
    for run, op in parse_cigar(cigar):
        assert run > 0 and op in "MID" and op != last, cigar
        last = op
        if op == "M":
            score += int(S[ca[i:i + run], cb[j:j + run]].sum())
            i, j = i + run, j + run
        else:
            score -= h + g * run
            if op == "I":
                i += run
            else:
                j += run
    assert (i, j) == tuple(end), (cigar, beg, end, (i, j))
    return score
