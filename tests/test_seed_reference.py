"""The seed yardstick (tests/seed_reference.py) against itself and against answers known by hand: its score is the
score of its own CIGAR recomputed from the sequences, the CIGAR consumes exactly end - beg, and small cases pin the
orientation of the left flank's ops, the empty flanks and the bare anchor.  Nothing here needs a GPU."""
import numpy as np
import pytest

import extend_band_reference as XB
import seed_reference as SR
import xdrop_reference as XD

DNA = XB.score_set("dna")  # +2 / -3, g = 2, h = 3


def _seeded_cases():
    """A few dozen (A, B, seed_a, seed_b, seed_len, score set, band, xdrop): similar pairs with a seed found where both
    hold the same symbols, random pairs with an arbitrary seed, both under three score sets."""
    out = []
    for k in range(36):
        rng = np.random.default_rng(9000 + k)
        sset = ("dna", "asym", "unit")[k % 3]
        if k % 2:
            A, B = XB.similar(rng, int(rng.integers(40, 160)), sub=0.08, indel=0.02)
        else:
            A, B = XB.rs(rng, int(rng.integers(1, 90))), XB.rs(rng, int(rng.integers(1, 90)))
        sl = int(rng.integers(0, min(len(A), len(B), 12) + 1))
        sa, sb = int(rng.integers(0, len(A) - sl + 1)), int(rng.integers(0, len(B) - sl + 1))
        out.append((A, B, sa, sb, sl, sset, (0, 3, 16, 200)[k % 4], (-1, 0, 6, 25)[(k // 4) % 4]))
    return out


@pytest.mark.parametrize("k", range(36))
def test_score_is_the_cigars(k):
    A, B, sa, sb, sl, sset, w, xdrop = _seeded_cases()[k]
    al, S, g, h = XB.score_set(sset)
    ref = SR.seed_reference(A, B, sa, sb, sl, al, S, g, h, w, xdrop)
    assert SR.rescore(ref["cigar"], A, B, ref["beg"], ref["end"], al, S, g, h) == ref["score"]
    used = SR.parse_cigar(ref["cigar"])
    assert sum(r for r, op in used if op in "MI") == ref["end"][0] - ref["beg"][0]
    assert sum(r for r, op in used if op in "MD") == ref["end"][1] - ref["beg"][1]
    assert ref["beg"][0] <= sa and ref["beg"][1] <= sb and ref["end"][0] >= sa + sl and ref["end"][1] >= sb + sl
    assert ref["score"] == ref["left"]["score"] + ref["seed_score"] + ref["right"]["score"]
    # each flank is the X-drop yardstick of its own two byte strings, the left one reversed
    (la, lb), (ra, rb) = SR.flanks(A, B, sa, sb, sl)
    assert (la, lb) == (A[:sa][::-1], B[:sb][::-1]) and (ra, rb) == (A[sa + sl:], B[sb + sl:])
    for f, a, b in ((ref["left"], la, lb), (ref["right"], ra, rb)):
        if a and b:
            x = XD.xdrop_reference(a, b, al, S, g, h, w, xdrop)
            assert f == {key: x[key] for key in SR.EMPTY}
        else:
            assert f == SR.EMPTY


def _rep():
    return XB.rs(np.random.default_rng(77), 90)


def test_exact_repeat():
    P = _rep()
    al, S, g, h = DNA
    ref = SR.seed_reference(P, P, 40, 40, 11, al, S, g, h, 8, 20)
    assert ref["cigar"] == "90M" and (ref["beg"], ref["end"], ref["score"]) == ((0, 0), (90, 90), 180)
    assert (ref["left"]["end"], ref["right"]["end"], ref["seed_score"]) == ((40, 40), (39, 39), 22)
    # ... shifted: the seed sits on another diagonal, and the coordinates follow it
    ref = SR.seed_reference(b"GG" + P, P, 42, 40, 11, al, S, g, h, 8, 20)
    assert ref["cigar"] == "90M" and (ref["beg"], ref["end"]) == ((2, 0), (92, 90))


def test_left_flank_deletion_pins_the_orientation():
    """B holds one symbol more than A, 10 symbols left of the seed: start -> end the alignment is 29 M, 1 D, 10 M, the
    seed, the right flank -- the mirrored order (10M1D29M) would be the left ops read the wrong way round."""
    P = _rep()
    al, S, g, h = DNA
    A = P[:29] + P[30:]          # A lacks P[29]
    B = P
    sa, sb, sl = 39, 40, 10      # A[39:49] == B[40:50]
    assert A[sa:sa + sl] == B[sb:sb + sl]
    ref = SR.seed_reference(A, B, sa, sb, sl, al, S, g, h, 8, -1)
    assert ref["cigar"] == "29M1D60M"
    assert (ref["beg"], ref["end"]) == ((0, 0), (89, 90))
    assert ref["score"] == 2 * 89 - (3 + 2)
    # (the flank's own CIGAR, what extend_align gives for the reversed prefixes, is the mirror image)
    assert ref["left"]["end"] == (39, 40) and SR.cigar_of(ref["left"]["ops"]) == "10M1D29M"
    # an insertion on the right flank, 5 symbols after the seed: it stays right of the seed's M
    A2 = P[:60] + b"T" + P[60:]
    ref = SR.seed_reference(A2, P, 45, 45, 10, al, S, g, h, 8, -1)
    assert ref["cigar"] == "60M1I30M"
    # the left flank's border gap comes after its ops: A holds one symbol more right next to the seed, so the left
    # flank's walk ends on its border at (1, 0) and the gap that completes it stands between the flank's M and the seed's
    t = b"A" if P[19:20] != b"A" and P[20:21] != b"A" else (b"C" if b"C" not in (P[19:20], P[20:21]) else b"G")
    A3 = P[:20] + t + P[20:50]
    ref = SR.seed_reference(A3, P[:50], 21, 20, 10, al, S, g, h, 4, -1)
    assert ref["left"]["ops"] == b"M" * 20 + b"I" and ref["left"]["end"] == (21, 20)
    assert ref["cigar"] == "20M1I30M" and (ref["beg"], ref["end"]) == ((0, 0), (51, 50))


def test_empty_flanks_and_bare_anchor():
    P = _rep()[:30]
    al, S, g, h = DNA
    # the seed at (0, 0): no left flank
    ref = SR.seed_reference(P, P, 0, 0, 6, al, S, g, h, 4, 10)
    assert ref["left"] == SR.EMPTY and ref["cigar"] == "30M" and ref["beg"] == (0, 0)
    # ... at 0 on one side only: the other side's symbols cannot be aligned to anything
    ref = SR.seed_reference(P, b"CC" + P, 0, 2, 6, al, S, g, h, 4, 10)
    assert ref["left"] == SR.EMPTY and ref["cigar"] == "30M" and (ref["beg"], ref["end"]) == ((0, 2), (30, 32))
    # the seed ending at (m, n): no right flank
    ref = SR.seed_reference(P, P, 24, 24, 6, al, S, g, h, 4, 10)
    assert ref["right"] == SR.EMPTY and ref["cigar"] == "30M" and ref["end"] == (30, 30)
    ref = SR.seed_reference(P, P + b"GG", 24, 24, 6, al, S, g, h, 4, 10)
    assert ref["right"] == SR.EMPTY and ref["end"] == (30, 30)
    # the seed = both whole sequences, with a mismatch inside it
    Q = P[:10] + (b"A" if P[10:11] != b"A" else b"C") + P[11:]
    ref = SR.seed_reference(P, Q, 0, 0, 30, al, S, g, h, 4, 10)
    assert ref["left"] == ref["right"] == SR.EMPTY
    assert (ref["score"], ref["seed_score"], ref["cigar"]) == (2 * 29 - 3, 2 * 29 - 3, "30M")
    # seed_len = 0: a bare anchor between two symbols
    ref = SR.seed_reference(P, P, 12, 12, 0, al, S, g, h, 4, 10)
    assert (ref["score"], ref["seed_score"], ref["cigar"]) == (60, 0, "30M")
    assert ref["left"]["end"] == (12, 12) and ref["right"]["end"] == (18, 18)
    # ... where nothing extends: the empty alignment at the anchor
    ref = SR.seed_reference(b"AAAA", b"CCCC", 2, 2, 0, al, S, g, h, 4, 10)
    assert (ref["score"], ref["cigar"], ref["beg"], ref["end"]) == (0, "", (2, 2), (2, 2))


def test_want_shapes_the_api_dictionary():
    P = _rep()
    al, S, g, h = DNA
    ref = SR.seed_reference(P, P, 40, 40, 11, al, S, g, h, 8, 20)
    w = SR.want(ref)
    assert set(w) == {"score", "a_beg", "b_beg", "a_end", "b_end", "seed_score", "left", "right", "cigar"}
    assert set(w["left"]) == set(w["right"]) == {"score", "a_end", "b_end", "diagonals", "dropped"}
    assert "cigar" not in SR.want(ref, traceback=False)
