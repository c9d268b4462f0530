"""The NW_EXTEND_BAND yardstick (tests/extend_band_reference.py) against independent statements, on the CPU: (a) a
plain triple-loop banded Gotoh over the WHOLE m x n matrix with the end-cell rule spelled out -- no clipping: cells
outside the band are -inf wherever they lie --, (b) the definition by exhaustion -- the best banded global score over
every pair of prefixes with |i - j| <= w --, (c) the clip rule, and (d) with w = max(m, n) the unbanded extension
yardstick itself."""
import numpy as np
import pytest

import extend_band_reference as XB
import extend_reference as ER
import nw_reference as R
import nw_scored_reference as RS
import wide_reference as WR

NINF = float("-inf")
SCORINGS = {"dna": RS.SCORE_SETS["dna"], "asym": RS.SCORE_SETS["asym"], "zero": ER.ZERO,
            "protein24": (ER.AL24, WR.table32()[:24, :24], 2, 9)}


def _rand(rng, n, alphabet, k=None):
    return WR.rs32(rng, n, alphabet[:k or len(alphabet)])


def brute_extend_band(A, B, alphabet, S, g, h, w):
    """(H, score, end cell, H(m, n) or None) of the contract include/msa.h documents at msa_extend_align_banded, cell by
    cell over the unclipped matrix in plain Python (exact -inf), the candidates scanned in row-major order with a
    strict >."""
    a, b = ER.codes(A, alphabet), ER.codes(B, alphabet)
    m, n = len(a), len(b)
    op = g + h
    H = [[NINF] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, min(n, w) + 1):
        H[0][j] = E[0][j] = -h - g * j
    for i in range(1, min(m, w) + 1):
        H[i][0] = F[i][0] = -h - g * i
    best, end = NINF, None
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if abs(i - j) > w:
                continue
            E[i][j] = max(H[i][j - 1] - op, E[i][j - 1] - g)
            F[i][j] = max(H[i - 1][j] - op, F[i - 1][j] - g)
            H[i][j] = max(H[i - 1][j - 1] + int(S[a[i - 1]][b[j - 1]]), E[i][j], F[i][j])
            if H[i][j] > best:
                best, end = H[i][j], (i, j)
    if best <= 0:
        best, end = 0, (0, 0)
    return H, best, end, (H[m][n] if abs(m - n) <= w else None)


def exhaustive(A, B, alphabet, S, g, h, w):
    """(score, end cell): max(0, the best BANDED global score of A[:i] against B[:j] over |i - j| <= w), the first such
    (i, j) in row-major order -- (0, 0) when nothing is positive."""
    best, end = 0, (0, 0)
    for i in range(1, len(A) + 1):
        for j in range(1, len(B) + 1):
            if abs(i - j) > w:
                continue
            sc = XB.banded_global(A[:i], B[:j], alphabet, S, g, h, w)["score"]
            if sc > best:
                best, end = sc, (i, j)
    return best, end


def _check_alignment(A, B, alphabet, S, g, h, w, ref):
    m, n = len(A), len(B)
    assert XB.rescore(A, B, ref["end"], ref["ops"], alphabet, S, g, h, w) == ref["score"]
    assert (ref["m_eff"], ref["n_eff"]) == XB.clip(m, n, w) and abs(ref["m_eff"] - ref["n_eff"]) <= w
    if (ref["m_eff"], ref["n_eff"]) == (m, n):
        assert ref["global_score"] == XB.banded_global(A, B, alphabet, S, g, h, w)["score"]
        assert ref["global_score"] <= ref["best"] or (m, n) == ref["end"]
    else:
        assert ref["global_score"] is None
    if ref["score"] == 0:
        assert (ref["end"], ref["stop"], ref["ops"]) == ((0, 0), (0, 0), b"") and ref["best"] <= 0
    else:
        assert ref["score"] == ref["best"] > 0 and abs(ref["end"][0] - ref["end"][1]) <= w
        assert (ref["stop"][0] == 0 or ref["stop"][1] == 0) and max(ref["stop"]) <= w


@pytest.mark.parametrize("scoring", list(SCORINGS))
def test_random_pairs_against_triple_loop(scoring):
    """60 random pairs per scoring up to 40 x 40 under bands 0..12 and one past both lengths (half of the pairs with a
    common prefix, a quarter with that prefix behind a few inserted symbols, so that results lie off the diagonal and on
    the band's edge): the in-band H cell by cell, the result, and the cells beyond the clip all out of band."""
    alphabet, S, g, h = SCORINGS[scoring]
    rng = np.random.default_rng(990 + len(scoring))
    clipped = 0
    for k in range(60):
        m, n = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        w = int(rng.integers(0, 13)) if k % 5 else max(m, n) + 3
        A, B = _rand(rng, m, alphabet), _rand(rng, n, alphabet)
        if k % 2:
            L = int(rng.integers(1, min(m, n) + 1))
            B = A[:L] + B[L:]
            if k % 4 == 1:
                B = (_rand(rng, int(rng.integers(0, w + 2)), alphabet) + B)[:n]
        ref = XB.extend_band_reference(A, B, alphabet, S, g, h, w)
        H, score, end, hmn = brute_extend_band(A, B, alphabet, S, g, h, w)
        assert (ref["score"], ref["end"], ref["global_score"]) == (score, end, hmn), (A, B, w)
        me, ne = ref["m_eff"], ref["n_eff"]
        clipped += (me, ne) != (m, n)
        full = np.array([[R.NEG if x == NINF else x for x in row] for row in H], dtype=np.int64)
        want = R.to_band(full[:me + 1, :ne + 1], w, fill=R.NEG)
        v = ref["valid"]
        assert np.array_equal(ref["H"][v], want[v]) and (ref["H"][v] > R.NEG // 2).all()
        # the clip rule: no cell beyond (m', n') is in band (the triple loop left every one of them at -inf)
        assert (full[me + 1:, :] == R.NEG).all() and (full[:, ne + 1:] == R.NEG).all()
        _check_alignment(A, B, alphabet, S, g, h, w, ref)
    assert clipped >= 10


@pytest.mark.parametrize("scoring", ["dna", "zero"])
def test_definition_by_exhaustion(scoring):
    """Pairs up to 12 x 12 under bands 0..4: the best banded global score over every in-band pair of prefixes."""
    alphabet, S, g, h = SCORINGS[scoring]
    rng = np.random.default_rng(77)
    for k in range(30):
        m, n, w = int(rng.integers(1, 13)), int(rng.integers(1, 13)), k % 5
        A, B = _rand(rng, m, alphabet, 3), _rand(rng, n, alphabet, 3)
        if k % 2:
            L = int(rng.integers(1, min(m, n) + 1))
            B = (_rand(rng, int(rng.integers(0, w + 2)), alphabet, 3) + A[:L] + B[L:])[:n]
        ref = XB.extend_band_reference(A, B, alphabet, S, g, h, w)
        assert (ref["score"], ref["end"]) == exhaustive(A, B, alphabet, S, g, h, w), (A, B, w)


def test_clip_rule():
    for (m, n, w), want in {(400, 150, 16): (166, 150), (150, 400, 16): (150, 166), (10, 10, 0): (10, 10),
                            (10, 11, 0): (10, 10), (1, 500, 3): (1, 4), (500, 1, 3): (4, 1), (7, 9, 2): (7, 9),
                            (7, 9, 100): (7, 9), (300, 290, 8): (298, 290)}.items():
        assert XB.clip(m, n, w) == want
    for m in range(1, 9):
        for n in range(1, 9):
            for w in range(0, 9):
                me, ne = XB.clip(m, n, w)
                assert abs(me - ne) <= w and me <= m and ne <= n
                inband = [(i, j) for i in range(1, m + 1) for j in range(1, n + 1) if abs(i - j) <= w]
                assert max(i for i, _ in inband) == me and max(j for _, j in inband) == ne


@pytest.mark.parametrize("name", [k for k in ER.SHAPES if k not in ("late_zero", "single_1000x3000")])
def test_full_band_is_the_unbanded_extension(name):
    """w = max(m, n): every cell is in band, nothing is clipped, and the result is extend_reference's."""
    set_name, make = ER.SHAPES[name]
    alphabet, S, g, h = ER.score_set(set_name)
    A, B = make()
    w = max(len(A), len(B))
    ref, want = XB.extend_band_reference(A, B, alphabet, S, g, h, w), ER.extend_reference(A, B, alphabet, S, g, h)
    for key in ("score", "end", "stop", "global_score", "best", "ops"):
        assert ref[key] == want[key], key
    v = want["valid"]
    assert np.array_equal(ref["valid"], v) and np.array_equal(ref["H"][v], want["H"][v])
    assert np.array_equal(ref["byte"][v], want["byte"][v])


@pytest.mark.parametrize("name", list(XB.CASES))
def test_named_cases(name):
    A, B, alphabet, S, g, h, w, ref = XB.case(name)
    _check_alignment(A, B, alphabet, S, g, h, w, ref)
    if name in XB.KNOWN:
        score, end, cigar, gs = XB.KNOWN[name]
        assert (ref["score"], ref["end"], XB.cigar_of(ref["ops"])) == (score, end, cigar)
        assert gs is ... or ref["global_score"] == gs
    assert ((ref["m_eff"], ref["n_eff"]) != (len(A), len(B))) == (name in XB.CLIPPED)
    if name in XB.CLIPPED:
        assert (ref["m_eff"], ref["n_eff"]) == XB.CLIPPED[name]
    if name in ("upper_edge_w64", "lower_edge_w64"):  # on the band's edge, in the stripe of rows 129..192
        assert abs(ref["end"][0] - ref["end"][1]) == w == 64 and 129 <= ref["end"][0] <= 192
        assert (len(A), len(B)) == (400, 400)
    if name == "outside_69_w64":  # the unbanded extension takes the diagonal the band excludes
        un = ER.extend_reference(A, B, alphabet, S, g, h)
        assert (un["score"], un["end"]) == (265, (203, 272))
    if name == "all_negative_w16":
        assert ref["best"] < 0
    if name in ("best_zero_w8", "zero_borders_w16"):
        assert ref["best"] == 0
    if name == "corner_on_edge_300x290_w10":
        assert ref["global_score"] is not None and abs(len(A) - len(B)) == w
    if name == "single_1000_w100":
        assert (len(A), len(B)) == (1000, 1000) and ref["score"] > 1000 and ref["end"][0] > 640


def test_batches_are_mixed():
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    w = XB.BATCH_BAND
    refs = [XB.extend_band_reference(a, b, alphabet, S, g, h, w) for a, b in XB.batch_pairs()]
    for (a, b), ref in zip(XB.batch_pairs(), refs):
        _check_alignment(a, b, alphabet, S, g, h, w, ref)
    assert [r["end"] for r in refs] == [(180, 180), (40, 40), (0, 0), (77, 77), (1, 1)]
    assert [r["global_score"] is None for r in refs] == [False, True, False, False, True]
    assert refs[3]["score"] == refs[3]["global_score"] == 154
    As, ref_b = XB.shared_b_batch()
    rs_ = [XB.extend_band_reference(a, ref_b, alphabet, S, g, h, w) for a in As]
    assert [r["end"] for r in rs_] == [(70, 70), (130, 130), (5, 5), (0, 0), (300, 300)]
    assert [r["global_score"] is None for r in rs_] == [True, True, True, True, True]
