"""The NW_OVERLAP yardstick (tests/overlap_reference.py) against independent restatements, on the CPU: a plain
triple-loop Gotoh under the two zero borders with the end-cell rule spelled out, and the definition by exhaustion --
the best global score (nw_scored_reference) over every piece of A against every piece of B that starts on the top or
left border and ends on the last row or column, floored at 0."""
import numpy as np
import pytest

import alphabet8 as A8
import nw_reference as R
import nw_scored_reference as RS
import overlap_reference as OR

NINF = float("-inf")
SCORINGS = {"dna": RS.SCORE_SETS["dna"], "unit": OR.UNIT, "table8": (A8.AL8, A8.TABLE8, A8.G8, A8.H8)}


def _rand(rng, n, alphabet):
    return A8.rs8(rng, n) if len(alphabet) == 8 else R.rs(rng, n)


def brute_overlap(A, B, alphabet, S, g, h):
    """(H, score, end cell) of the contract include/msa.h documents at msa_overlap_align, cell by cell in plain
    Python (exact -inf), the candidates scanned in the order the rule names them."""
    a, b = OR.codes(A, alphabet), OR.codes(B, alphabet)
    m, n = len(a), len(b)
    op = g + h
    H = [[NINF] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    for j in range(n + 1):
        H[0][j] = 0
    for i in range(1, m + 1):
        H[i][0] = 0
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            E[i][j] = max(H[i][j - 1] - op, E[i][j - 1] - g)
            F[i][j] = max(H[i - 1][j] - op, F[i - 1][j] - g)
            H[i][j] = max(H[i - 1][j - 1] + int(S[a[i - 1]][b[j - 1]]), E[i][j], F[i][j])
    best_r, j_r = max((H[m][j], -j) for j in range(1, n + 1))
    best_c, i_c = max((H[i][n], -i) for i in range(1, m + 1))
    best = max(best_r, best_c)
    end = (m, -j_r) if best_r >= best_c else (-i_c, n)
    if best <= 0:
        best, end = 0, (m, 0)
    return H, best, end


def exhaustive_score(A, B, alphabet, S, g, h):
    m, n = len(A), len(B)
    starts = [(0, j) for j in range(n + 1)] + [(i, 0) for i in range(1, m + 1)]
    ends = [(m, j) for j in range(n + 1)] + [(i, n) for i in range(m)]
    best = 0
    for i0, j0 in starts:
        for i1, j1 in ends:
            if i1 > i0 and j1 > j0:
                best = max(best, RS.nw_scored_reference(A[i0:i1], B[j0:j1], alphabet, S, g, h, walk=False)["score"])
    return best


def _check_alignment(A, B, alphabet, S, g, h, ref):
    m, n = len(A), len(B)
    assert OR.borders_ok(ref, m, n)
    assert OR.rescore(A, B, ref["beg"], ref["end"], ref["ops"], alphabet, S, g, h) == ref["score"]
    if ref["score"] == 0:
        assert (ref["beg"], ref["end"], ref["ops"]) == ((m, 0), (m, 0), b"")
    else:
        assert ref["score"] > 0 and ref["end"][0] > ref["beg"][0] and ref["end"][1] > ref["beg"][1]


@pytest.mark.parametrize("scoring", list(SCORINGS))
def test_against_the_definition(scoring):
    """About 40 random pairs in all (14 per scoring), m, n <= 12."""
    alphabet, S, g, h = SCORINGS[scoring]
    rng = np.random.default_rng(770 + len(scoring))
    for _ in range(14):
        m, n = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        A, B = _rand(rng, m, alphabet[:4]), _rand(rng, n, alphabet[:4])
        if len(alphabet) == 8:
            A, B = A8.rs8(rng, m), A8.rs8(rng, n)
        ref = OR.overlap_reference(A, B, alphabet, S, g, h)
        assert ref["score"] == exhaustive_score(A, B, alphabet, S, g, h), (A, B)
        H, score, end = brute_overlap(A, B, alphabet, S, g, h)
        assert (ref["score"], ref["end"]) == (score, end), (A, B)
        _check_alignment(A, B, alphabet, S, g, h, ref)


@pytest.mark.parametrize("scoring", list(SCORINGS))
@pytest.mark.parametrize("shape", [(65, 70), (40, 97), (30, 12), (1, 9), (7, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_triple_loop(shape, scoring):
    m, n = shape
    alphabet, S, g, h = SCORINGS[scoring]
    rng = np.random.default_rng(1000 * m + n)
    A, B = (A8.rs8(rng, m), A8.rs8(rng, n)) if len(alphabet) == 8 else (R.rs(rng, m), R.rs(rng, n))
    ref = OR.overlap_reference(A, B, alphabet, S, g, h)
    H, score, end = brute_overlap(A, B, alphabet, S, g, h)
    assert (ref["score"], ref["end"]) == (score, end)
    want = R.to_band(np.array(H).astype(np.int64), ref["w"], fill=R.NEG)
    v = ref["valid"]
    assert v.sum() == m * n
    assert np.array_equal(ref["H"][v], want[v])
    _check_alignment(A, B, alphabet, S, g, h, ref)


@pytest.mark.parametrize("name", [k for k in OR.SHAPES if k != "single_1000x3000"])
def test_named_shapes(name):
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    A, B = OR.SHAPES[name]()
    m, n = len(A), len(B)
    ref = OR.overlap_reference(A, B, alphabet, S, g, h)
    _check_alignment(A, B, alphabet, S, g, h, ref)
    if name in OR.KNOWN:
        assert (ref["score"], ref["beg"], ref["end"], OR.cigar_of(ref["ops"])) == OR.KNOWN[name]
    if name == "empty":
        u = OR.overlap_reference(A, B, *OR.UNIT)
        assert max(u["best_r"], u["best_c"]) == 0  # a zero-score tie, not a negative best
        assert (u["score"], u["beg"], u["end"], OR.cigar_of(u["ops"])) == OR.KNOWN_UNIT_EMPTY
    if name == "a_in_b":
        assert (ref["beg"], ref["end"]) == ((0, 300), (100, 400))
    if name == "b_in_a":
        assert (ref["beg"], ref["end"]) == ((300, 0), (400, 100)) and ref["best_c"] > ref["best_r"]
    if name == "dovetail_ba":
        assert ref["best_c"] > ref["best_r"] and (ref["end"][0] - 1) // 64 == 1 and (m + 63) // 64 == 4
    if name == "corner":
        assert ref["best_r"] == ref["best_c"] and (ref["j_r"], ref["i_c"]) == (n, m)
    if name == "tie_row_col":
        assert ref["best_r"] == ref["best_c"] == 120 and (ref["i_c"], ref["j_r"]) == (60, 60)
    if name == "tie_col_twice":
        w, H = ref["w"], ref["H"]
        assert H[130, n - 130 + w] == H[270, n - 270 + w] == 180 and ref["best_c"] > ref["best_r"]
        assert (130 - 1) // 64 != (270 - 1) // 64
    if name == "late_5000":
        assert ref["end"] == (60, 5000) and ref["beg"] == (0, 4940)
    if name == "n1":
        assert ref["end"][1] in (0, 1)


def test_batches_are_mixed():
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = OR.batch_pairs()
    assert ([len(a) for a, _ in pairs], [len(b) for _, b in pairs]) == (OR.BATCH_MS, OR.BATCH_NS)
    refs = [OR.overlap_reference(a, b, alphabet, S, g, h) for a, b in pairs]
    for (a, b), ref in zip(pairs, refs):
        _check_alignment(a, b, alphabet, S, g, h, ref)
    assert (refs[0]["beg"], refs[0]["end"]) == ((0, 10), (200, 210))            # contained
    assert (refs[1]["beg"], refs[1]["end"]) == ((90, 0), (150, 60))             # dovetail, the last row
    assert (refs[2]["beg"], refs[2]["end"]) == ((0, 50), (40, 90))              # dovetail, the last column
    assert refs[3]["score"] == 0 and refs[3]["end"] == (64, 0)                  # empty
    As, ref_b = OR.shared_b_batch()
    ends = [OR.overlap_reference(a, ref_b, alphabet, S, g, h)["end"] for a in As]
    assert ends[:4] == [(120, 70), (80, 300), (90, 190), (330, 300)]


def test_eight_symbols_reach_code_7():
    A, B, alphabet, S, g, h = OR.eight_symbols()
    ref = OR.overlap_reference(A, B, alphabet, S, g, h)
    _check_alignment(A, B, alphabet, S, g, h, ref)
    # (the table's mean is positive: the best overlap is longer than the planted one, whatever it is it holds code 7)
    k = alphabet[7:8]
    (bi, bj), (ei, ej) = ref["beg"], ref["end"]
    assert k in A[bi:ei] and k in B[bj:ej] and ref["score"] > 0
    assert not np.array_equal(np.asarray(S), np.asarray(S).T)
    # ... and a transposed table changes the result (a kernel that swaps the roles of A and B cannot pass)
    assert OR.overlap_reference(A, B, alphabet, np.asarray(S).T, g, h)["score"] != ref["score"]


def test_protein32_is_a_dovetail():
    for k in range(3):
        A, B, alphabet, S, g, h = OR.protein32(k)
        assert (len(A), len(B), len(alphabet)) == (150, 330, 24)
        ref = OR.overlap_reference(A, B, alphabet, S, g, h)
        _check_alignment(A, B, alphabet, S, g, h, ref)
        assert ref["end"][0] == 150 and ref["beg"][1] == 0 and ref["score"] > 500
