"""The NW_FIT yardstick (tests/fit_reference.py) against independent restatements, on the CPU: a plain triple-loop
Gotoh with the fit borders, a brute force over every substring of the reference with the global yardstick, and the
global yardstick on the substring the fit alignment chose."""
import numpy as np
import pytest

import fit_reference as FR
import nw_reference as R
import nw_scored_reference as RS

NINF = float("-inf")


def brute_fit_h(A, B, alphabet, S, g, h):
    """H of the recurrence include/msa.h documents at msa_fit_align, cell by cell in plain Python (exact -inf)."""
    a, b = RS.codes(A, alphabet), RS.codes(B, alphabet)
    m, n = len(a), len(b)
    op = g + h
    H = [[NINF] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    for j in range(n + 1):
        H[0][j] = 0
    for i in range(1, m + 1):
        H[i][0] = F[i][0] = -h - g * i
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            E[i][j] = max(H[i][j - 1] - op, E[i][j - 1] - g)
            F[i][j] = max(H[i - 1][j] - op, F[i - 1][j] - g)
            H[i][j] = max(H[i - 1][j - 1] + int(S[a[i - 1]][b[j - 1]]), E[i][j], F[i][j])
    return H


@pytest.mark.parametrize("set_name", list(RS.SCORE_SETS))
@pytest.mark.parametrize("shape", [(65, 70), (40, 97), (30, 12), (1, 9), (7, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_triple_loop(shape, set_name):
    m, n = shape
    alphabet, S, g, h = RS.SCORE_SETS[set_name]
    rng = np.random.default_rng(1000 * m + n)
    A, B = RS.set_input(set_name, R.rs(rng, m), R.rs(rng, n))
    ref = FR.fit_reference(A, B, alphabet, S, g, h)
    H = np.array(brute_fit_h(A, B, alphabet, S, g, h))
    row = H[m, 1:]
    assert ref["score"] == int(row.max()) and ref["end_j"] == int(np.argmax(row)) + 1
    want = R.to_band(H.astype(np.int64), ref["w"], fill=R.NEG)
    v = ref["valid"]
    assert v.sum() == m * n
    assert np.array_equal(ref["H"][v], want[v])
    _check_alignment(A, B, alphabet, S, g, h, ref)


def _check_alignment(A, B, alphabet, S, g, h, ref):
    beg, end = ref["beg_j"], ref["end_j"]
    assert 0 <= beg <= end <= len(B) and 1 <= end
    assert ref["stop"][1] == beg and (ref["stop"][0] == 0 or beg == 0)
    assert ref["ops"].endswith(b"I" * ref["stop"][0])  # the border gap is 'I' only
    assert FR.rescore(A, B, beg, end, ref["ops"], alphabet, S, g, h) == ref["score"]
    if end > beg:
        assert RS.nw_scored_reference(A, B[beg:end], alphabet, S, g, h, walk=False)["score"] == ref["score"]
    else:
        assert ref["score"] == -h - g * len(A)


@pytest.mark.parametrize("set_name", list(RS.SCORE_SETS))
def test_against_every_substring(set_name):
    """The best global score over every substring B[x:y], y > x, and -h - g m for the empty one."""
    alphabet, S, g, h = RS.SCORE_SETS[set_name]
    rng = np.random.default_rng(77)
    for _ in range(12):
        m, n = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        A, B = R.rs(rng, m), R.rs(rng, n)
        best = -h - g * m
        for x in range(n):
            for y in range(x + 1, n + 1):
                best = max(best, RS.nw_scored_reference(A, B[x:y], alphabet, S, g, h, walk=False)["score"])
        ref = FR.fit_reference(A, B, alphabet, S, g, h)
        assert ref["score"] == best, (A, B)
        _check_alignment(A, B, alphabet, S, g, h, ref)


@pytest.mark.parametrize("name", [k for k in FR.SHAPES if k != "q1000_r3000"])
def test_named_shapes(name):
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    A, B = FR.SHAPES[name]()
    ref = FR.fit_reference(A, B, alphabet, S, g, h)
    _check_alignment(A, B, alphabet, S, g, h, ref)
    if name in FR.KNOWN:
        assert (ref["score"], ref["beg_j"], ref["end_j"], FR.cigar_of(ref["ops"])) == FR.KNOWN[name]
    if name == "end_at_n":
        assert ref["end_j"] == len(B) and ref["beg_j"] == len(B) - len(A)
    if name == "end_at_1":
        assert ref["stop"] == (0, 1)
        u = FR.fit_reference(A, B, *FR.UNIT)
        assert (u["score"], u["beg_j"], u["end_j"], FR.cigar_of(u["ops"])) == FR.KNOWN_UNIT_END_AT_1
    if name == "overhang_25I":
        assert ref["stop"] == (25, 0)
    if name == "q100_r5000_late":
        assert ref["beg_j"] == 4700 and ref["end_j"] == 4800
    if name == "q100_in_r700":
        assert (ref["beg_j"], ref["end_j"]) == (333, 433)


def test_eight_symbols_reach_code_7():
    A, B, alphabet, S, g, h = FR.eight_symbols()
    ref = FR.fit_reference(A, B, alphabet, S, g, h)
    _check_alignment(A, B, alphabet, S, g, h, ref)
    k = alphabet[7:8]
    assert k in A and k in B[ref["beg_j"]:ref["end_j"]]
    assert not np.array_equal(np.asarray(S), np.asarray(S).T)
    # ... and a transposed table changes the result (a kernel that swaps the roles of A and B cannot pass)
    assert FR.fit_reference(A, B, alphabet, np.asarray(S).T, g, h)["score"] != ref["score"]
