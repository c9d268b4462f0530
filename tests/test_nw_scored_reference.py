"""The NW_SCORED yardstick (tests/nw_scored_reference.py) against independent restatements, on the CPU: a plain
triple-loop Gotoh for every score set, nw_reference under identity scoring, and the Levenshtein distance."""
import functools

import numpy as np
import pytest

import alphabet8 as A8
import nw_reference as R
import nw_scored_reference as RS

NINF = float("-inf")
# rows, columns, band of the brute-force shapes
BRUTE_SHAPES = [(65, 70, 8), (40, 37, -1), (130, 129, 3), (90, 90, 1)]


def brute_gotoh(A, B, alphabet, S, g, h, band):
    """H(m, n) of the recurrence include/msa.h documents, cell by cell in plain Python (exact -inf)."""
    return int(brute_gotoh_h(A, B, alphabet, S, g, h, band)[len(A)][len(B)])


def brute_gotoh_h(A, B, alphabet, S, g, h, band):
    """That recurrence's whole H, row-major (m + 1) x (n + 1), -inf outside the band."""
    a, b = RS.codes(A, alphabet), RS.codes(B, alphabet)
    m, n = len(a), len(b)
    w = max(m, n) if band < 0 else band
    op = g + h
    H = [[NINF] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, min(n, w) + 1):
        H[0][j] = -h - g * j
    for i in range(1, min(m, w) + 1):
        H[i][0] = -h - g * i
    for i in range(1, m + 1):
        for j in range(max(1, i - w), min(n, i + w) + 1):
            E[i][j] = max(H[i][j - 1] - op, E[i][j - 1] - g)
            F[i][j] = max(H[i - 1][j] - op, F[i - 1][j] - g)
            H[i][j] = max(H[i - 1][j - 1] + int(S[a[i - 1]][b[j - 1]]), E[i][j], F[i][j])
    return H


@functools.lru_cache(maxsize=None)
def _brute_input(m, n):
    rng = np.random.default_rng(1000 * m + n)
    return R.rs(rng, m), R.rs(rng, n)


@pytest.mark.parametrize("set_name", list(RS.SCORE_SETS))
@pytest.mark.parametrize("shape", BRUTE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_w{s[2]}")
def test_against_brute_force(shape, set_name):
    m, n, band = shape
    alphabet, S, g, h = RS.SCORE_SETS[set_name]
    A, B = RS.set_input(set_name, *_brute_input(m, n))
    ref = RS.nw_scored_reference(A, B, alphabet, S, g, h, band)
    assert ref["score"] == brute_gotoh(A, B, alphabet, S, g, h, band)
    assert RS.rescore(A, B, ref["ops"], alphabet, S, g, h, band) == ref["score"]


@pytest.mark.parametrize("gh", A8.EDGE_GH, ids=lambda t: f"g{t[0]}h{t[1]}")
@pytest.mark.parametrize("shape", A8.EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_w{s[2]}")
def test_edge_shapes_every_cell_against_brute_force(shape, gh):
    """The edge shapes of test_gpu_full_alphabet.py over eight symbols and the dense table: every in-band H cell,
    not only H(m, n), and the walk's ops rescored."""
    (m, n, band), (g, h) = shape, gh
    A, B = A8.edge_pair(m, n)
    ref = RS.nw_scored_reference(A, B, A8.AL8, A8.TABLE8, g, h, band)
    H = np.array(brute_gotoh_h(A, B, A8.AL8, A8.TABLE8, g, h, band))
    assert ref["score"] == int(H[m][n])
    want = R.to_band(np.where(np.isinf(H), R.NEG, H).astype(np.int64), ref["w"], fill=R.NEG)
    v = ref["valid"]
    assert v.sum() == sum(min(n, i + ref["w"]) - max(1, i - ref["w"]) + 1 for i in range(1, m + 1))
    assert np.array_equal(ref["H"][v], want[v])
    assert RS.rescore(A, B, ref["ops"], A8.AL8, A8.TABLE8, g, h, band) == ref["score"]


def test_titv_inputs_hold_n():
    """(the "titv" inputs really exercise the fifth code)"""
    A, B = RS.set_input("titv", *_brute_input(65, 70))
    assert b"N" in A and b"N" in B and set(A + B) <= set(b"ACGTN")


def test_asym_is_not_symmetric_in_effect():
    """A transposed table changes the result (so a kernel that swaps the roles of A and B cannot pass)."""
    alphabet, S, g, h = RS.SCORE_SETS["asym"]
    A, B = _brute_input(65, 70)
    assert RS.nw_scored_reference(A, B, alphabet, S, g, h, 8, walk=False)["score"] != \
        RS.nw_scored_reference(A, B, alphabet, S.T, g, h, 8, walk=False)["score"]


@pytest.mark.parametrize("name", ["random_65x70_w8", "random_300x290_w32", "ties_A400_A390_w16",
                                  "random_500x480_noband", "random_300x290_w32_g0h3"])
def test_identity_scoring_is_nw_reference(name):
    A, B, band, g, h = R.SMALL[name]()
    want = R.nw_reference(A, B, g, h, band)
    got = RS.nw_scored_reference(A, B, b"ACGT", RS.match_mismatch(b"ACGT", 1, 0), g, h, band)
    assert got["score"] == want["score"]
    assert got["ops"] == want["ops"] and got["stop"] == want["stop"]
    v = want["valid"]
    assert (got["valid"] == v).all()
    assert (got["byte"][v] == want["byte"][v]).all()
    assert (got["H"][v] == want["H"][v]).all()
    assert RS.rescore(A, B, got["ops"], b"ACGT", RS.match_mismatch(b"ACGT", 1, 0), g, h, band) == \
        R.rescore(A, B, want["ops"], g, h, band) == want["score"]


def levenshtein(A, B):
    a, b = np.frombuffer(A, dtype=np.uint8), np.frombuffer(B, dtype=np.uint8)
    prev = np.arange(len(b) + 1)
    for i in range(1, len(a) + 1):
        cur = np.empty_like(prev)
        cur[0] = i
        sub = np.minimum(prev[:-1] + (b != a[i - 1]), prev[1:] + 1)
        for j in range(1, len(b) + 1):  # (the insertion chain is sequential)
            cur[j] = min(sub[j - 1], cur[j - 1] + 1)
        prev = cur
    return int(prev[-1])


def test_edit_distance():
    A, B, _, _, _ = R.SMALL["random_300x290_w32"]()
    alphabet, S, g, h = RS.SCORE_SETS["edit"]
    d = levenshtein(A, B)
    assert d == 154
    assert RS.nw_scored_reference(A, B, alphabet, S, g, h, -1, walk=False)["score"] == -d
