"""The X-drop yardstick (tests/xdrop_reference.py) checked on the CPU: against a plain triple loop that restates the
contract of include/msa.h at msa_extend_align_xdrop cell by cell, against the banded yardstick for xdrop < 0, on the
values a prototype of the rule gave, and on the row-major tie the GPU test uses (found again here by exhaustion)."""
import itertools

import numpy as np
import pytest

import extend_band_reference as XB
import xdrop_reference as XD

INF = 10 ** 9


def _plain(A, B, alphabet, S, g, h, w, xdrop):
    """(score, end, D) by loops over cells: banded Gotoh on the clipped pair, then the stopping rule, then the first
    row-major maximum over the cells with i + j <= D."""
    m, n = XB.clip(len(A), len(B), w)
    a = [alphabet.index(c) for c in A[:m]]
    b = [alphabet.index(c) for c in B[:n]]
    H = [[-INF] * (n + 1) for _ in range(m + 1)]
    E = [[-INF] * (n + 1) for _ in range(m + 1)]
    F = [[-INF] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, min(n, w) + 1):
        H[0][j] = -h - g * j
    for i in range(1, min(m, w) + 1):
        H[i][0] = -h - g * i
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if abs(i - j) > w:
                continue
            E[i][j] = max(H[i][j - 1] - g - h, E[i][j - 1] - g)
            F[i][j] = max(H[i - 1][j] - g - h, F[i - 1][j] - g)
            H[i][j] = max(H[i - 1][j - 1] + int(S[a[i - 1]][b[j - 1]]), E[i][j], F[i][j])
    ad = [-INF] * (m + n + 1)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if abs(i - j) <= w:
                ad[i + j] = max(ad[i + j], H[i][j])
    D, best = m + n, 0
    for d in range(2, m + n + 1):
        best = max(best, ad[d])
        if xdrop >= 0 and best - max(ad[d - 1], ad[d]) > xdrop:
            D = d
            break
    top, end = -INF, None
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if abs(i - j) <= w and i + j <= D and H[i][j] > top:
                top, end = H[i][j], (i, j)
    return (top, end, D) if top > 0 else (0, (0, 0), D)


@pytest.mark.parametrize("sset", ["dna", "unit", "asym", "zero"])
def test_against_the_triple_loop(sset):
    alphabet, S, g, h = XB.score_set(sset)
    rng = np.random.default_rng(len(sset))
    stops = 0
    for _ in range(150):
        m, n = (int(x) for x in rng.integers(1, 13, 2))
        w = int(rng.integers(0, 5))
        L = int(rng.integers(0, min(m, n) + 1))  # a common prefix, so that something positive exists to drop from
        P = XB.rs(rng, L)
        A, B = P + XB.rs(rng, m - L), P + XB.rs(rng, n - L)
        for xdrop in (-1, 0, 1, 2, 4, 9):
            r = XD.xdrop_reference(A, B, alphabet, S, g, h, w, xdrop)
            assert (r["score"], r["end"], r["diagonals"]) == _plain(A, B, alphabet, S, g, h, w, xdrop), (A, B, w, xdrop)
            assert r["dropped"] == (r["diagonals"] < r["m_eff"] + r["n_eff"])
            assert XB.rescore(A, B, r["end"], r["ops"], alphabet, S, g, h, w) == r["score"]
            stops += r["dropped"]
    # (the rule fired often enough for the comparison to mean something; with free gaps, "zero", H rarely declines)
    assert stops >= 20


@pytest.mark.parametrize("name", ["random_300x290_w8", "similar_150_w0", "clip_rows_400x150_w16", "all_negative_w16",
                                  "best_zero_w8", "upper_edge_w64"])
def test_never_stopping_is_the_banded_yardstick(name):
    A, B, alphabet, S, g, h, w, ref = XB.case(name)
    for xdrop in (-1, -(2 ** 31), 2 ** 30):
        r = XD.xdrop_reference(A, B, alphabet, S, g, h, w, xdrop, band_ref=ref)
        for key in ("score", "end", "stop", "global_score", "best", "walk_ops", "ops"):
            assert r[key] == ref[key], (key, xdrop)
        assert r["diagonals"] == ref["m_eff"] + ref["n_eff"] and not r["dropped"] and r["delta"] is None
        assert (r["live"] == ref["valid"]).all() and r["byte"] is ref["byte"]


@pytest.mark.parametrize("name", list(XD.STOPS))
def test_prototype_values(name):
    A, B, alphabet, S, g, h, w, ref = XD.stop_case(name)
    for xdrop, (score, end, D, dropped) in XD.STOPS[name][3].items():
        r = XD.xdrop_reference(A, B, alphabet, S, g, h, w, xdrop, band_ref=ref)
        assert (r["score"], r["end"], r["diagonals"], r["dropped"]) == (score, end, D, dropped), xdrop
        assert (r["global_score"] is None) == dropped
        if dropped:
            assert r["delta"] > xdrop
            # one less would not have stopped here: D is the FIRST anti-diagonal at which the rule fires
            assert XD.stop_diagonal(r["a"], r["delta"])[0] > D
    # termination changes the answer on the islands, and only there
    assert name != "islands_w32" or XD.xdrop_reference(A, B, alphabet, S, g, h, w, 10, band_ref=ref)["score"] < \
        ref["score"]


def test_one_diagonal_rule_would_fire_at_once():
    """Why the rule looks at two anti-diagonals: on a perfect match the odd ones hold gap cells only."""
    A, B, alphabet, S, g, h, w, ref = XD.stop_case("prefix40_w16")
    a = XD.diagonal_maxima(ref)
    assert a[2] == 2 and a[2] - a[3] >= g + h   # one anti-diagonal: stops at d = 3 for every xdrop below the gap open
    assert a[2] - max(a[2], a[3]) == 0          # two: goes on


def _tie_property(r, c1, c2):
    w, H, live = r["w"], r["H"], r["live"]
    (i1, j1), (i2, j2) = c1, c2
    return (r["end"] == c1 and r["score"] > 0 and live[i1, j1 - i1 + w] and live[i2, j2 - i2 + w]
            and H[i1, j1 - i1 + w] == H[i2, j2 - i2 + w] == r["score"] and i1 < i2 and i1 + j1 > i2 + j2)


def test_row_major_tie():
    A, B, alphabet, S, g, h, w, xdrop, c1, c2 = XD.row_major_tie()
    r = XD.xdrop_reference(A, B, alphabet, S, g, h, w, xdrop)
    assert _tie_property(r, c1, c2)
    assert c1[0] + c1[1] <= r["diagonals"] and c2[0] + c2[1] <= r["diagonals"]
    # no pair of shorter sequences over three symbols has such a tie under this scoring and band
    for m, n in itertools.product(range(1, 5), repeat=2):
        for a in itertools.product(b"ACG", repeat=m):
            for b in itertools.product(b"ACG", repeat=n):
                q = XD.xdrop_reference(bytes(a), bytes(b), alphabet, S, g, h, w, xdrop)
                Hv = np.where(q["live"], q["H"], XD.NEG)
                for i2, c in np.argwhere(Hv == q["best"]):
                    assert not _tie_property(q, q["end"], (int(i2), int(c + i2 - w))), (a, b)
