"""The profile yardstick (tests/profile_reference.py) against the table yardsticks and a plain-Python DP, and the
conditions the GPU tests' inputs are meant to satisfy (test_gpu_profile.py), asserted here so that a degenerate input
cannot pass silently.  Nothing here needs a GPU."""
import numpy as np
import pytest

import profile_reference as PR
import wide_reference as W

MODES = PR.MODES


def _same(x, y, path=""):
    """Two yardstick dictionaries agree key by key (arrays element by element)."""
    assert type(x) is type(y) or (np.isscalar(x) and np.isscalar(y)), path
    if isinstance(x, dict):
        assert x.keys() == y.keys(), path
        for k in x:
            _same(x[k], y[k], f"{path}.{k}")
    elif isinstance(x, np.ndarray):
        assert x.shape == y.shape and x.dtype == y.dtype and (x == y).all(), path
    else:
        assert x == y, path


def _from_matrix(A, alphabet, S):
    from cse305_parallel_sequence_alignment_amd import api

    return api.profile_from_matrix(A, alphabet, S)


@pytest.mark.parametrize("mode", MODES)
def test_table_profile_equals_table_yardstick(mode):
    al, T = PR.alphabet_of(mode), PR.table_of(mode)
    rng = np.random.default_rng(7)
    cases = [PR.table_case(mode), (W.rs32(rng, 1, al), W.rs32(rng, 9, al)), (W.rs32(rng, 70, al), W.rs32(rng, 33, al))]
    for A, B in cases:
        P = _from_matrix(A, al, T)
        assert P.shape == (len(A), len(al)) and P.dtype == np.int8
        _same(PR.profile_reference(mode, P, B, al), PR.table_reference(mode, A, B, al, T))
    # the lookups are the yardsticks' own again afterwards
    import fit_reference as FR
    import nw_scored_reference as RS
    import sw_scored_reference as SS

    assert SS.codes32 is W.codes32 and RS.codes.__module__ == "nw_scored_reference" and FR.codes is RS.codes


def _cells(mode, ref, m, n):
    """(H, E finite, F finite) of a yardstick dictionary as (m+1) x (n+1) arrays over the interior."""
    if mode == "local":
        return ref["H"], None, None
    w = ref["w"]
    i, j = np.meshgrid(np.arange(m + 1), np.arange(n + 1), indexing="ij")
    return ref["H"][i, j - i + w], ref["efin"][i, j - i + w], ref["ffin"][i, j - i + w]


@pytest.mark.parametrize("mode", MODES)
def test_random_profiles_equal_the_brute_force_dp(mode):
    al = PR.alphabet_of(mode)
    rng = np.random.default_rng(11 + MODES.index(mode))
    for m, n, (go, ge) in ((1, 1, (5, 2)), (1, 13, (3, 1)), (17, 1, (3, 3)), (23, 31, (5, 2)), (40, 22, (2, 0))):
        P = rng.integers(-9, 12, size=(m, len(al)))
        B = W.rs32(rng, n, al)
        ref = PR.profile_reference(mode, P, B, al, go, ge)
        Hb, Eb, Fb = PR.profile_brute(mode, P, B, al, go, ge)
        H, efin, ffin = _cells(mode, ref, m, n)
        assert H[1:, 1:].tolist() == [row[1:] for row in Hb[1:]]
        if mode == "local":
            assert ref["E"][1:, 1:].tolist() == [row[1:] for row in Eb[1:]]
            assert ref["F"][1:, 1:].tolist() == [row[1:] for row in Fb[1:]]
            assert ref["score"] == max(max(row) for row in Hb)
        else:
            # without a band every interior E and F is finite: bits 2 and 3 of every interior byte are defined
            assert efin[1:, 1:].all() and ffin[1:, 1:].all()
            assert ref["score"] == (Hb[m][n] if mode == "global" else max(Hb[m][1:]))
        # the ops rescored under the profile give the score
        if mode == "local":
            if ref["score"] > 0:
                assert PR.rescore(mode, P, B, al, ref["ops"], beg=ref["beg"], go=go, ge=ge) == (ref["score"], ref["end"])
        elif mode == "global":
            assert PR.rescore(mode, P, B, al, ref["ops"], go=go, ge=ge) == ref["score"]
        else:
            assert PR.rescore(mode, P, B, al, ref["ops"], span=(ref["beg_j"], ref["end_j"]), go=go, ge=ge) == ref["score"]


def test_pad32():
    P = np.arange(-6, 6).reshape(3, 4)
    out = PR.pad32(P)
    assert out.shape == (3, 32) and out.dtype == np.int8 and (out[:, :4] == P).all() and not out[:, 4:].any()


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_table_case_input(mode):
    A, B = PR.table_case(mode)
    assert (len(A), len(B)) == (330, 300)
    ref = PR.table_reference(mode, A, B, PR.alphabet_of(mode), PR.table_of(mode))
    assert {b"M", b"I", b"D"} <= {bytes([c]) for c in ref["ops"]}


@pytest.mark.parametrize("mode", MODES)
def test_specific_case_input(mode):
    al = PR.alphabet_of(mode)
    P, B = PR.specific_case(mode)
    assert P.shape == (330, len(al)) and len(B) == 300 and -128 <= P.min() and P.max() <= 127
    # no 32 x 32 table reproduces the profile: a table has at most 32 distinct rows
    assert len(np.unique(P, axis=0)) > 32
    # ... and positions with the same best symbol carry different rows, inside the shifted run and outside it
    best = P.argmax(axis=1)
    for rows in (np.arange(150, 180), np.arange(0, 150)):
        c = np.bincount(best[rows]).argmax()
        same = rows[best[rows] == c]
        assert len(same) >= 2 and len(np.unique(P[same], axis=0)) == len(same)
    base = PR.specific_profile(910 + MODES.index(mode), 330, len(al))
    assert (best[150:180] == base.argmax(axis=1)[150:180] + 1).all() and (best[:150] == base.argmax(axis=1)[:150]).all()
    # B is an alignment with gaps of both kinds against the profile, and a positive local one
    loc = PR.profile_reference("local", P[:, :31], B, PR.AL31)
    assert loc["score"] > 0 and {b"M", b"I", b"D"} <= {bytes([c]) for c in loc["ops"]}
    ref = PR.profile_reference(mode, P, B, al)
    assert {b"M", b"I", b"D"} <= {bytes([c]) for c in ref["ops"]}
    # row r must be the row that scores row r: the profile rolled by one row gives another result (free ends let the
    # alignment move along with the rows: then the score stays and the cells differ)
    rolled = PR.profile_reference(mode, np.roll(P, 1, axis=0), B, al)
    assert PR.result_of(mode, rolled, 330, 300) != PR.result_of(mode, ref, 330, 300)
    assert (rolled["byte"] != ref["byte"]).any()
    # ... and so do two neighbouring rows swapped inside the aligned part
    sw = P.copy()
    sw[[200, 201]] = sw[[201, 200]]
    assert PR.profile_reference(mode, sw, B, al)["score"] != ref["score"]


@pytest.mark.parametrize("mode", MODES)
def test_batch_inputs(mode):
    al = PR.alphabet_of(mode)
    P, Bs = PR.batch_case(mode)
    assert len(P) == PR.BATCH_ROWS == 580 and [len(b) for b in Bs] == PR.BATCH_NS and {1, 64, 65} <= set(PR.BATCH_NS)
    assert (len(P) + 63) // 64 == 10   # ten stripes on an eight-wave workgroup
    if mode == "local":  # the unrelated sequence: an empty local result, next to a positive one
        empty = PR.profile_reference(mode, P, Bs[4], al)
        assert (empty["score"], empty["end"], empty["ops"]) == (0, (0, 0), b"")
        assert PR.profile_reference(mode, P, Bs[3], al)["score"] > 0
    Q, Cs = PR.slice_case(mode)
    assert Q is P and PR.SLICES[-1][0] + PR.SLICES[-1][1] == len(P) and [m for _, m in PR.SLICES] == [580, 64, 65]
    for (a, m), B in zip(PR.SLICES, Cs):
        ref = PR.profile_reference(mode, P[a:a + m], B, al)
        # the slice's own rows score it: against the rows one further on (or back) the result is another one (under
        # free ends the alignment may move with the rows), against the profile's first m rows the score is
        if m < len(P):
            b = a + 1 if a + m < len(P) else a - 1
            other = PR.profile_reference(mode, P[b:b + m], B, al)
            assert PR.result_of(mode, other, m, len(B)) != PR.result_of(mode, ref, m, len(B))
            assert PR.profile_reference(mode, P[:m], B, al)["score"] != ref["score"]


@pytest.mark.parametrize("mode", MODES)
def test_edge_inputs(mode):
    for m in PR.EDGE_MS:
        P, B = PR.edge_case(mode, m)
        assert (len(P), len(B)) == (m, 70)
        if mode == "local":
            assert PR.profile_reference(mode, P, B, PR.AL31)["score"] > 0


def test_all_positive_input():
    P, Bs = PR.all_positive_case()
    assert P.min() >= 1 and P.shape == (70, 31) and [len(b) for b in Bs] == [40, 90]


def test_end_cell_format_inputs():
    for L, score in ((516, 65532), (517, 65659)):
        P, B = PR.self127(L)
        assert max(0, int(P.max())) == 127 and min(len(P), len(B)) == L and 127 * L == score
        assert (127 * 516 < 65536) and (127 * 517 >= 65536)


@pytest.mark.parametrize("mode", MODES)
def test_extreme_input(mode):
    al = PR.alphabet_of(mode)
    P, B, cs = PR.extreme_case(mode)
    assert cs == list(range(8, 30 if mode == "local" else 32)) and PR.EXT_ROW0 >= 64
    b = W.codes32(B, al)
    ref = PR.profile_reference(mode, P, B, al)
    for t, c in enumerate(cs):
        r = PR.EXT_ROW0 + t
        assert P[r, c] == 127 and (P[r] == -128).sum() == 1 and c in b and c // 4 >= 2
        # each extreme decides cells: with this 127 made -2, or this -128 made 127 (a lost sign), bytes change
        for v in (127, -128):
            Q = P.copy()
            Q[r][Q[r] == v] = -2 if v == 127 else 127
            alt = PR.profile_reference(mode, Q, B, al)
            assert (alt["byte"] != ref["byte"]).any(), (c, v)
    # every byte lane of the profile dwords 2..7 carries a 127 and a -128 somewhere
    lanes127 = {int(np.flatnonzero(P[PR.EXT_ROW0 + t] == 127)[0]) for t in range(len(cs))}
    lanes128 = {int(np.flatnonzero(P[PR.EXT_ROW0 + t] == -128)[0]) for t in range(len(cs))}
    assert lanes127 == lanes128 == set(cs)
    # the alignment takes 127s and avoids -128s
    assert ref["score"] > 127 * (len(cs) // 2)
