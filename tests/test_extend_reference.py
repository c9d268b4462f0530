"""The NW_EXTEND yardstick (tests/extend_reference.py) against two independent statements, on the CPU: (a) a plain
triple-loop Gotoh under the global borders with the end-cell rule spelled out, and (b) the definition by exhaustion --
the best global score (nw_scored_reference) over every pair of prefixes A[:i], B[:j], floored at 0, the end cell being
the first such (i, j) in row-major order.  Under +2 / -3, an asymmetric table, unit scores with free gaps (g = h = 0:
the borders are 0 and tie with the empty result) and a 24-symbol table."""
import itertools

import numpy as np
import pytest

import extend_reference as ER
import nw_reference as R
import nw_scored_reference as RS
import wide_reference as WR

NINF = float("-inf")
SCORINGS = {"dna": RS.SCORE_SETS["dna"], "asym": RS.SCORE_SETS["asym"], "zero": ER.ZERO,
            "protein24": (ER.AL24, WR.table32()[:24, :24], 2, 9)}


def _rand(rng, n, alphabet, k=None):
    return WR.rs32(rng, n, alphabet[:k or len(alphabet)])


def brute_extend(A, B, alphabet, S, g, h):
    """(H, score, end cell, H(m, n)) of the contract include/msa.h documents at msa_extend_align, cell by cell in plain
    Python (exact -inf), the candidates scanned in row-major order with a strict >."""
    a, b = ER.codes(A, alphabet), ER.codes(B, alphabet)
    m, n = len(a), len(b)
    op = g + h
    H = [[NINF] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, n + 1):
        H[0][j] = E[0][j] = -h - g * j
    for i in range(1, m + 1):
        H[i][0] = F[i][0] = -h - g * i
    best, end = NINF, None
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            E[i][j] = max(H[i][j - 1] - op, E[i][j - 1] - g)
            F[i][j] = max(H[i - 1][j] - op, F[i - 1][j] - g)
            H[i][j] = max(H[i - 1][j - 1] + int(S[a[i - 1]][b[j - 1]]), E[i][j], F[i][j])
            if H[i][j] > best:
                best, end = H[i][j], (i, j)
    if best <= 0:
        best, end = 0, (0, 0)
    return H, best, end, H[m][n]


def exhaustive(A, B, alphabet, S, g, h):
    """(score, end cell): max(0, the best global score of A[:i] against B[:j]), the first such (i, j) in row-major
    order -- (0, 0) when nothing is positive."""
    best, end = 0, (0, 0)
    for i in range(1, len(A) + 1):
        for j in range(1, len(B) + 1):
            sc = ER.global_reference(A[:i], B[:j], alphabet, S, g, h)["score"]
            if sc > best:
                best, end = sc, (i, j)
    return best, end


def _check_alignment(A, B, alphabet, S, g, h, ref):
    m, n = len(A), len(B)
    assert ER.rescore(A, B, ref["end"], ref["ops"], alphabet, S, g, h) == ref["score"]
    assert ref["global_score"] == ER.global_reference(A, B, alphabet, S, g, h)["score"]
    assert ref["global_score"] <= ref["best"] or (m, n) == ref["end"]
    if ref["score"] == 0:
        assert (ref["end"], ref["stop"], ref["ops"]) == ((0, 0), (0, 0), b"") and ref["best"] <= 0
    else:
        assert ref["score"] == ref["best"] > 0 and 1 <= ref["end"][0] <= m and 1 <= ref["end"][1] <= n
        assert ref["stop"][0] == 0 or ref["stop"][1] == 0


@pytest.mark.parametrize("scoring", ["dna", "asym", "zero"])
def test_every_small_pair(scoring):
    """Every pair of sequences over 2 symbols with m, n <= 4, and over 3 symbols with m, n <= 3 (about 2,400 pairs),
    against both statements; a sample of them at up to 6 x 6."""
    alphabet, S, g, h = SCORINGS[scoring]
    seqs = {k: [bytes(t) for L in range(1, top + 1) for t in itertools.product(alphabet[:k], repeat=L)]
            for k, top in ((2, 4), (3, 3))}
    pairs = [(a, b) for k in seqs for a in seqs[k] for b in seqs[k]]
    rng = np.random.default_rng(5)
    pairs += [(_rand(rng, int(rng.integers(1, 7)), alphabet, 3), _rand(rng, int(rng.integers(1, 7)), alphabet, 3))
              for _ in range(60)]
    for A, B in pairs:
        ref = ER.extend_reference(A, B, alphabet, S, g, h)
        _, score, end, hmn = brute_extend(A, B, alphabet, S, g, h)
        assert (ref["score"], ref["end"], ref["global_score"]) == (score, end, hmn), (A, B)
        assert (ref["score"], ref["end"]) == exhaustive(A, B, alphabet, S, g, h), (A, B)
        _check_alignment(A, B, alphabet, S, g, h, ref)


@pytest.mark.parametrize("scoring", list(SCORINGS))
def test_random_pairs_against_triple_loop(scoring):
    """80 random pairs per scoring up to 40 x 40 (half of them with a common prefix, so that many results are not
    empty), H cell by cell and the result; the first 10 against the definition by exhaustion too."""
    alphabet, S, g, h = SCORINGS[scoring]
    rng = np.random.default_rng(880 + len(scoring))
    for k in range(80):
        m, n = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        if k < 10:
            m, n = min(m, 12), min(n, 12)
        A, B = _rand(rng, m, alphabet), _rand(rng, n, alphabet)
        if k % 2:
            L = int(rng.integers(1, min(m, n) + 1))
            B = A[:L] + B[L:]
        ref = ER.extend_reference(A, B, alphabet, S, g, h)
        H, score, end, hmn = brute_extend(A, B, alphabet, S, g, h)
        assert (ref["score"], ref["end"], ref["global_score"]) == (score, end, hmn), (A, B)
        want = R.to_band(np.array(H).astype(np.int64), ref["w"], fill=R.NEG)
        v = ref["valid"]
        assert v.sum() == m * n and np.array_equal(ref["H"][v], want[v])
        if k < 10:
            assert (ref["score"], ref["end"]) == exhaustive(A, B, alphabet, S, g, h), (A, B)
        _check_alignment(A, B, alphabet, S, g, h, ref)


@pytest.mark.parametrize("name", [k for k in ER.SHAPES if k != "single_1000x3000"])
def test_named_shapes(name):
    set_name, make = ER.SHAPES[name]
    alphabet, S, g, h = ER.score_set(set_name)
    A, B = make()
    ref = ER.extend_reference(A, B, alphabet, S, g, h)
    _check_alignment(A, B, alphabet, S, g, h, ref)
    assert name in ER.KNOWN
    assert (ref["score"], ref["end"], ER.cigar_of(ref["ops"])) == ER.KNOWN[name]
    w, H = ref["w"], ref["H"]
    for (i, j) in ER.TIES.get(name, []):
        assert H[i, j - i + w] == ref["score"] and (i, j) > ref["end"]
    if name in ("tie_two_stripes", "tie_two_lanes"):
        (i, _), = ER.TIES[name]
        assert ((i - 1) // 64 != (ref["end"][0] - 1) // 64) == (name == "tie_two_stripes")
    if name == "first_stripe":  # a positive best where whole stripes hold negative values only
        rows = np.where(ref["valid"], H, R.NEG)[65:]
        assert rows.max() < 0
    if name == "all_negative":
        assert ref["best"] < 0
    if name in ("best_zero", "zero_borders"):
        assert ref["best"] == 0
    if name == "zero_borders":  # the borders are 0 as well: -h - g j with g = h = 0 (the band form keeps the top one)
        assert (g, h) == (0, 0) and H[0, w + 5] == 0
    if name == "m65_random":
        assert ref["best"] < 0
    if name == "late_zero":
        assert (len(A), len(B)) == (200, 5000) and (ref["end"][0] - 1) // 64 == 1


def test_single_1000x3000():
    set_name, make = ER.SHAPES["single_1000x3000"]
    A, B = make()
    ref = ER.extend_reference(A, B, *ER.score_set(set_name))
    assert (len(A), len(B), ref["end"]) == (1000, 3000, (700, 700)) and ref["score"] > 1000 > 0 > ref["global_score"]


def test_batches_are_mixed():
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = ER.batch_pairs()
    assert ([len(a) for a, _ in pairs], [len(b) for _, b in pairs]) == (ER.BATCH_MS, ER.BATCH_NS)
    refs = [ER.extend_reference(a, b, alphabet, S, g, h) for a, b in pairs]
    for (a, b), ref in zip(pairs, refs):
        _check_alignment(a, b, alphabet, S, g, h, ref)
    assert [r["end"] for r in refs] == [(180, 180), (40, 40), (0, 0), (77, 77), (1, 1)]
    assert refs[3]["score"] == refs[3]["global_score"] == 154
    As, ref_b = ER.shared_b_batch()
    ends = [ER.extend_reference(a, ref_b, alphabet, S, g, h)["end"] for a in As]
    assert ends == [(70, 70), (130, 130), (5, 5), (0, 0), (300, 300)]


def test_eight_symbols_use_every_code():
    A, B, alphabet, S, g, h = ER.eight_symbols()
    ref = ER.extend_reference(A, B, alphabet, S, g, h)
    _check_alignment(A, B, alphabet, S, g, h, ref)
    (ei, ej) = ref["end"]
    assert ref["score"] > 0 and set(A[:ei]) == set(B[:ej]) == set(alphabet) and len(alphabet) == 8
    assert not np.array_equal(np.asarray(S), np.asarray(S).T)
    # ... and a transposed table changes the result (a kernel that swaps the roles of A and B cannot pass)
    assert ER.extend_reference(A, B, alphabet, np.asarray(S).T, g, h)["score"] != ref["score"]


def test_protein32_extends():
    for k in range(3):
        A, B, alphabet, S, g, h = ER.protein32(k)
        assert (len(A), len(B), len(alphabet)) == (150, 330, 24)
        ref = ER.extend_reference(A, B, alphabet, S, g, h)
        _check_alignment(A, B, alphabet, S, g, h, ref)
        assert ref["end"][0] >= 80 and ref["end"][1] >= 80 and ref["score"] > 500
