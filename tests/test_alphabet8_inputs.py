"""The conditions under which test_gpu_full_alphabet.py cannot pass vacuously, checked on the CPU.

A GPU test over eight symbols proves something about the profile bytes of codes 4-7 only if those bytes decide its
expected result.  So: every entry of the dense table changes the NW_SCORED yardstick's result on the test's input;
every symbol of every equality-scored input changes the oracle's result when it stops matching; and the host-entry
inputs hand code 7 to a symbol that both sequences hold, at a stripe's first or last row and inside the first 16
columns.  No condition has an exception list."""
import numpy as np
import pytest

import alphabet8 as A8
import nw_scored_reference as RS

OTHER = ord("#")  # a byte outside AL8


def test_nw_scored_input_feels_every_table_entry():
    """Each of the 64 entries, moved by +1 and by -1, changes the score or bits 0-1 of an in-band byte."""
    A, B = A8.pair8(5, 300, 290)
    base = RS.nw_scored_reference(A, B, A8.AL8, A8.TABLE8, A8.G8, A8.H8, 32, walk=False)
    v = base["valid"]
    unnoticed = []
    for x in range(8):
        for y in range(8):
            for d in (1, -1):
                S = A8.TABLE8.copy()
                S[x, y] += d
                r = RS.nw_scored_reference(A, B, A8.AL8, S, A8.G8, A8.H8, 32, walk=False)
                if r["score"] == base["score"] and not (v & ((r["byte"] & 3) != (base["byte"] & 3))).any():
                    unnoticed.append((x, y, d))
    assert unnoticed == []
    assert RS.nw_scored_reference(A, B, A8.AL8, A8.TABLE8.T, A8.G8, A8.H8, 32, walk=False)["score"] != base["score"]


def test_tables():
    assert A8.TABLE8.shape == (8, 8) and A8.TABLE8.min() == -3 and A8.TABLE8.max() == 4
    assert (A8.TABLE8 != A8.TABLE8.T).any()
    assert A8.TABLE8_WIDE.max() == 80 and A8.TABLE8_WIDE.min() >= -128
    assert 80 + 2 * 1 + 2 <= 127 < 80 + 2 * 20 + 10  # band_kernel's profile byte S + 2g + h
    for perm in A8.PERMS:
        assert sorted(perm) == list(range(8))
        Sp = A8.permuted(perm, S=A8.TABLE8)
        assert all(Sp[perm[x]][perm[y]] == A8.TABLE8[x][y] for x in range(8) for y in range(8))
    assert A8.PERMS[0][0] == 7 and A8.PERMS[0][7] == 0


def _gaps(text):
    """Where main_alignment's two printed lines hold a gap (not the letters: they change with B trivially)."""
    l1, l2 = text.split("\n")[5:7]
    return [k for k, c in enumerate(l1) if c == "-"], [k for k, c in enumerate(l2) if c == "-"]


def _result(oracle, kind, A, B):
    if kind in ("sw", "swa"):
        o = oracle.sw(A, B, *((2, -1, 1, 1) if kind == "sw" else (2, -3, 5, 2)), want_h=True)
        return o["score"], o["H"].tobytes()
    if kind in ("banded32", "banded"):
        w = 32 if kind == "banded32" else max(len(A), len(B))
        score, H = oracle.banded_ref(A, B, w, 1.0, 2.0, want_h=True)
        i, j = np.indices(H.shape)
        return score, H[np.abs(i - j) <= w].tobytes()
    if kind == "tables":
        return [T.tobytes() for T in oracle.subproblem_tables(A, B, -1, 1.0, 2.0)[:3]]
    if kind == "partial":
        T, R = oracle.partial_tables(A, B, 1.0, 2.0, 1, 1)
        return [x.tobytes() for x in T + R]
    text, score = oracle.main_alignment_text(A, B, 1.0, 2.0)
    return score, _gaps(text)


@pytest.mark.parametrize("name", list(A8.INPUTS))
def test_every_symbol_decides_the_expected_result(oracle, name):
    """Replacing every s of B by a byte that occurs in neither sequence changes the oracle's result, for every
    symbol s of the alphabet in use (in a batch: the result of some pair)."""
    kind, k, _ = A8.INPUTS[name]
    pairs = A8.named(name)
    pairs = pairs if isinstance(pairs, list) else [pairs]
    assert set(b"".join(a + b for a, b in pairs)) == set(A8.AL8[:k])
    base = {}
    for s in A8.AL8[:k]:
        for p, (A, B) in enumerate(pairs):
            if s not in B:
                continue
            if p not in base:
                base[p] = _result(oracle, kind, A, B)
            if _result(oracle, kind, A, B.replace(bytes([s]), bytes([OTHER]))) != base[p]:
                break
        else:
            pytest.fail(f"{name}: symbol {chr(s)} decides nothing")


@pytest.mark.parametrize("name", list(A8.HOST_SHAPES))
def test_code7_is_handed_out(name):
    """msa_encode_pair's eighth code goes to a symbol of both sequences that sits at a stripe's first or last row
    (lane 0 or 63 of the 64-row stripe) and among the first 16 columns (the first code read of a lane)."""
    rows, cols = A8.host_run_order(name)
    codes = A8.first_seen(rows, cols)
    assert sorted(codes.values()) == list(range(8))
    s = [c for c, k in codes.items() if k == 7][0]
    assert s in rows and s in cols
    assert any(rows[i - 1] == s and (i - 1) % 64 in (0, 63) for i in range(1, len(rows) + 1))
    assert s in cols[:16]


def test_helpers():
    rng = np.random.default_rng(3)
    x = A8.rs8(rng, 500, 7)
    assert set(x) == set(A8.AL7)
    assert (A8.enc8(A8.AL8) == np.arange(8)).all()
    assert A8.first_seen(b"KAN", b"YRT") == {65: 0, 67: 1, 71: 2, 84: 3, ord("K"): 4, ord("N"): 5, ord("Y"): 6,
                                             ord("R"): 7}
    with pytest.raises(ValueError):
        A8.first_seen(A8.AL8, b"X")
    A, B = A8.chunked8()
    assert len(A) == 9001 and abs(len(A) - len(B)) <= 64 and set(A) == set(B) == set(A8.AL8)
