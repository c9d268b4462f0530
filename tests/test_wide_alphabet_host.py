"""Host side of the 32-symbol entries (msa_plan_create_scored32, msa_nw_align_scored32, msa_nw_align_batch_scored32,
msa_fit_align32, msa_fit_align_batch32, api.* with max_symbols=32), and the yardstick tests/wide_reference.py itself:
the exports, the yardstick against the 8-code yardsticks and against a plain-Python Gotoh DP, the argument errors --
each decided before any device call (without a GPU a valid call is MSA_ERR_NODEV, so any other status was decided on
the host) -- and which library entry each argument combination reaches.  Nothing here needs a GPU; every comparison is
exact."""
import ctypes as C

import numpy as np
import pytest

import fit_reference as FR
import nw_reference as R
import nw_scored_reference as RS
import wide_reference as W

ARG, ALPHABET, NODEV, UNSUPPORTED = -1, -2, -4, -5
NEW = ("msa_plan_create_scored32", "msa_nw_align_scored32", "msa_nw_align_batch_scored32", "msa_fit_align32",
       "msa_fit_align_batch32")
P20 = np.ascontiguousarray(W.protein20(), dtype=np.int8)
A20, B20 = W.rs32(np.random.default_rng(70), 23, W.AL20), W.rs32(np.random.default_rng(71), 31, W.AL20)


def test_new_symbols_exported():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    for name in NEW:
        assert name in LB.EXPORTED
        assert hasattr(L, name), f"libmsa.so does not export {name}"


# ---- the yardstick ----------------------------------------------------------------------------------------------
def _same(got: dict, want: dict):
    assert got.keys() == want.keys()
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape and (got[k] == v).all(), k
        else:
            assert got[k] == v, k


@pytest.mark.parametrize("set_name", ["asym", "titv"])
def test_reference_equals_the_8_code_yardsticks(set_name):
    alphabet, S, g, h = RS.SCORE_SETS[set_name]
    rng = np.random.default_rng(81)
    A, B = RS.set_input(set_name, R.rs(rng, 150), R.rs(rng, 140))
    for band in (-1, 16):
        _same(W.nw_reference32(A, B, alphabet, S, g, h, band), RS.nw_scored_reference(A, B, alphabet, S, g, h, band))
    _same(W.fit_reference32(A[:60], B, alphabet, S, g, h), FR.fit_reference(A[:60], B, alphabet, S, g, h))
    assert RS.codes is not W.codes32 and FR.codes is RS.codes  # (the lookup is back in place)


def _seeded20():
    """A seeded asymmetric 20 x 20 table in [-9, 9] and gap costs."""
    return np.random.default_rng(72).integers(-9, 10, size=(20, 20)), 2, 3


def test_reference_equals_a_brute_force_dp():
    S, g, h = _seeded20()
    assert (S != S.T).any()
    m, n = len(A20), len(B20)
    assert (m, n) == (23, 31) and len(set(A20 + B20)) > 8
    H, E, F = W.gotoh_brute(A20, B20, W.AL20, S, g, h)
    ref = W.nw_reference32(A20, B20, W.AL20, S, g, h)
    assert ref["score"] == H[m][n]
    assert W.rescore32(A20, B20, ref["ops"], W.AL20, S, g, h) == ref["score"]
    full = np.array([[x for x in row] for row in H], dtype=np.int64)
    assert (ref["H"][ref["valid"]] == R.to_band(full, ref["w"])[ref["valid"]]).all()
    # fit: the first maximum of row m over columns 1..n
    H, E, F = W.gotoh_brute(A20, B20, W.AL20, S, g, h, fit=True)
    fit = W.fit_reference32(A20, B20, W.AL20, S, g, h)
    best = max(H[m][1:])
    assert (fit["score"], fit["end_j"]) == (best, H[m][1:].index(best) + 1)
    assert W.fit_rescore32(A20, B20, fit["beg_j"], fit["end_j"], fit["ops"], W.AL20, S, g, h) == fit["score"]


# ---- the entries' argument errors -------------------------------------------------------------------------------
def _i64(*v):
    return np.array(v, dtype=np.int64)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _lib():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    return LB.lib()


def _nw(alphabet, n_sym, sub, a=A20, b=B20, gap_open=5, gap_extend=2, band=-1):
    sc = C.c_int32()
    return _lib().msa_nw_align_scored32(a, len(a), b, len(b), alphabet, n_sym, _p(sub), gap_open, gap_extend, band,
                                        C.byref(sc), None, 0)


def _nw_batch(alphabet, n_sym, sub, a=A20, b=B20, gap_open=5, gap_extend=2, band=-1):
    sc = np.zeros(1, dtype=np.int32)
    off, m, n = _i64(0), _i64(len(a)), _i64(len(b))
    return _lib().msa_nw_align_batch_scored32(a, len(a), b, len(b), 1, _p(off), _p(m), _p(off), _p(n), alphabet, n_sym,
                                              _p(sub), gap_open, gap_extend, band, _p(sc), None, 0, None)


def _fit(alphabet, n_sym, sub, a=A20, b=B20, gap_open=5, gap_extend=2, band=-1):
    sc, bj, ej = C.c_int32(), C.c_int64(), C.c_int64()
    return _lib().msa_fit_align32(a, len(a), b, len(b), alphabet, n_sym, _p(sub), gap_open, gap_extend, C.byref(sc),
                                  C.byref(bj), C.byref(ej), None, 0)


def _fit_batch(alphabet, n_sym, sub, a=A20, b=B20, gap_open=5, gap_extend=2, band=-1):
    sc = np.zeros(1, dtype=np.int32)
    be = np.zeros(2, dtype=np.int64)
    off, m, n = _i64(0), _i64(len(a)), _i64(len(b))
    return _lib().msa_fit_align_batch32(a, len(a), b, len(b), 1, _p(off), _p(m), _p(off), _p(n), alphabet, n_sym,
                                        _p(sub), gap_open, gap_extend, _p(sc), _p(be), None, 0, None)


CALLS = {"nw": _nw, "nw_batch": _nw_batch, "fit": _fit, "fit_batch": _fit_batch}


@pytest.mark.parametrize("kind", list(CALLS))
def test_entry_argument_errors(kind):
    call = CALLS[kind]
    big = np.zeros((33, 33), dtype=np.int8)
    assert call(b"", 0, P20) == ARG                                          # n_sym 0
    assert call(W.AL32 + b"f", 33, big) == ARG                               # n_sym 33
    assert call(W.AL20[:19] + W.AL20[:1], 20, P20) == ARG                    # a duplicate symbol
    assert call(None, 20, P20) == ARG                                        # no alphabet
    assert call(W.AL20, 20, None) == ARG                                     # no matrix
    assert call(W.AL20, 20, P20, a=A20[:5] + b"B" + A20[6:]) == ALPHABET     # a symbol of A outside the 20
    assert call(W.AL20, 20, P20, b=B20 + b"*") == ALPHABET                   # ... of B
    assert call(W.AL20, 20, P20, gap_open=1, gap_extend=2) == UNSUPPORTED
    # the gap rule comes before the symbols are looked at
    assert call(W.AL20, 20, P20, a=A20[:5] + b"B" + A20[6:], gap_open=1, gap_extend=2) == UNSUPPORTED
    if kind.startswith("nw"):
        assert call(W.AL20, 20, P20, band=7) == ARG                          # |m - n| = 8 > band
        # ... and the band before them too
        assert call(W.AL20, 20, P20, a=A20[:5] + b"B" + A20[6:], band=7) == ARG
    # the 8-symbol twins keep their limit
    nine = np.zeros((9, 9), dtype=np.int8)
    sc = C.c_int32()
    assert _lib().msa_nw_align_scored(A20, len(A20), B20, len(B20), W.AL20[:9], 9, _p(nine), 5, 2, -1, C.byref(sc),
                                      None, 0) == ARG


def _gpu_present():
    n = C.c_int(0)
    return _lib().msa_device_count(C.byref(n)) == 0 and n.value > 0


@pytest.mark.parametrize("kind", list(CALLS))
def test_no_device_status(kind):
    """Without a GPU a valid 20-symbol call returns MSA_ERR_NODEV (no fallback), and so does a 4-symbol one."""
    if _gpu_present():
        pytest.skip("a GPU is present")
    assert CALLS[kind](W.AL20, 20, P20) == NODEV
    assert CALLS[kind](W.AL20[:8], 8, np.zeros((8, 8), dtype=np.int8), a=W.AL20[:8], b=W.AL20[:8]) == NODEV


def test_plan_create_scored32_arguments():
    """What msa_plan_create_scored32 decides before it asks for a device."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    arrs = [(C.c_int64 * 1)(v) for v in (40, 40, 0, 0)]
    tab = np.zeros((32, 32), dtype=np.int8)
    h = C.c_void_p()

    def create(alg, sub):
        d = LB.PlanDesc(alg=alg, cells=LB.CELLS_DIR, match=1, mismatch=0, gap_open=3, gap_extend=1, start_type=-1,
                        band=-1, track_end=0, single=1, n_pairs=1, m=arrs[0], n=arrs[1], a_off=arrs[2], b_off=arrs[3])
        return L.msa_plan_create_scored32(C.byref(d), _p(sub), C.byref(h))

    for alg in (LB.SW_LINEAR, LB.SW_AFFINE, LB.NW_BANDED, LB.REF_GOTOH, LB.PARTIAL, LB.NW_ALIGN):
        assert create(alg, tab) == UNSUPPORTED
    assert create(LB.NW_SCORED, None) == ARG and create(LB.NW_FIT, None) == ARG
    assert L.msa_plan_create_scored32(None, _p(tab), C.byref(h)) == ARG


# ---- api: which entry runs --------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the library handle: every entry records its name and arguments and returns MSA_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0

        return entry


def _table(ptr, k):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int8)), shape=(k * k,)).reshape(k, k)


def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_which_entry_runs(monkeypatch):
    from cse305_parallel_sequence_alignment_amd import _lib, api

    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    twelve_a, twelve_b, twelve = b"MKVLAAGIW", b"KMWDEFHV", b"MKVLAGIWDEFH"  # 12 distinct symbols, first seen
    assert len(set(twelve_a + twelve_b)) == len(twelve) == 12
    # alphabet + matrix with max_symbols=32: the *32 entry, both passed through
    api.nw_align(A20, B20, alphabet=W.AL20, matrix=P20, max_symbols=32, band=9)
    api.nw_align_batch([A20], [B20], alphabet=W.AL20, matrix=P20, max_symbols=32)
    api.fit_align(A20, B20, alphabet=W.AL20, matrix=P20, max_symbols=32)
    api.fit_align_batch([A20], B20, alphabet=W.AL20, matrix=P20, max_symbols=32)
    assert [c[0] for c in rec.calls] == ["msa_nw_align_scored32", "msa_nw_align_batch_scored32", "msa_fit_align32",
                                         "msa_fit_align_batch32"]
    for (name, args), at in zip(rec.calls, (4, 9, 4, 9)):
        assert args[at] == W.AL20 and args[at + 1] == 20 and (_table(args[at + 2], 20) == P20).all(), name
    assert rec.calls[0][1][:4] == (A20, len(A20), B20, len(B20)) and rec.calls[0][1][9] == 9
    assert [len(c[1]) for c in rec.calls] == [13, 19, 14, 19]  # (the twins' argument counts)
    rec.calls.clear()
    # match over 12 distinct symbols: the first-seen alphabet and a 12 x 12 table
    api.nw_align(twelve_a, twelve_b, match=3, max_symbols=32)
    api.fit_align_batch([twelve_a], [twelve_b], mismatch=-2, max_symbols=32)
    (n0, a0), (n1, a1) = rec.calls
    assert n0 == "msa_nw_align_scored32" and a0[4] == twelve and a0[5] == 12
    assert (_table(a0[6], 12) == np.where(np.eye(12, dtype=bool), 3, 0)).all()
    assert n1 == "msa_fit_align_batch32" and a1[9] == twelve and a1[10] == 12
    assert (_table(a1[11], 12) == np.where(np.eye(12, dtype=bool), 1, -2)).all()
    rec.calls.clear()
    # none of the four scoring arguments: +1 / 0 over the sequences' symbols, through the *32 entry
    api.nw_align(twelve_a, twelve_b, max_symbols=32)
    name, args = rec.calls[0]
    assert name == "msa_nw_align_scored32" and args[4] == twelve
    assert (_table(args[6], 12) == np.eye(12, dtype=np.int8)).all()
    rec.calls.clear()
    # the default: today's entries with today's arguments
    api.nw_align(b"ACGTACGTAC", b"ACGTTCGTA", gap_open=4, gap_extend=1, band=7)
    api.nw_align(b"GATTACA", b"GCATN", mismatch=-3)
    api.nw_align_batch([b"GA", b"TT"], b"CAG", match=2)
    api.fit_align(b"GATTACA", b"GCATN")
    api.fit_align_batch([b"GA"], b"CAG")
    assert [c[0] for c in rec.calls] == ["msa_nw_align", "msa_nw_align_scored", "msa_nw_align_batch_scored",
                                         "msa_fit_align", "msa_fit_align_batch"]
    assert rec.calls[0][1][:7] == (b"ACGTACGTAC", 10, b"ACGTTCGTA", 9, 4, 1, 7) and len(rec.calls[0][1]) == 10
    assert rec.calls[1][1][4] == b"GATCN" and rec.calls[1][1][5] == 5 and len(rec.calls[1][1]) == 13
    assert rec.calls[2][1][9] == b"GATC" and len(rec.calls[2][1]) == 19
    assert len(rec.calls[3][1]) == 14 and len(rec.calls[4][1]) == 19


def test_api_max_symbols_errors():
    from cse305_parallel_sequence_alignment_amd import api

    for f, a, b in ((api.nw_align, A20, B20), (api.nw_align_batch, [A20], [B20]), (api.fit_align, A20, B20),
                    (api.fit_align_batch, [A20], [B20])):
        with pytest.raises(ValueError):
            f(a, b, max_symbols=16)
        with pytest.raises(ValueError):
            f(a, b, alphabet=W.AL20, matrix=P20, max_symbols=0)
    # 33 distinct symbols: the ALPHABET status, decided before any library call
    many = W.AL32 + b"f"
    assert len(set(many)) == 33
    assert _status(lambda: api.nw_align(many, many[::-1], match=2, max_symbols=32)) == ALPHABET
    assert _status(lambda: api.nw_align(many, many[::-1], max_symbols=32)) == ALPHABET
    assert _status(lambda: api.fit_align_batch([many[:20]], [many[15:]], mismatch=-1, max_symbols=32)) == ALPHABET
    # the default keeps its 8: a ninth symbol is the ALPHABET status
    assert _status(lambda: api.nw_align(W.AL20[:9], W.AL20[:9], match=2)) == ALPHABET
