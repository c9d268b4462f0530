"""Host side of the scored global alignment entries (msa_nw_align_scored, msa_nw_align_batch_scored,
api.nw_align / api.nw_align_batch with match / mismatch / alphabet / matrix): the argument errors, which come before
any device call (without a GPU a valid call is MSA_ERR_NODEV, so any other status was decided on the host), and
which library entry each argument combination reaches.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

ARG, ALPHABET, NODEV, UNSUPPORTED = -1, -2, -4, -5
A, B = b"ACGTACGTAC", b"ACGTTCGTA"
DNA = np.array([[2, -3, -3, -3], [-3, 2, -3, -3], [-3, -3, 2, -3], [-3, -3, -3, 2]], dtype=np.int8)


def _i64(*v):
    return np.array(v, dtype=np.int64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _single(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, band=-1):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc = C.c_int32()
    return LB.lib().msa_nw_align_scored(a, len(a), b, len(b), alphabet, n_sym, None if sub is None else _p(sub),
                                        gap_open, gap_extend, band, C.byref(sc), None, 0)


def _batch(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, band=-1):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc = np.zeros(1, dtype=np.int32)
    off, m, n = _i64(0), _i64(len(a)), _i64(len(b))
    return LB.lib().msa_nw_align_batch_scored(a, len(a), b, len(b), 1, _p(off), _p(m), _p(off), _p(n), alphabet,
                                              n_sym, None if sub is None else _p(sub), gap_open, gap_extend, band,
                                              _p(sc), None, 0, None)


def test_new_symbols_exported():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    assert LB.NW_SCORED == 6
    for name in ("msa_plan_create_scored", "msa_nw_align_scored", "msa_nw_align_batch_scored"):
        assert name in LB.EXPORTED
        assert hasattr(L, name), f"libmsa.so does not export {name}"


@pytest.mark.parametrize("call", [_single, _batch], ids=["single", "batch"])
def test_entry_argument_errors(call):
    big = np.zeros((9, 9), dtype=np.int8)
    assert call(b"ACGA", 4, DNA) == ARG                      # a duplicate symbol
    assert call(b"", 0, DNA) == ARG                          # n_sym 0
    assert call(b"ACGTNRYKM", 9, big) == ARG                 # n_sym 9
    assert call(None, 4, DNA) == ARG                         # no alphabet
    assert call(b"ACGT", 4, None) == ARG                     # no matrix
    assert call(b"ACGT", 4, DNA, a=b"ACGNACGT") == ALPHABET  # a symbol of A outside the alphabet
    assert call(b"ACGT", 4, DNA, b=b"ACGTTCGTX") == ALPHABET  # ... of B
    assert call(b"ACGT", 4, DNA, gap_open=1, gap_extend=2) == UNSUPPORTED
    assert call(b"ACGT", 4, DNA, gap_open=1, gap_extend=-1) == UNSUPPORTED
    assert call(b"ACGT", 4, DNA, band=0) == ARG              # |m - n| = 1 > band
    # the gap and band rules come before the symbols are looked at, as in msa_nw_align
    assert call(b"ACGT", 4, DNA, a=b"ACGNACGT", b=b"ACGTACGT", gap_open=1, gap_extend=2) == UNSUPPORTED


def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_api_argument_errors():
    from cse305_parallel_sequence_alignment_amd import api

    for f, a, b in ((api.nw_align, A, B), (api.nw_align_batch, [A], [B])):
        with pytest.raises(ValueError):
            f(a, b, matrix=DNA)                                  # matrix without alphabet
        with pytest.raises(ValueError):
            f(a, b, alphabet=b"ACGT", matrix=DNA, match=2)       # matrix with match
        with pytest.raises(ValueError):
            f(a, b, alphabet=b"ACGT", matrix=DNA, mismatch=-3)
        with pytest.raises(ValueError):
            f(a, b, alphabet=b"ACGT")                            # alphabet without matrix
        with pytest.raises(ValueError):
            f(a, b, alphabet=b"ACG", matrix=DNA)                 # not len(alphabet) x len(alphabet)
        assert _status(lambda: f(a, b, alphabet=b"ACGA", matrix=DNA)) == ARG
        assert _status(lambda: f(a, b, alphabet=b"", matrix=np.zeros((0, 0), dtype=np.int8))) == ARG
        assert _status(lambda: f(a, b, alphabet=b"ACGTNRYKM", matrix=np.zeros((9, 9), dtype=np.int8))) == ARG
        assert _status(lambda: f(a, b, alphabet=b"ACG", matrix=DNA[:3, :3])) == ALPHABET  # T is outside
        assert _status(lambda: f(a, b, alphabet=b"ACGT", matrix=DNA, gap_open=1, gap_extend=2)) == UNSUPPORTED
        assert _status(lambda: f(a, b, match=2, mismatch=-3, gap_open=1, gap_extend=2)) == UNSUPPORTED
        assert _status(lambda: f(a, b, match=128)) == UNSUPPORTED
    # match / mismatch build the alphabet from the sequences: a ninth symbol is the ALPHABET status
    nine = b"ACGTNRYKM"
    assert _status(lambda: api.nw_align(nine, nine[2:], match=2)) == ALPHABET
    assert _status(lambda: api.nw_align_batch([nine[:5]], [nine[4:]], mismatch=-1)) == ALPHABET


def test_no_device_status():
    """Without a GPU a valid scored call returns MSA_ERR_NODEV (no fallback)."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    n = C.c_int(0)
    if LB.lib().msa_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    assert _single(b"ACGT", 4, DNA) == NODEV
    assert _batch(b"ACGT", 4, DNA) == NODEV


class _Recorder:
    """Stands in for the library handle: every entry records its name and arguments and returns MSA_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0

        return entry


def test_which_entry_runs(monkeypatch):
    from cse305_parallel_sequence_alignment_amd import _lib, api

    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    # no new argument: today's calls, with today's arguments
    api.nw_align(A, B, gap_open=4, gap_extend=1, band=7)
    api.nw_align_batch([A], [B], gap_open=4, gap_extend=1, band=7)
    assert [c[0] for c in rec.calls] == ["msa_nw_align", "msa_nw_align_batch"]
    name, args = rec.calls[0]
    assert args[:7] == (A, len(A), B, len(B), 4, 1, 7) and len(args) == 10
    assert len(rec.calls[1][1]) == 16
    rec.calls.clear()
    # match and / or mismatch: the scored entry, alphabet = the symbols in first-seen order, A then B
    api.nw_align(b"GATTACA", b"GCATN", mismatch=-3)
    name, args = rec.calls[0]
    assert name == "msa_nw_align_scored"
    assert args[4] == b"GATCN" and args[5] == 5
    S = np.ctypeslib.as_array(C.cast(args[6], C.POINTER(C.c_int8)), shape=(25,)).reshape(5, 5)
    assert (S == np.where(np.eye(5, dtype=bool), 1, -3)).all()
    rec.calls.clear()
    api.nw_align_batch([b"GA", b"TT"], b"CAG", match=2)  # all As, then the shared B
    name, args = rec.calls[0]
    assert name == "msa_nw_align_batch_scored" and args[9] == b"GATC" and args[10] == 4
    S = np.ctypeslib.as_array(C.cast(args[11], C.POINTER(C.c_int8)), shape=(16,)).reshape(4, 4)
    assert (S == np.where(np.eye(4, dtype=bool), 2, 0)).all()
    rec.calls.clear()
    # alphabet + matrix: passed through
    api.nw_align(A, B, alphabet=b"ACGT", matrix=DNA.tolist(), traceback=False)
    name, args = rec.calls[0]
    assert name == "msa_nw_align_scored" and args[4] == b"ACGT" and args[5] == 4 and args[11] is None
    S = np.ctypeslib.as_array(C.cast(args[6], C.POINTER(C.c_int8)), shape=(16,)).reshape(4, 4)
    assert (S == DNA).all()
