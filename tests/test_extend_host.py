"""Host side of the extension alignment entries (msa_extend_align, msa_extend_align_batch, their *32 twins,
api.extend_align / api.extend_align_batch): the exported symbols, the argument errors, which come before any device
call (without a GPU a valid call is MSA_ERR_NODEV, so any other status was decided on the host), and which library
entry the api functions reach with which scoring.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

ARG, ALPHABET, NODEV, UNSUPPORTED = -1, -2, -4, -5
A, B = b"ACGTACGTAC", b"ACGTTCGTAGGTT"
DNA = np.array([[2, -3, -3, -3], [-3, 2, -3, -3], [-3, -3, 2, -3], [-3, -3, -3, 2]], dtype=np.int8)


def _i64(*v):
    return np.array(v, dtype=np.int64)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _single(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, m=None, n=None, entry="msa_extend_align"):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc, gs = C.c_int32(), C.c_int32()
    end = np.zeros(2, dtype=np.int64)
    return getattr(LB.lib(), entry)(a, len(a) if m is None else m, b, len(b) if n is None else n, alphabet, n_sym,
                                    _p(sub), gap_open, gap_extend, C.byref(sc), _p(end), C.byref(gs), None, 0)


def _batch(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, m=None, n=None, a_off=0, b_off=0, n_pairs=1,
           end=True, gscore=True, cigars=False, cigar_off=False, entry="msa_extend_align_batch"):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc, gs = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    en = np.zeros(2, dtype=np.int64)
    ao, bo = _i64(a_off), _i64(b_off)
    mm, nn = _i64(len(a) if m is None else m), _i64(len(b) if n is None else n)
    cig = C.create_string_buffer(256) if cigars else None
    coff = np.zeros(2, dtype=np.int64) if cigar_off else None
    return getattr(LB.lib(), entry)(a, 0 if a is None else len(a), b, 0 if b is None else len(b), n_pairs, _p(ao),
                                    _p(mm), _p(bo), _p(nn), alphabet, n_sym, _p(sub), gap_open, gap_extend, _p(sc),
                                    _p(en) if end else None, _p(gs) if gscore else None, cig, 256 if cigars else 0,
                                    _p(coff))


def _single32(*a, **k):
    return _single(*a, entry="msa_extend_align32", **k)


def _batch32(*a, **k):
    return _batch(*a, entry="msa_extend_align_batch32", **k)


def test_new_symbols_exported():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    assert LB.NW_EXTEND == 10
    for name in ("msa_extend_align", "msa_extend_align_batch", "msa_extend_align32", "msa_extend_align_batch32"):
        assert name in LB.EXPORTED
        assert hasattr(L, name), f"libmsa.so does not export {name}"


@pytest.mark.parametrize("call", [_single, _batch, _single32, _batch32], ids=["single", "batch", "single32", "batch32"])
def test_entry_argument_errors(call):
    wide = call in (_single32, _batch32)
    assert call(b"ACGA", 4, DNA) == ARG                      # a duplicate symbol
    assert call(b"", 0, DNA) == ARG                          # n_sym 0
    if wide:
        al33 = bytes(range(65, 98))
        assert call(al33, 33, np.zeros((33, 33), dtype=np.int8)) == ARG      # n_sym 33
    else:
        assert call(b"ACGTNRYKM", 9, np.zeros((9, 9), dtype=np.int8)) == ARG  # n_sym 9
    assert call(None, 4, DNA) == ARG                         # no alphabet
    assert call(b"ACGT", 4, None) == ARG                     # no matrix
    assert call(b"ACGT", 4, DNA, a=b"ACGNACGT") == ALPHABET  # a symbol of A outside the alphabet
    assert call(b"ACGT", 4, DNA, b=b"ACGTTCGTX") == ALPHABET  # ... of B
    assert call(b"ACGT", 4, DNA, gap_open=1, gap_extend=2) == UNSUPPORTED
    assert call(b"ACGT", 4, DNA, gap_open=1, gap_extend=-1) == UNSUPPORTED
    assert call(b"ACGT", 4, DNA, m=0) == ARG                 # an empty A
    assert call(b"ACGT", 4, DNA, n=0) == ARG                 # an empty B
    # the gap rule comes before the symbols are looked at, as in msa_overlap_align
    assert call(b"ACGT", 4, DNA, a=b"ACGNACGT", gap_open=1, gap_extend=2) == UNSUPPORTED


def test_single_entry_null_sequences():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc = C.c_int32()
    f = LB.lib().msa_extend_align
    assert f(None, 4, B, len(B), b"ACGT", 4, _p(DNA), 5, 2, C.byref(sc), None, None, None, 0) == ARG
    assert f(A, len(A), None, 4, b"ACGT", 4, _p(DNA), 5, 2, C.byref(sc), None, None, None, 0) == ARG
    assert f(A, (1 << 26) + 1, B, len(B), b"ACGT", 4, _p(DNA), 5, 2, C.byref(sc), None, None, None, 0) == ARG


def test_batch_entry_argument_errors():
    ok = dict(alphabet=b"ACGT", n_sym=4, sub=DNA)
    assert _batch(**ok, n_pairs=0) == ARG
    assert _batch(**ok, end=False) == ARG                    # the end cells are the entry's result
    assert _batch(**ok, cigars=True, cigar_off=False) == ARG  # cigars without cigar_off
    assert _batch(**ok, a_off=1) == ARG                      # A's range leaves the buffer
    assert _batch(**ok, b_off=-1) == ARG
    assert _batch(**ok, n=len(B) + 1) == ARG                 # B's range leaves the buffer
    assert _batch(**ok, a=None, m=4) == ARG
    assert _batch(**ok, b=None, n=4) == ARG


def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_api_argument_errors():
    from cse305_parallel_sequence_alignment_amd import api

    for f, a, b in ((api.extend_align, A, B), (api.extend_align_batch, [A], [B]), (api.extend_align_batch, [A], B)):
        with pytest.raises(ValueError):
            f(a, b, max_symbols=16)                              # 8 or 32
        with pytest.raises(ValueError):
            f(a, b, matrix=DNA)                                  # matrix without alphabet
        with pytest.raises(ValueError):
            f(a, b, alphabet=b"ACGT", matrix=DNA, match=2)       # matrix with match
        with pytest.raises(ValueError):
            f(a, b, alphabet=b"ACGT")                            # alphabet without matrix
        with pytest.raises(ValueError):
            f(a, b, alphabet=b"ACG", matrix=DNA)                 # not len(alphabet) x len(alphabet)
        assert _status(lambda: f(a, b, alphabet=b"ACGA", matrix=DNA)) == ARG
        assert _status(lambda: f(a, b, alphabet=b"ACG", matrix=DNA[:3, :3])) == ALPHABET  # T is outside
        assert _status(lambda: f(a, b, alphabet=b"ACGT", matrix=DNA, gap_open=1, gap_extend=2)) == UNSUPPORTED
        assert _status(lambda: f(a, b, gap_open=1, gap_extend=2)) == UNSUPPORTED
        assert _status(lambda: f(a, b, match=128)) == UNSUPPORTED
    nine = b"ACGTNRYKM"
    assert _status(lambda: api.extend_align(nine, nine[2:])) == ALPHABET
    with pytest.raises(ValueError):
        api.extend_align_batch([A, A], [B])                      # Bs as long as As, or one bytes object
    assert api.extend_align_batch([], B) == []                   # an empty batch
    with pytest.raises(ValueError):
        api.extend_align_batch([], B, max_symbols=9)             # ... still checks max_symbols first


def test_no_device_status():
    """Without a GPU a valid call returns MSA_ERR_NODEV (no fallback).  (With one, the GPU tests cover these calls.)"""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    n = C.c_int(0)
    if LB.lib().msa_device_count(C.byref(n)) == 0 and n.value > 0:
        return
    assert _single(b"ACGT", 4, DNA) == NODEV
    assert _batch(b"ACGT", 4, DNA) == NODEV
    assert _batch(b"ACGT", 4, DNA, gscore=False) == NODEV    # the global scores are optional
    assert _batch(b"ACGT", 4, DNA, cigars=True, cigar_off=True) == NODEV
    assert _single32(b"ACGT", 4, DNA) == NODEV
    assert _batch32(b"ACGT", 4, DNA) == NODEV


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


def test_which_entry_runs(monkeypatch):
    from cse305_parallel_sequence_alignment_amd import _lib, api

    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    # no scoring argument: +1 / 0 over the symbols in first-seen order, A then B
    r = api.extend_align(b"GATTACA", b"GCATN", gap_open=4, gap_extend=1)
    name, args = rec.calls[0]
    assert name == "msa_extend_align" and len(args) == 14
    assert args[:4] == (b"GATTACA", 7, b"GCATN", 5) and args[4] == b"GATCN" and args[5] == 5
    assert (_table(args[6], 5) == np.eye(5, dtype=np.int8)).all()
    assert args[7:9] == (4, 1) and args[12] is not None and args[13] > 0
    assert set(r) == {"score", "a_end", "b_end", "global_score", "cigar"}
    rec.calls.clear()
    # match and / or mismatch; no traceback: no cigar buffer
    r = api.extend_align(b"GATTACA", b"GCATN", mismatch=-3, traceback=False)
    name, args = rec.calls[0]
    assert name == "msa_extend_align" and (_table(args[6], 5) == np.where(np.eye(5, dtype=bool), 1, -3)).all()
    assert args[12] is None and args[13] == 0
    assert set(r) == {"score", "a_end", "b_end", "global_score"}
    rec.calls.clear()
    # alphabet + matrix: passed through; max_symbols = 32: the twin
    api.extend_align(A, B, alphabet=b"ACGT", matrix=DNA.tolist(), max_symbols=32)
    name, args = rec.calls[0]
    assert name == "msa_extend_align32" and args[4] == b"ACGT" and args[5] == 4 and (_table(args[6], 4) == DNA).all()
    rec.calls.clear()
    # nine symbols need the twin: under 8 the symbols do not fit (decided before any library call)
    nine = b"ACGTNRYKM"
    api.extend_align(nine, nine[::-1], max_symbols=32)
    name, args = rec.calls[0]
    assert name == "msa_extend_align32" and args[4] == nine and args[5] == 9
    rec.calls.clear()
    # the batch: all of As, then the shared B (offsets all 0, sent once)
    api.extend_align_batch([b"GA", b"TT"], b"CAG", match=2)
    name, args = rec.calls[0]
    assert name == "msa_extend_align_batch" and len(args) == 20
    assert args[0] == b"GATT" and args[2] == b"CAG" and args[3] == 3 and args[4] == 2
    assert args[9] == b"GATC" and args[10] == 4
    assert (_table(args[11], 4) == np.where(np.eye(4, dtype=bool), 2, 0)).all()
    b_off = np.ctypeslib.as_array(C.cast(args[7], C.POINTER(C.c_int64)), shape=(2,))
    n = np.ctypeslib.as_array(C.cast(args[8], C.POINTER(C.c_int64)), shape=(2,))
    assert list(b_off) == [0, 0] and list(n) == [3, 3]
    assert args[15] is not None and args[16] is not None     # the end cells and the global scores
    rec.calls.clear()
    # ... and a list of Bs, back to back
    api.extend_align_batch([b"GA", b"TT"], [b"CAG", b"TTTT"], traceback=False, max_symbols=32)
    name, args = rec.calls[0]
    assert name == "msa_extend_align_batch32" and args[2] == b"CAGTTTT" and args[17] is None and args[19] is None
    b_off = np.ctypeslib.as_array(C.cast(args[7], C.POINTER(C.c_int64)), shape=(2,))
    assert list(b_off) == [0, 3]
