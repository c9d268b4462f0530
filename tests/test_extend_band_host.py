"""Host side of the banded extension entries (msa_extend_align_banded, msa_extend_align_batch_banded, their *32 twins,
msa_extend_band_clip, api.extend_align / api.extend_align_batch with ``band``): the exported symbols, the clip rule,
the argument errors, which come before any device call (without a GPU a valid call is MSA_ERR_NODEV, so any other
status was decided on the host), and which library entry the api functions reach for which band.  Nothing here needs
a GPU."""
import ctypes as C

import numpy as np
import pytest

ARG, ALPHABET, NODEV, UNSUPPORTED = -1, -2, -4, -5
A, B = b"ACGTACGTAC", b"ACGTTCGTAGGTT"
DNA = np.array([[2, -3, -3, -3], [-3, 2, -3, -3], [-3, -3, 2, -3], [-3, -3, -3, 2]], dtype=np.int8)
ENTRIES = ("msa_extend_align_banded", "msa_extend_align_batch_banded", "msa_extend_align_banded32",
           "msa_extend_align_batch_banded32")


def _i64(*v):
    return np.array(v, dtype=np.int64)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _single(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, band=4, m=None, n=None,
            entry="msa_extend_align_banded"):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc, gs = C.c_int32(), C.c_int32()
    end = np.zeros(2, dtype=np.int64)
    return getattr(LB.lib(), entry)(a, len(a) if m is None else m, b, len(b) if n is None else n, alphabet, n_sym,
                                    _p(sub), gap_open, gap_extend, band, C.byref(sc), _p(end), C.byref(gs), None, 0)


def _batch(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, band=4, m=None, n=None, a_off=0, b_off=0,
           n_pairs=1, end=True, gscore=True, cigars=False, cigar_off=False, entry="msa_extend_align_batch_banded"):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc, gs = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    en = np.zeros(2, dtype=np.int64)
    ao, bo = _i64(a_off), _i64(b_off)
    mm, nn = _i64(len(a) if m is None else m), _i64(len(b) if n is None else n)
    cig = C.create_string_buffer(256) if cigars else None
    coff = np.zeros(2, dtype=np.int64) if cigar_off else None
    return getattr(LB.lib(), entry)(a, 0 if a is None else len(a), b, 0 if b is None else len(b), n_pairs, _p(ao),
                                    _p(mm), _p(bo), _p(nn), alphabet, n_sym, _p(sub), gap_open, gap_extend, band,
                                    _p(sc), _p(en) if end else None, _p(gs) if gscore else None, cig,
                                    256 if cigars else 0, _p(coff))


def _single32(*a, **k):
    return _single(*a, entry="msa_extend_align_banded32", **k)


def _batch32(*a, **k):
    return _batch(*a, entry="msa_extend_align_batch_banded32", **k)


def test_new_symbols_exported():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    assert LB.NW_EXTEND_BAND == 11 and LB.NW_EXTEND == 10
    assert LB.SCORE_NONE == -2 ** 31
    for name in ENTRIES + ("msa_extend_band_clip",):
        assert name in LB.EXPORTED
        assert hasattr(L, name), f"libmsa.so does not export {name}"


def test_band_clip():
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import extend_band_clip

    for (m, n, w), want in {(400, 150, 16): (166, 150), (150, 400, 16): (150, 166), (10, 10, 0): (10, 10),
                            (10, 11, 0): (10, 10), (11, 10, 0): (10, 10), (1, 500, 3): (1, 4), (500, 1, 3): (4, 1),
                            (7, 9, 2): (7, 9), (7, 9, 1): (7, 8), (7, 9, 100): (7, 9), (300, 290, 8): (298, 290),
                            (203, 322, 64): (203, 267), (5, 3, 2 ** 62): (5, 3),
                            (2 ** 40, 1, 2 ** 62): (2 ** 40, 1)}.items():
        assert extend_band_clip(m, n, w) == want, (m, n, w)
        assert abs(want[0] - want[1]) <= w
    f = LB.lib().msa_extend_band_clip
    me, ne = C.c_int64(-7), C.c_int64(-7)
    for m, n, w in ((0, 5, 3), (5, 0, 3), (5, 5, -1), (-1, 5, 3)):
        assert f(m, n, w, C.byref(me), C.byref(ne)) == ARG and (me.value, ne.value) == (-7, -7)
    assert f(9, 3, 2, None, C.byref(ne)) == 0 and ne.value == 3        # either output may be NULL
    assert f(9, 3, 2, C.byref(me), None) == 0 and me.value == 5
    assert f(9, 3, 2, None, None) == 0


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
    # the gap rule comes before the symbols are looked at, as in msa_extend_align
    assert call(b"ACGT", 4, DNA, a=b"ACGNACGT", gap_open=1, gap_extend=2) == UNSUPPORTED
    # a band is required: -1 (the unbanded entries' "none") and anything below are argument errors, decided with the
    # other arguments -- before the gap rule and the symbols
    assert call(b"ACGT", 4, DNA, band=-1) == ARG
    assert call(b"ACGT", 4, DNA, band=-2) == ARG
    assert call(b"ACGT", 4, DNA, band=-1, gap_open=1, gap_extend=2) == ARG
    assert call(b"ACGT", 4, DNA, band=-1, a=b"ACGNACGT") == ARG
    # |m - n| > band is no error here: the entry clips (so the next decision is the device's)
    for band in (0, 1, 2, 3, 1 << 40):
        assert call(b"ACGT", 4, DNA, band=band) in (0, NODEV)
    assert call(b"ACGT", 4, DNA, band=0, b=b"ACGTTCGTX") == ALPHABET  # ... and a clipped-away symbol is still checked


def test_single_entry_null_sequences():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc = C.c_int32()
    f = LB.lib().msa_extend_align_banded
    assert f(None, 4, B, len(B), b"ACGT", 4, _p(DNA), 5, 2, 4, C.byref(sc), None, None, None, 0) == ARG
    assert f(A, len(A), None, 4, b"ACGT", 4, _p(DNA), 5, 2, 4, C.byref(sc), None, None, None, 0) == ARG
    assert f(A, (1 << 26) + 1, B, len(B), b"ACGT", 4, _p(DNA), 5, 2, 4, C.byref(sc), None, None, None, 0) == ARG


def test_batch_entry_argument_errors():
    ok = dict(alphabet=b"ACGT", n_sym=4, sub=DNA)
    assert _batch(**ok, n_pairs=0) == ARG
    assert _batch(**ok, end=False) == ARG                    # the end cells are the entry's result
    assert _batch(**ok, cigars=True, cigar_off=False) == ARG  # cigars without cigar_off
    assert _batch(**ok, a_off=1) == ARG                      # A's range leaves the buffer
    assert _batch(**ok, b_off=-1) == ARG
    assert _batch(**ok, n=len(B) + 1) == ARG                 # B's range leaves the buffer, clipped or not
    assert _batch(**ok, n=len(B) + 1, band=0) == ARG
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
            f(a, b, band=4, max_symbols=16)                      # 8 or 32
        with pytest.raises(ValueError):
            f(a, b, band=4, matrix=DNA)                          # matrix without alphabet
        assert _status(lambda: f(a, b, band=4, alphabet=b"ACGA", matrix=DNA)) == ARG
        assert _status(lambda: f(a, b, band=4, alphabet=b"ACG", matrix=DNA[:3, :3])) == ALPHABET  # T is outside
        assert _status(lambda: f(a, b, band=4, gap_open=1, gap_extend=2)) == UNSUPPORTED
        assert _status(lambda: f(a, b, band=-2)) == ARG          # no band is -1, the default, alone
    assert api.extend_align_batch([], B, band=4) == []           # an empty batch


def test_no_device_status():
    """Without a GPU a valid call returns MSA_ERR_NODEV (no fallback).  (With one, the GPU tests cover these calls.)"""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    n = C.c_int(0)
    if LB.lib().msa_device_count(C.byref(n)) == 0 and n.value > 0:
        return
    assert _single(b"ACGT", 4, DNA) == NODEV
    assert _single(b"ACGT", 4, DNA, band=0) == NODEV         # a clipped pair
    assert _batch(b"ACGT", 4, DNA) == NODEV
    assert _batch(b"ACGT", 4, DNA, gscore=False) == NODEV    # the global scores are optional
    assert _batch(b"ACGT", 4, DNA, cigars=True, cigar_off=True) == NODEV
    assert _single32(b"ACGT", 4, DNA) == NODEV
    assert _batch32(b"ACGT", 4, DNA) == NODEV


class _Recorder:
    """Stands in for the library handle: every entry records its name and arguments and returns MSA_OK."""

    def __init__(self, gscore=None):
        self.calls, self.gscore = [], gscore

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if self.gscore is not None:  # the single entries' global_score: argument 12 with a band
                args[12]._obj.value = self.gscore
            return 0

        return entry


def test_which_entry_runs(monkeypatch):
    from cse305_parallel_sequence_alignment_amd import _lib, api

    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    # band = -1, given or not: exactly the unbanded call, 14 arguments, no band among them
    for kw in ({}, {"band": -1}):
        api.extend_align(b"GATTACA", b"GCATN", gap_open=4, gap_extend=1, **kw)
        name, args = rec.calls.pop()
        assert name == "msa_extend_align" and len(args) == 14 and args[7:9] == (4, 1) and args[12] is not None
        api.extend_align_batch([b"GA", b"TT"], b"CAG", match=2, **kw)
        name, args = rec.calls.pop()
        assert name == "msa_extend_align_batch" and len(args) == 20
        api.extend_align(A, B, max_symbols=32, **kw)
        assert rec.calls.pop()[0] == "msa_extend_align32"
        api.extend_align_batch([A], B, max_symbols=32, **kw)
        assert rec.calls.pop()[0] == "msa_extend_align_batch32"
    # band >= 0: the banded entries, the band after gap_extend and everything else where it was
    r = api.extend_align(b"GATTACA", b"GCATN", gap_open=4, gap_extend=1, band=0)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_banded" and len(args) == 15
    assert args[:4] == (b"GATTACA", 7, b"GCATN", 5) and args[4] == b"GATCN" and args[5] == 5
    assert args[7:10] == (4, 1, 0) and args[13] is not None and args[14] > 0  # (the cigar and its capacity)
    assert set(r) == {"score", "a_end", "b_end", "global_score", "cigar"}
    r = api.extend_align(b"GATTACA", b"GCATN", band=3, traceback=False)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_banded" and args[9] == 3 and args[13] is None and args[14] == 0
    assert set(r) == {"score", "a_end", "b_end", "global_score"}
    api.extend_align(A, B, alphabet=b"ACGT", matrix=DNA.tolist(), max_symbols=32, band=5)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_banded32" and args[4] == b"ACGT" and args[9] == 5
    api.extend_align_batch([b"GA", b"TT"], b"CAG", match=2, band=7)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_batch_banded" and len(args) == 21 and args[12:15] == (3, 1, 7)
    assert args[0] == b"GATT" and args[2] == b"CAG" and args[4] == 2 and args[9] == b"GATC"
    assert args[16] is not None and args[17] is not None     # the end cells and the global scores
    api.extend_align_batch([b"GA", b"TT"], [b"CAG", b"TTTT"], traceback=False, max_symbols=32, band=1)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_batch_banded32" and args[14] == 1 and args[18] is None and args[20] is None
    assert not rec.calls


def test_global_score_none(monkeypatch):
    """MSA_SCORE_NONE from the entry is None in the dict; any other value is itself."""
    from cse305_parallel_sequence_alignment_amd import _lib, api

    for raw, want in ((_lib.SCORE_NONE, None), (-17, -17), (0, 0)):
        monkeypatch.setattr(_lib, "lib", lambda raw=raw: _Recorder(gscore=raw))
        assert api.extend_align(A, B, band=2)["global_score"] == want
