"""Host side of the X-drop extension entries (msa_extend_align_xdrop, msa_extend_align_batch_xdrop, their *32 twins,
msa_xdrop_extend_run / msa_xdrop_extend_walk, api.extend_align / api.extend_align_batch with ``xdrop``): the exported
symbols, the argument errors, which come before any device call and in the *_banded twins' order (without a GPU a valid
call is MSA_ERR_NODEV, so any other status was decided on the host), and which library entry the api functions reach.
Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

ARG, ALPHABET, NODEV, UNSUPPORTED = -1, -2, -4, -5
A, B = b"ACGTACGTAC", b"ACGTTCGTAGGTT"
DNA = np.array([[2, -3, -3, -3], [-3, 2, -3, -3], [-3, -3, 2, -3], [-3, -3, -3, 2]], dtype=np.int8)
ENTRIES = ("msa_extend_align_xdrop", "msa_extend_align_batch_xdrop", "msa_extend_align_xdrop32",
           "msa_extend_align_batch_xdrop32")
CAP = 640


def _i64(*v):
    return np.array(v, dtype=np.int64)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _single(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, band=4, xdrop=10, m=None, n=None, diag=True,
            entry="msa_extend_align_xdrop"):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc, gs, dg = C.c_int32(), C.c_int32(), C.c_int64()
    end = np.zeros(2, dtype=np.int64)
    return getattr(LB.lib(), entry)(a, len(a) if m is None else m, b, len(b) if n is None else n, alphabet, n_sym,
                                    _p(sub), gap_open, gap_extend, band, xdrop, C.byref(sc), _p(end), C.byref(gs),
                                    C.byref(dg) if diag else None, None, 0)


def _batch(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, band=4, xdrop=10, m=None, n=None, a_off=0, b_off=0,
           n_pairs=1, end=True, gscore=True, diag=True, cigars=False, cigar_off=False,
           entry="msa_extend_align_batch_xdrop"):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc, gs, dg = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    en = np.zeros(2, dtype=np.int64)
    ao, bo = _i64(a_off), _i64(b_off)
    mm, nn = _i64(len(a) if m is None else m), _i64(len(b) if n is None else n)
    cig = C.create_string_buffer(256) if cigars else None
    coff = np.zeros(2, dtype=np.int64) if cigar_off else None
    return getattr(LB.lib(), entry)(a, 0 if a is None else len(a), b, 0 if b is None else len(b), n_pairs, _p(ao),
                                    _p(mm), _p(bo), _p(nn), alphabet, n_sym, _p(sub), gap_open, gap_extend, band, xdrop,
                                    _p(sc), _p(en) if end else None, _p(gs) if gscore else None,
                                    _p(dg) if diag else None, cig, 256 if cigars else 0, _p(coff))


def _single32(*a, **k):
    return _single(*a, entry="msa_extend_align_xdrop32", **k)


def _batch32(*a, **k):
    return _batch(*a, entry="msa_extend_align_batch_xdrop32", **k)


def test_new_symbols_exported():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    assert LB.XDROP_BAND_MAX == CAP >= 512
    for name in ENTRIES + ("msa_xdrop_extend_run", "msa_xdrop_extend_walk"):
        assert name in LB.EXPORTED
        assert hasattr(L, name), f"libmsa.so does not export {name}"
    names = {name for name, _ in LB.KINDS["extend"].entries()}
    assert set(ENTRIES) <= names and "msa_extend_align_batch_banded32" in names and len(names) == 12
    # the slots of an X-drop entry: the banded twin's with xdrop after band and diagonals after global_score
    name, slots = LB.KINDS["extend"].entry(True, banded=True, xdrop=True)
    _, twin = LB.KINDS["extend"].entry(True, banded=True)
    assert name == "msa_extend_align_batch_xdrop"
    assert [s for s in slots if s not in ("xdrop", "diagonals")] == list(twin)
    assert slots[slots.index("band") + 1] == "xdrop" and slots[slots.index("global_score") + 1] == "diagonals"


@pytest.mark.parametrize("call", [_single, _batch, _single32, _batch32], ids=["single", "batch", "single32", "batch32"])
def test_entry_argument_errors(call):
    wide = call in (_single32, _batch32)
    assert call(b"ACGA", 4, DNA) == ARG                      # a duplicate symbol
    assert call(b"", 0, DNA) == ARG                          # n_sym 0
    if wide:
        assert call(bytes(range(65, 98)), 33, np.zeros((33, 33), dtype=np.int8)) == ARG      # n_sym 33
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
    # the gap rule comes before the symbols are looked at
    assert call(b"ACGT", 4, DNA, a=b"ACGNACGT", gap_open=1, gap_extend=2) == UNSUPPORTED
    # band < 0 is an argument error, decided with the other arguments: before the gap rule and the symbols
    assert call(b"ACGT", 4, DNA, band=-1) == ARG
    assert call(b"ACGT", 4, DNA, band=-1, gap_open=1, gap_extend=2) == ARG
    assert call(b"ACGT", 4, DNA, band=-1, a=b"ACGNACGT") == ARG
    # |m - n| > band is no error: the entry clips; any xdrop is valid, negative (never stop) included
    for band in (0, 1, 2, 3):
        for xdrop in (-1, 0, 7, 2 ** 31 - 1, -(2 ** 31)):
            assert call(b"ACGT", 4, DNA, band=band, xdrop=xdrop) in (0, NODEV)
    assert call(b"ACGT", 4, DNA, band=0, b=b"ACGTTCGTX") == ALPHABET  # a clipped-away symbol is still checked


@pytest.mark.parametrize("call", [_single, _batch, _single32, _batch32], ids=["single", "batch", "single32", "batch32"])
def test_band_cap(call):
    """A band above MSA_XDROP_BAND_MAX is MSA_ERR_UNSUPPORTED, decided with the gap rule: after the argument errors,
    before the symbols.  A band wider than the longest sequence holds the same cells as that sequence's length."""
    long_a, long_b = b"ACGT" * 200, b"ACGT" * 180  # 800 x 720: a band up to 800 means something
    kw = dict(a=long_a, b=long_b)
    assert call(b"ACGT", 4, DNA, band=CAP, **kw) in (0, NODEV)
    assert call(b"ACGT", 4, DNA, band=CAP + 1, **kw) == UNSUPPORTED
    assert call(b"ACGT", 4, DNA, band=1 << 40, **kw) == UNSUPPORTED
    assert call(b"ACGT", 4, DNA, band=CAP + 1, a=long_a[:-1] + b"N", b=long_b) == UNSUPPORTED  # before the symbols
    assert call(b"ACGT", 4, DNA, band=CAP + 1, m=0, **kw) == ARG                               # after the arguments
    assert call(b"ACGT", 4, DNA, band=CAP + 1) in (0, NODEV)  # 10 x 13: band 13 holds every cell
    assert call(b"ACGT", 4, DNA, band=1 << 40) in (0, NODEV)


def test_single_entry_null_sequences():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc = C.c_int32()
    f = LB.lib().msa_extend_align_xdrop
    assert f(None, 4, B, len(B), b"ACGT", 4, _p(DNA), 5, 2, 4, 10, C.byref(sc), None, None, None, None, 0) == ARG
    assert f(A, len(A), None, 4, b"ACGT", 4, _p(DNA), 5, 2, 4, 10, C.byref(sc), None, None, None, None, 0) == ARG
    assert f(A, (1 << 26) + 1, B, len(B), b"ACGT", 4, _p(DNA), 5, 2, 4, 10, C.byref(sc), None, None, None, None,
             0) == ARG


def test_batch_entry_argument_errors():
    ok = dict(alphabet=b"ACGT", n_sym=4, sub=DNA)
    assert _batch(**ok, n_pairs=0) == ARG
    assert _batch(**ok, end=False) == ARG                    # the end cells are the entry's result
    assert _batch(**ok, cigars=True, cigar_off=False) == ARG  # cigars without cigar_off
    assert _batch(**ok, a_off=1) == ARG                      # A's range leaves the buffer
    assert _batch(**ok, b_off=-1) == ARG
    assert _batch(**ok, n=len(B) + 1, band=0) == ARG         # B's range leaves the buffer, clipped or not
    assert _batch(**ok, a=None, m=4) == ARG
    assert _batch(**ok, b=None, n=4) == ARG


def test_device_entry_argument_errors():
    """msa_xdrop_extend_run / _walk decide their own arguments before they ask for a device."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    p = 4096  # (never dereferenced on the host)
    run = lambda **k: L.msa_xdrop_extend_run(*[k.get(s, d) for s, d in (  # noqa: E731
        ("dA", p), ("dB", p), ("np", 1), ("m", p), ("n", p), ("ao", p), ("bo", p), ("sub", None), ("match", 2),
        ("mismatch", -3), ("go", 5), ("ge", 2), ("band", 4), ("xdrop", 10), ("dir", None), ("doff", None), ("res", p),
        ("stream", None))])
    # (a valid call would launch: the GPU tests make those)
    assert run(dA=None) == ARG and run(res=None) == ARG and run(np=0) == ARG and run(band=-1) == ARG
    assert run(dir=p) == ARG                                 # bytes without their offsets
    assert run(band=CAP + 1) == UNSUPPORTED and run(go=1) == UNSUPPORTED and run(ge=-1) == UNSUPPORTED
    assert run(match=128) == UNSUPPORTED and run(match=128, sub=p, band=-1) == ARG
    walk = lambda **k: L.msa_xdrop_extend_walk(*[k.get(s, d) for s, d in (  # noqa: E731
        ("np", 1), ("band", 4), ("dir", p), ("doff", p), ("res", p), ("ops", p), ("ooff", p), ("info", p),
        ("stream", None))])
    assert walk(dir=None) == ARG and walk(info=None) == ARG and walk(np=0) == ARG and walk(band=-1) == ARG
    assert walk(band=CAP + 1) == UNSUPPORTED


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
            f(a, b, xdrop=10)                                    # xdrop without a band: before any C call
        with pytest.raises(ValueError):
            f(a, b, xdrop=10, band=-1)
        with pytest.raises(ValueError):
            f(a, b, band=4, xdrop=10, max_symbols=16)
        assert _status(lambda: f(a, b, band=4, xdrop=10, alphabet=b"ACGA", matrix=DNA)) == ARG
        assert _status(lambda: f(a, b, band=4, xdrop=10, alphabet=b"ACG", matrix=DNA[:3, :3])) == ALPHABET
        assert _status(lambda: f(a, b, band=4, xdrop=10, gap_open=1, gap_extend=2)) == UNSUPPORTED
        assert _status(lambda: f(a, b, band=-2, xdrop=10)) == ARG
    assert api.extend_align_batch([], B, band=4, xdrop=3) == []  # an empty batch


def test_xdrop_without_band_makes_no_c_call(monkeypatch):
    from cse305_parallel_sequence_alignment_amd import _lib, api

    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    with pytest.raises(ValueError):
        api.extend_align(A, B, xdrop=5)
    with pytest.raises(ValueError):
        api.extend_align_batch([A], B, xdrop=5)
    assert not rec.calls


def test_no_device_status():
    """Without a GPU a valid call returns MSA_ERR_NODEV under its entry's name (no fallback)."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd import api

    n = C.c_int(0)
    if LB.lib().msa_device_count(C.byref(n)) == 0 and n.value > 0:
        return
    assert _single(b"ACGT", 4, DNA) == NODEV
    assert _single(b"ACGT", 4, DNA, band=0, xdrop=-1) == NODEV
    assert _single(b"ACGT", 4, DNA, diag=False) == NODEV     # diagonals is optional
    assert _batch(b"ACGT", 4, DNA) == NODEV
    assert _batch(b"ACGT", 4, DNA, gscore=False, diag=False) == NODEV
    assert _batch(b"ACGT", 4, DNA, cigars=True, cigar_off=True) == NODEV
    assert _single32(b"ACGT", 4, DNA) == NODEV
    assert _batch32(b"ACGT", 4, DNA) == NODEV
    for fn, args, kw, entry in (
            (api.extend_align, (A, B), dict(band=3, xdrop=5), "msa_extend_align_xdrop"),
            (api.extend_align_batch, ([A, A], B), dict(band=3, xdrop=0), "msa_extend_align_batch_xdrop"),
            (api.extend_align, (A, B), dict(band=0, xdrop=-1, max_symbols=32), "msa_extend_align_xdrop32"),
            (api.extend_align_batch, ([A], [B]), dict(band=3, xdrop=5, max_symbols=32, traceback=False),
             "msa_extend_align_batch_xdrop32")):
        with pytest.raises(LB.MsaError) as e:
            fn(*args, **kw)
        assert e.value.status == NODEV and str(e.value).startswith(entry + ":")


class _Recorder:
    """Stands in for the library handle: every entry records its name and arguments, writes ``diagonals`` where the
    entry has one (a single entry's argument 14) and returns MSA_OK."""

    def __init__(self, diagonals=None):
        self.calls, self.diagonals = [], diagonals

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if self.diagonals is not None:
                args[14]._obj.value = self.diagonals
            return 0

        return entry


def test_which_entry_runs(monkeypatch):
    from cse305_parallel_sequence_alignment_amd import _lib, api

    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    # xdrop=None, given or not: exactly today's calls
    for kw in ({}, {"xdrop": None}):
        api.extend_align(b"GATTACA", b"GCATN", gap_open=4, gap_extend=1, **kw)
        name, args = rec.calls.pop()
        assert name == "msa_extend_align" and len(args) == 14
        r = api.extend_align(b"GATTACA", b"GCATN", gap_open=4, gap_extend=1, band=0, **kw)
        name, args = rec.calls.pop()
        assert name == "msa_extend_align_banded" and len(args) == 15 and args[7:10] == (4, 1, 0)
        assert set(r) == {"score", "a_end", "b_end", "global_score", "cigar"}
        api.extend_align_batch([b"GA", b"TT"], b"CAG", match=2, band=7, **kw)
        name, args = rec.calls.pop()
        assert name == "msa_extend_align_batch_banded" and len(args) == 21
    # with xdrop: the X-drop entries, xdrop after the band, diagonals after the global score
    r = api.extend_align(b"GATTACA", b"GCATN", gap_open=4, gap_extend=1, band=2, xdrop=9)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_xdrop" and len(args) == 17
    assert args[:4] == (b"GATTACA", 7, b"GCATN", 5) and args[4] == b"GATCN" and args[5] == 5
    assert args[7:11] == (4, 1, 2, 9) and args[14] is not None and args[15] is not None and args[16] > 0
    assert set(r) == {"score", "a_end", "b_end", "global_score", "diagonals", "dropped", "cigar"}
    r = api.extend_align(b"GATTACA", b"GCATN", band=3, xdrop=-1, traceback=False)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_xdrop" and args[9:11] == (3, -1) and args[15] is None and args[16] == 0
    assert set(r) == {"score", "a_end", "b_end", "global_score", "diagonals", "dropped"}
    api.extend_align(A, B, alphabet=b"ACGT", matrix=DNA.tolist(), max_symbols=32, band=5, xdrop=0)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_xdrop32" and args[4] == b"ACGT" and args[9:11] == (5, 0)
    api.extend_align_batch([b"GA", b"TT"], b"CAG", match=2, band=7, xdrop=11)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_batch_xdrop" and len(args) == 23 and args[12:16] == (3, 1, 7, 11)
    assert args[17] is not None and args[18] is not None and args[19] is not None
    api.extend_align_batch([b"GA", b"TT"], [b"CAG", b"TTTT"], traceback=False, max_symbols=32, band=1, xdrop=4)
    name, args = rec.calls.pop()
    assert name == "msa_extend_align_batch_xdrop32" and args[14:16] == (1, 4) and args[20] is None and args[22] is None
    assert not rec.calls


def test_dropped_is_diagonals_below_the_clipped_sum(monkeypatch):
    from cse305_parallel_sequence_alignment_amd import _lib, api

    # A is 10 long, B 13: band 2 clips to (10, 12), 22 anti-diagonals; band 0 to (10, 10)
    for band, diagonals, dropped in ((2, 22, False), (2, 21, True), (0, 20, False), (0, 19, True), (50, 23, False)):
        monkeypatch.setattr(_lib, "lib", lambda d=diagonals: _Recorder(diagonals=d))
        r = api.extend_align(A, B, band=band, xdrop=3, traceback=False)
        assert (r["diagonals"], r["dropped"]) == (diagonals, dropped)
