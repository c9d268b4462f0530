"""Host side of the seed-extension entries (msa_seed_align, msa_seed_align_batch, their *32 twins, msa_xdrop_flank_run,
api.seed_align / api.seed_align_batch): the exported symbols, the argument errors, which come before any device call and
in the order include/msa.h states (without a GPU a valid call with a flank to launch is MSA_ERR_NODEV, so any other
status was decided on the host), a call whose flanks are all empty, which makes no device call at all, and which library
entry the api functions reach.  Nothing here needs a GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ARG, ALPHABET, NODEV, UNSUPPORTED = -1, -2, -4, -5
A, B = b"ACGTACGTACGG", b"TTACGTTCGTAGGTT"
DNA = np.array([[2, -3, -3, -3], [-3, 2, -3, -3], [-3, -3, 2, -3], [-3, -3, -3, 2]], dtype=np.int8)
ENTRIES = ("msa_seed_align", "msa_seed_align_batch", "msa_seed_align32", "msa_seed_align_batch32")
CAP = 640
HEADER = Path(__file__).resolve().parent.parent / "include" / "msa.h"


def _i64(*v):
    return np.array(v, dtype=np.int64)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _single(alphabet, n_sym, sub, a=A, b=B, seed=(4, 6, 3), gap_open=5, gap_extend=2, band=4, xdrop=10, m=None, n=None,
            score=True, beg=True, end=True, flank=True, diag=True, entry="msa_seed_align", out=None):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc = C.c_int32()
    be, en, dg = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    fs = np.zeros(2, dtype=np.int32)
    rc = getattr(LB.lib(), entry)(a, len(a) if m is None else m, b, len(b) if n is None else n, *seed, alphabet, n_sym,
                                  _p(sub), gap_open, gap_extend, band, xdrop, C.byref(sc) if score else None,
                                  _p(be) if beg else None, _p(en) if end else None, _p(fs) if flank else None,
                                  _p(dg) if diag else None, None, 0)
    if out is not None:
        out.update(score=sc.value, beg=tuple(be), end=tuple(en), flank=tuple(fs), diag=tuple(dg))
    return rc


def _batch(alphabet, n_sym, sub, a=A, b=B, seed=(4, 6, 3), gap_open=5, gap_extend=2, band=4, xdrop=10, m=None, n=None,
           a_off=0, b_off=0, n_pairs=1, score=True, beg=True, end=True, flank=True, diag=True, cigars=False,
           cigar_off=False, seeds=(True, True, True), entry="msa_seed_align_batch", out=None):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc, fs = np.zeros(1, dtype=np.int32), np.zeros(2, dtype=np.int32)
    be, en, dg = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    ao, bo = _i64(a_off), _i64(b_off)
    mm, nn = _i64(len(a) if m is None else m), _i64(len(b) if n is None else n)
    sd = [_p(_i64(v)) if on else None for v, on in zip(seed, seeds)]
    cig = C.create_string_buffer(256) if cigars else None
    coff = np.zeros(2, dtype=np.int64) if cigar_off else None
    rc = getattr(LB.lib(), entry)(a, 0 if a is None else len(a), b, 0 if b is None else len(b), n_pairs, _p(ao),
                                  _p(mm), _p(bo), _p(nn), *sd, alphabet, n_sym, _p(sub), gap_open, gap_extend, band,
                                  xdrop, _p(sc) if score else None, _p(be) if beg else None, _p(en) if end else None,
                                  _p(fs) if flank else None, _p(dg) if diag else None, cig, 256 if cigars else 0,
                                  _p(coff))
    if out is not None:
        out.update(score=int(sc[0]), beg=tuple(be), end=tuple(en), flank=tuple(fs), diag=tuple(dg),
                   cigar=cig.value.decode() if cigars else None)
    return rc


def _single32(*a, **k):
    return _single(*a, entry="msa_seed_align32", **k)


def _batch32(*a, **k):
    return _batch(*a, entry="msa_seed_align_batch32", **k)


CALLS = pytest.mark.parametrize("call", [_single, _batch, _single32, _batch32],
                                ids=["single", "batch", "single32", "batch32"])


def test_new_symbols_exported():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    header = HEADER.read_text()
    names = [name for name, _ in LB.KINDS["seed"].entries()]
    assert sorted(names) == sorted(ENTRIES)
    for name in ENTRIES + ("msa_xdrop_flank_run",):
        assert name in LB.EXPORTED
        assert hasattr(L, name), f"libmsa.so does not export {name}"
        assert re.search(r"^int " + name + r"\(", header, re.M), f"msa.h does not declare {name}"
    # the slots: three int64 inputs after the sequences (values for one pair, arrays for a batch), band and xdrop in
    # every entry, the 2-wide flank scores and diagonals after the two cells
    _, one = LB.KINDS["seed"].entry(False)
    _, many = LB.KINDS["seed"].entry(True)
    assert one == ("A", "a_len", "B", "b_len", "seed_a0", "seed_b0", "seed_len0", "alphabet", "n_sym", "sub",
                   "gap_open", "gap_extend", "band", "xdrop", "score", "beg", "end", "flank_score", "diagonals", "cigar",
                   "cap")
    assert many == ("A", "a_len", "B", "b_len", "k", "a_off", "m", "b_off", "n", "seed_a", "seed_b", "seed_len",
                    "alphabet", "n_sym", "sub", "gap_open", "gap_extend", "band", "xdrop", "score", "beg", "end",
                    "flank_score", "diagonals", "cigar", "cap", "cigar_off")
    # the argument names of the header's declaration, in its order, say the same
    decl = re.search(r"^int msa_seed_align_batch\((.*?)\);", header, re.M | re.S).group(1)
    args = [re.sub(r".*[ *]", "", x.strip()) for x in decl.split(",")]
    assert args == ["A", "a_len", "B", "b_len", "n_pairs", "a_off", "m", "b_off", "n", "seed_a", "seed_b", "seed_len",
                    "alphabet", "n_sym", "sub", "gap_open", "gap_extend", "band", "xdrop", "score", "beg_ij", "end_ij",
                    "flank_score", "diagonals", "cigars", "cigar_cap", "cigar_off"]
    # the kinds from before are what they were
    assert len({name for name, _ in LB.KINDS["extend"].entries()}) == 12


@CALLS
def test_entry_argument_errors(call):
    wide = call in (_single32, _batch32)
    ok = (b"ACGT", 4, DNA)
    assert call(b"ACGA", 4, DNA) == ARG                      # a duplicate symbol
    assert call(b"", 0, DNA) == ARG                          # n_sym 0
    if wide:
        assert call(bytes(range(65, 98)), 33, np.zeros((33, 33), dtype=np.int8)) == ARG      # n_sym 33
    else:
        assert call(b"ACGTNRYKM", 9, np.zeros((9, 9), dtype=np.int8)) == ARG  # n_sym 9
    assert call(None, 4, DNA) == ARG                         # no alphabet
    assert call(b"ACGT", 4, None) == ARG                     # no matrix
    # a missing output among score, beg_ij and end_ij; flank_score and diagonals are optional
    assert call(*ok, score=False) == ARG and call(*ok, beg=False) == ARG and call(*ok, end=False) == ARG
    assert call(*ok, flank=False, diag=False) in (0, NODEV)
    assert call(*ok, m=0) == ARG and call(*ok, n=0) == ARG   # an empty A, an empty B
    # the seed: negative, or past the end of either sequence
    assert call(*ok, seed=(4, 6, -1)) == ARG
    assert call(*ok, seed=(-1, 6, 3)) == ARG and call(*ok, seed=(4, -1, 3)) == ARG
    assert call(*ok, seed=(len(A) - 2, 6, 3)) == ARG and call(*ok, seed=(4, len(B) - 2, 3)) == ARG
    assert call(*ok, seed=(len(A) + 1, 6, 0)) == ARG and call(*ok, seed=(1 << 62, 6, 1 << 62)) == ARG
    assert call(*ok, seed=(len(A) - 3, len(B) - 3, 3)) in (0, NODEV)   # ... ending at (m, n) is a seed
    assert call(*ok, band=-1) == ARG
    # the argument errors come before the unsupported parameters, and those before the symbols
    assert call(*ok, band=-1, gap_open=1, gap_extend=2) == ARG
    assert call(*ok, seed=(4, 6, -1), gap_open=1, gap_extend=2) == ARG
    assert call(*ok, band=-1, a=b"ACGNACGTACGG") == ARG
    assert call(*ok, gap_open=1, gap_extend=2) == UNSUPPORTED
    assert call(*ok, gap_open=1, gap_extend=-1) == UNSUPPORTED
    assert call(*ok, a=b"ACGNACGTACGG", gap_open=1, gap_extend=2) == UNSUPPORTED
    assert call(*ok, a=b"ACGNACGTACGG") == ALPHABET          # a symbol of A outside the alphabet
    assert call(*ok, b=b"TTACGTTCGTAGGTX") == ALPHABET       # ... of B, in a part the band clips away
    assert call(*ok, b=b"TTACGTTCGTAGGTX", band=0) == ALPHABET
    # the value-range inequality, taken with the whole m + n: (127 + 4 * 500000) * (12 + 15 + 256) >= 2^28
    big = DNA.copy()
    big[0, 0] = 127
    assert call(b"ACGT", 4, big, gap_open=500000, gap_extend=500000) == UNSUPPORTED
    assert call(b"ACGT", 4, big, gap_open=500000, gap_extend=500000, a=b"ACGNACGTACGG") == UNSUPPORTED  # before symbols
    assert call(b"ACGT", 4, big, gap_open=500000, gap_extend=500000, band=-1) == ARG
    # any xdrop is valid, negative (never stop) included; |m - n| > band is no error: each flank is clipped
    for band in (0, 1, 3):
        for xdrop in (-1, 0, 7, 2 ** 31 - 1, -(2 ** 31)):
            assert call(*ok, band=band, xdrop=xdrop) in (0, NODEV)


@CALLS
def test_band_cap(call):
    """A band above MSA_XDROP_BAND_MAX is MSA_ERR_UNSUPPORTED: after the argument errors, before the symbols.  A band
    wider than the call's longest sequence holds the same cells as that sequence's length."""
    long_a, long_b = b"ACGT" * 200, b"ACGT" * 180  # 800 x 720
    kw = dict(a=long_a, b=long_b, seed=(400, 400, 8))
    ok = (b"ACGT", 4, DNA)
    assert call(*ok, band=CAP, **kw) in (0, NODEV)
    assert call(*ok, band=CAP + 1, **kw) == UNSUPPORTED
    assert call(*ok, band=1 << 40, **kw) == UNSUPPORTED
    assert call(*ok, band=CAP + 1, a=long_a[:-1] + b"N", b=long_b, seed=(400, 400, 8)) == UNSUPPORTED
    assert call(*ok, band=CAP + 1, m=0, **kw) == ARG
    assert call(*ok, band=CAP + 1, a=long_a, b=long_b, seed=(400, 400, -8)) == ARG
    assert call(*ok, band=CAP + 1) in (0, NODEV)   # 12 x 15: band 15 holds every cell
    assert call(*ok, band=1 << 40) in (0, NODEV)


def test_single_entry_null_sequences():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc = C.c_int32()
    ij = np.zeros(4, dtype=np.int64)
    f = LB.lib().msa_seed_align
    tail = (b"ACGT", 4, _p(DNA), 5, 2, 4, 10, C.byref(sc), _p(ij), _p(ij[2:]), None, None, None, 0)
    assert f(None, 4, B, len(B), 1, 1, 1, *tail) == ARG
    assert f(A, len(A), None, 4, 1, 1, 1, *tail) == ARG
    assert f(A, (1 << 26) + 1, B, len(B), 1, 1, 1, *tail) == ARG


def test_batch_entry_argument_errors():
    ok = dict(alphabet=b"ACGT", n_sym=4, sub=DNA)
    assert _batch(**ok, n_pairs=0) == ARG
    assert _batch(**ok, cigars=True, cigar_off=False) == ARG  # cigars without cigar_off
    assert _batch(**ok, a_off=1) == ARG                      # A's range leaves the buffer
    assert _batch(**ok, b_off=-1) == ARG
    assert _batch(**ok, n=len(B) + 1, band=0) == ARG         # B's range leaves the buffer, clipped or not
    assert _batch(**ok, a=None, m=4) == ARG
    assert _batch(**ok, b=None, n=4) == ARG
    for k in range(3):                                       # a missing seed array
        assert _batch(**ok, seeds=tuple(j != k for j in range(3))) == ARG
    # the seed is relative to its pair, not to the buffer: the pair is A[2:8], 6 long
    assert _batch(**ok, a_off=2, m=6, seed=(3, 6, 3)) in (0, NODEV)
    assert _batch(**ok, a_off=2, m=6, seed=(4, 6, 3)) == ARG


def test_all_flanks_empty_makes_no_device_call():
    """A seed that leaves no symbols on either side of each flank has nothing to launch: the answer -- the seed's own
    score, the seed's own cells, seed_len M -- comes from the host, with or without a GPU."""
    ok = (b"ACGT", 4, DNA)
    for call in (_single, _batch, _single32, _batch32):
        out = {}
        # the seed = both whole sequences, one mismatch in it
        assert call(*ok, a=b"ACGTAC", b=b"ACGGAC", seed=(0, 0, 6), out=out) == 0
        assert (out["score"], out["beg"], out["end"], out["flank"], out["diag"]) == (7, (0, 0), (6, 6), (0, 0), (0, 0))
        # a side of each flank is empty: seed_a == 0 on the left, the seed ending at n on the right
        assert call(*ok, a=b"ACGTAC", b=b"TTACG", seed=(0, 2, 3), out=out) == 0
        assert (out["score"], out["beg"], out["end"], out["flank"], out["diag"]) == (6, (0, 2), (3, 5), (0, 0), (0, 0))
        # a bare anchor in a corner
        assert call(*ok, seed=(0, len(B), 0), out=out) == 0
        assert (out["score"], out["beg"], out["end"]) == (0, (0, len(B)), (0, len(B)))
        # the checks still come first
        assert call(*ok, a=b"ACGTAC", b=b"ACGGAN", seed=(0, 0, 6)) == ALPHABET
        assert call(*ok, a=b"ACGTAC", b=b"ACGGAC", seed=(0, 0, 6), band=-1) == ARG
        assert call(*ok, a=b"ACGTAC", b=b"ACGGAC", seed=(0, 0, 6), gap_open=1, gap_extend=2) == UNSUPPORTED
    out = {}
    assert _batch(*ok, a=b"ACGTAC", b=b"ACGGAC", seed=(0, 0, 6), cigars=True, cigar_off=True, out=out) == 0
    assert out["cigar"] == "6M"
    assert _batch(*ok, seed=(0, len(B), 0), cigars=True, cigar_off=True, out=out) == 0
    assert out["cigar"] == ""


def test_device_entry_argument_errors():
    """msa_xdrop_flank_run decides its own arguments before it asks for a device: msa_xdrop_extend_run's checks."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    p = 4096  # (never dereferenced on the host)
    for step in (None, p):
        run = lambda **k: L.msa_xdrop_flank_run(*[k.get(s, d) for s, d in (  # noqa: E731
            ("dA", p), ("dB", p), ("np", 1), ("m", p), ("n", p), ("ao", p), ("bo", p), ("step", step), ("sub", None),
            ("match", 2), ("mismatch", -3), ("go", 5), ("ge", 2), ("band", 4), ("xdrop", 10), ("dir", None),
            ("doff", None), ("res", p), ("stream", None))])
        assert run(dA=None) == ARG and run(res=None) == ARG and run(np=0) == ARG and run(band=-1) == ARG
        assert run(dir=p) == ARG                                 # bytes without their offsets
        assert run(band=CAP + 1) == UNSUPPORTED and run(go=1) == UNSUPPORTED and run(ge=-1) == UNSUPPORTED
        assert run(match=128) == UNSUPPORTED and run(match=128, sub=p, band=-1) == ARG


def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_api_argument_errors():
    from cse305_parallel_sequence_alignment_amd import api

    for f, a, b, s in ((api.seed_align, A, B, (4, 6, 3)), (api.seed_align_batch, [A], [B], ([4], [6], [3])),
                       (api.seed_align_batch, [A], B, ([4], [6], [3]))):
        with pytest.raises(TypeError):
            f(a, b, *s)                                          # band is required
        with pytest.raises(ValueError):
            f(a, b, *s, 4, max_symbols=16)
        assert _status(lambda: f(a, b, *s, None)) == ARG         # no band, a negative band: the entries' status
        assert _status(lambda: f(a, b, *s, -1)) == ARG
        assert _status(lambda: f(a, b, *s, band=-2, xdrop=10)) == ARG
        assert _status(lambda: f(a, b, *s, 4, alphabet=b"ACGA", matrix=DNA)) == ARG
        assert _status(lambda: f(a, b, *s, 4, alphabet=b"ACG", matrix=DNA[:3, :3])) == ALPHABET
        assert _status(lambda: f(a, b, *s, 4, gap_open=1, gap_extend=2)) == UNSUPPORTED
        assert _status(lambda: f(a, b, *s, CAP + 1)) in (0, NODEV)   # 12 x 15: band 15 holds every cell
    assert _status(lambda: api.seed_align(A, B, 4, 6, len(A), 4)) == ARG
    assert api.seed_align_batch([], B, [], [], [], 4) == []      # an empty batch
    with pytest.raises(ValueError):
        api.seed_align_batch([A, A], B, [4], [6, 6], [3, 3], 4)  # one seed per pair


def test_api_without_a_flank_to_launch():
    """The whole result dictionary of a call the host answers alone."""
    from cse305_parallel_sequence_alignment_amd import api

    empty = dict(score=0, a_end=0, b_end=0, diagonals=0, dropped=False)
    want = dict(score=7, a_beg=0, b_beg=0, a_end=6, b_end=6, seed_score=7, left=empty, right=empty)
    kw = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2)
    assert api.seed_align(b"ACGTAC", b"ACGGAC", 0, 0, 6, 4, **kw) == dict(want, cigar="6M")
    assert api.seed_align(b"ACGTAC", b"ACGGAC", 0, 0, 6, 4, traceback=False, **kw) == want
    got = api.seed_align_batch([b"ACGTAC", b"ACGTAC"], [b"ACGGAC", b"TTACG"], [0, 0], [0, 2], [6, 3], 0, xdrop=5, **kw)
    assert got == [dict(want, cigar="6M"),
                   dict(score=6, a_beg=0, b_beg=2, a_end=3, b_end=5, seed_score=6, left=empty, right=empty, cigar="3M")]
    assert api.seed_align(b"ACGTAC", b"ACGGAC", 0, 0, 6, 4, max_symbols=32, **kw) == dict(want, cigar="6M")


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
    r = api.seed_align(b"GATTACA", b"GCATN", 2, 1, 2, 3, gap_open=4, gap_extend=1)
    name, args = rec.calls.pop()
    assert name == "msa_seed_align" and len(args) == 21
    assert args[:7] == (b"GATTACA", 7, b"GCATN", 5, 2, 1, 2) and args[7] == b"GATCN" and args[8] == 5
    assert args[10:14] == (4, 1, 3, -1) and all(x is not None for x in args[14:20]) and args[20] > 0
    assert set(r) == {"score", "a_beg", "b_beg", "a_end", "b_end", "seed_score", "left", "right", "cigar"}
    assert set(r["left"]) == set(r["right"]) == {"score", "a_end", "b_end", "diagonals", "dropped"}
    r = api.seed_align(b"GATTACA", b"GCATN", 2, 1, 2, band=3, xdrop=9, traceback=False)
    name, args = rec.calls.pop()
    assert name == "msa_seed_align" and args[12:14] == (3, 9) and args[19] is None and args[20] == 0
    assert "cigar" not in r
    api.seed_align(A, B, 4, 6, 3, 5, xdrop=0, alphabet=b"ACGT", matrix=DNA.tolist(), max_symbols=32)
    name, args = rec.calls.pop()
    assert name == "msa_seed_align32" and args[7] == b"ACGT" and args[12:14] == (5, 0)
    api.seed_align_batch([b"GA", b"TT"], b"CAG", [0, 1], [1, 2], [1, 0], 7, xdrop=11, match=2)
    name, args = rec.calls.pop()
    assert name == "msa_seed_align_batch" and len(args) == 27 and args[4] == 2 and args[15:19] == (3, 1, 7, 11)
    assert all(x is not None for x in args[9:12]) and all(x is not None for x in args[19:25])
    api.seed_align_batch([b"GA", b"TT"], [b"CAG", b"TTTT"], [0, 1], [1, 2], [1, 0], 1, traceback=False, max_symbols=32)
    name, args = rec.calls.pop()
    assert name == "msa_seed_align_batch32" and args[17:19] == (1, -1) and args[24] is None and args[26] is None
    assert not rec.calls


def test_no_device_status():
    """Without a GPU a valid call with a flank to launch returns MSA_ERR_NODEV under its entry's name (no fallback)."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd import api

    n = C.c_int(0)
    if LB.lib().msa_device_count(C.byref(n)) == 0 and n.value > 0:
        return
    ok = (b"ACGT", 4, DNA)
    assert _single(*ok) == NODEV and _single32(*ok) == NODEV and _batch(*ok) == NODEV and _batch32(*ok) == NODEV
    assert _single(*ok, seed=(0, 0, 3)) == NODEV             # the right flank alone
    assert _single(*ok, seed=(len(A) - 3, 6, 3)) == NODEV    # the left flank alone
    assert _batch(*ok, cigars=True, cigar_off=True) == NODEV
    for fn, args, kw, entry in (
            (api.seed_align, (A, B, 4, 6, 3, 3), dict(xdrop=5), "msa_seed_align"),
            (api.seed_align_batch, ([A, A], B, [4, 0], [6, 0], [3, 2], 3), {}, "msa_seed_align_batch"),
            (api.seed_align, (A, B, 4, 6, 3, 0), dict(max_symbols=32), "msa_seed_align32"),
            (api.seed_align_batch, ([A], [B], [4], [6], [3], 3), dict(max_symbols=32, traceback=False),
             "msa_seed_align_batch32")):
        with pytest.raises(LB.MsaError) as e:
            fn(*args, **kw)
        assert e.value.status == NODEV and str(e.value).startswith(entry + ":")
