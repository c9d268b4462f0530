"""Host side of profile alignment (msa_plan_create_profile, msa_profile_align, msa_profile_align_batch,
api.profile_align / profile_align_batch / profile_from_matrix, Plan(profile=)): the exported symbols, the argument
errors in their stated order -- all decided before any device call: without a GPU a valid call is MSA_ERR_NODEV, so
any other status came from the host -- and the api's ValueErrors.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

ARG, ALPHABET, NODEV, UNSUPPORTED = -1, -2, -4, -5
LOCAL, GLOBAL, FIT = 0, 1, 2
AL = b"ACGT"
B = b"ACGTTCGTAGGTT"
PROF = np.array([[2, -3, -3, -3], [-3, 2, -3, -3], [-3, -3, 4, -3], [-3, -3, -3, 2], [1, 1, -2, -2]], dtype=np.int8)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i64(*v):
    return np.array(v, dtype=np.int64)


def _single(mode=LOCAL, prof=PROF, m=None, b=B, n=None, alphabet=AL, n_sym=None, gap_open=5, gap_extend=2):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc = C.c_int32()
    beg, end = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    return LB.lib().msa_profile_align(mode, _p(prof), len(PROF) if m is None else m, b, len(B) if n is None else n,
                                      alphabet, len(AL) if n_sym is None else n_sym, gap_open, gap_extend, C.byref(sc),
                                      _p(beg), _p(end), None, 0)


def _batch(mode=LOCAL, prof=PROF, m=None, b=B, n=None, alphabet=AL, n_sym=None, gap_open=5, gap_extend=2, b_off=0,
           n_pairs=1, arrays=True, cigars=False, cigar_off=False):
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    sc = np.zeros(1, dtype=np.int32)
    beg, end = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    bo, nn = _i64(b_off), _i64(len(B) if n is None else n)
    cig = C.create_string_buffer(256) if cigars else None
    coff = np.zeros(2, dtype=np.int64) if cigar_off else None
    return LB.lib().msa_profile_align_batch(mode, _p(prof), len(PROF) if m is None else m, b, 0 if b is None else len(b),
                                            n_pairs, _p(bo) if arrays else None, _p(nn) if arrays else None, alphabet,
                                            len(AL) if n_sym is None else n_sym, gap_open, gap_extend, _p(sc), _p(beg),
                                            _p(end), cig, 256 if cigars else 0, _p(coff))


def test_new_symbols_exported():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    assert (LB.PROFILE_LOCAL, LB.PROFILE_GLOBAL, LB.PROFILE_FIT) == (0, 1, 2)
    for name in ("msa_plan_create_profile", "msa_profile_align", "msa_profile_align_batch"):
        assert name in LB.EXPORTED
        assert hasattr(L, name), f"libmsa.so does not export {name}"


@pytest.mark.parametrize("call", [_single, _batch], ids=["single", "batch"])
@pytest.mark.parametrize("mode", [LOCAL, GLOBAL, FIT])
def test_entry_argument_errors_in_order(call, mode):
    assert call(mode) == NODEV                                   # a valid call gets as far as the device
    # 1. the mode, the alphabet, the profile pointer
    assert call(3) == ARG and call(-1) == ARG
    assert call(mode, n_sym=0) == ARG
    al33, al32 = bytes(range(65, 98)), bytes(range(65, 97))
    assert call(mode, alphabet=al33, n_sym=33, prof=np.zeros((5, 33), dtype=np.int8)) == ARG
    wide = call(mode, alphabet=al32, n_sym=32, prof=np.zeros((5, 32), dtype=np.int8), b=al32[:13])
    assert wide == (ARG if mode == LOCAL else NODEV)             # 31 symbols for a local call, 32 otherwise
    assert call(mode, alphabet=al32[:31], n_sym=31, prof=np.zeros((5, 31), dtype=np.int8), b=al32[:13]) == NODEV
    assert call(mode, alphabet=b"ACGA") == ARG                   # a duplicate symbol
    assert call(mode, alphabet=None) == ARG
    assert call(mode, prof=None) == ARG
    # ... before everything else: a bad mode with a bad gap rule and a foreign symbol is still ARG
    assert call(3, gap_open=1, gap_extend=-2, b=b"ACGTTCGTAGGTX") == ARG
    assert call(mode, alphabet=b"ACGA", gap_open=1, gap_extend=-2) == ARG
    # 2. the other argument errors, before the gap rule
    assert call(mode, m=0) == ARG
    assert call(mode, n=0) == ARG
    assert call(mode, b=None) == ARG
    assert call(mode, m=(1 << 26) + 1) == ARG
    assert call(mode, n=0, gap_open=1, gap_extend=-2) == ARG
    # 3. the gap rule, before the symbols are looked at
    assert call(mode, gap_open=1, gap_extend=-1) == UNSUPPORTED
    assert call(mode, gap_open=-1, gap_extend=0) == UNSUPPORTED
    assert call(mode, gap_open=1, gap_extend=2) == (NODEV if mode == LOCAL else UNSUPPORTED)  # open >= extend: global
    assert call(mode, gap_open=1, gap_extend=-1, b=b"ACGTTCGTAGGTX") == UNSUPPORTED
    # 4. a symbol of B outside the alphabet
    assert call(mode, b=b"ACGTTCGTAGGTX") == ALPHABET


def test_batch_entry_argument_errors():
    assert _batch(n_pairs=0) == ARG
    assert _batch(arrays=False) == ARG
    assert _batch(cigars=True, cigar_off=False) == ARG           # cigars without cigar_off
    assert _batch(cigars=True, cigar_off=True) == NODEV
    assert _batch(b_off=-1) == ARG
    assert _batch(b_off=1) == ARG                                # B's range leaves the buffer
    assert _batch(n=len(B) + 1) == ARG


def _desc(LB, alg, ms, ns, a_offs, band=-1, cells=0):
    k = len(ms)
    arrs = [(C.c_int64 * k)(*v) for v in (ms, ns, a_offs, [0] * k)]
    d = LB.PlanDesc(alg=alg, cells=cells, match=1, mismatch=0, gap_open=5, gap_extend=2, start_type=-1, band=band,
                    track_end=0, single=int(k == 1), n_pairs=k, m=arrs[0], n=arrs[1], a_off=arrs[2], b_off=arrs[3])
    return d, arrs


def test_plan_create_profile_host_errors():
    """What msa_plan_create_profile decides before it asks for the device."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    f = LB.lib().msa_plan_create_profile
    prof = np.zeros((10, 32), dtype=np.int8)
    h = C.c_void_p()
    d, keep = _desc(LB, LB.SW_SCORED, [10], [20], [0])
    assert f(C.byref(d), None, 10, C.byref(h)) == ARG
    assert f(C.byref(d), _p(prof), 0, C.byref(h)) == ARG
    assert f(None, _p(prof), 10, C.byref(h)) == ARG
    assert f(C.byref(d), _p(prof), 10, C.byref(h)) == NODEV
    for alg in (LB.NW_OVERLAP, LB.NW_EXTEND, LB.SW_AFFINE, LB.NW_ALIGN):
        d, keep = _desc(LB, alg, [10], [20], [0])
        assert f(C.byref(d), _p(prof), 10, C.byref(h)) == UNSUPPORTED
    for ms, offs in (([10], [1]), ([11], [0]), ([4], [-1]), ([4, 4], [0, 7])):
        d, keep = _desc(LB, LB.NW_FIT, ms, [20] * len(ms), offs)
        assert f(C.byref(d), _p(prof), 10, C.byref(h)) == ARG
    d, keep = _desc(LB, LB.NW_FIT, [4, 4, 10], [20] * 3, [0, 6, 0])  # shared rows, a slice ending at the last row
    assert f(C.byref(d), _p(prof), 10, C.byref(h)) == NODEV
    assert not h.value


def test_plan_wrapper_value_errors():
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    prof = np.zeros((10, 32), dtype=np.int8)
    with pytest.raises(ValueError):
        Plan(LB.SW_SCORED, LB.CELLS_NONE, [10], [20], [0], [0], sub=np.zeros((32, 32)), profile=prof)
    for bad in (np.zeros((10, 31)), np.zeros(32), np.zeros((0, 32)), np.full((10, 32), 128)):
        with pytest.raises(ValueError):
            Plan(LB.SW_SCORED, LB.CELLS_NONE, [10], [20], [0], [0], profile=bad)
    with pytest.raises(LB.MsaError) as e:
        Plan(LB.SW_SCORED, LB.CELLS_NONE, [10], [20], [0], [0], profile=prof)
    assert e.value.status == NODEV


def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_api_value_errors():
    from cse305_parallel_sequence_alignment_amd import api

    for f, seq in ((api.profile_align, B), (api.profile_align_batch, [B, B[:5]])):
        with pytest.raises(ValueError):
            f(PROF, seq, AL, mode="overlap")
        with pytest.raises(ValueError):
            f(PROF[0], seq, AL)                                   # not 2-D
        with pytest.raises(ValueError):
            f(PROF.astype(np.int64) * 100, seq, AL)               # not int8-representable
        with pytest.raises(ValueError):
            f(PROF + 0.5, seq, AL)
        with pytest.raises(ValueError):
            f(PROF, seq, b"ACG")                                  # the width is not len(alphabet)
        with pytest.raises(ValueError):
            f(PROF[:, :3], seq, AL)
        for mode in ("local", "global", "fit"):
            assert _status(lambda: f(PROF, seq, AL, mode=mode)) == NODEV
            assert _status(lambda: f(PROF.tolist(), seq, AL, mode=mode, traceback=False)) == NODEV
        assert _status(lambda: f(PROF, seq, b"ACGA")) == ARG
        assert _status(lambda: f(PROF, seq, AL, mode="global", gap_open=1, gap_extend=2)) == UNSUPPORTED
    assert _status(lambda: api.profile_align(PROF, b"ACGN", AL)) == ALPHABET
    assert api.profile_align_batch(PROF, [], AL) == []


def test_profile_from_matrix_by_hand():
    from cse305_parallel_sequence_alignment_amd import api

    S = [[5, -1, -2], [-3, 6, -4], [0, -7, 7]]                   # rows X, Y, Z; not symmetric
    P = api.profile_from_matrix(b"ZXXY", b"XYZ", S)
    assert P.dtype == np.int8 and P.flags["C_CONTIGUOUS"]
    assert P.tolist() == [[0, -7, 7], [5, -1, -2], [5, -1, -2], [-3, 6, -4]]
    assert api.profile_from_matrix("Y", "XYZ", np.array(S)).tolist() == [[-3, 6, -4]]
    with pytest.raises(ValueError):
        api.profile_from_matrix(b"XQ", b"XYZ", S)                # a symbol outside the alphabet
    with pytest.raises(ValueError):
        api.profile_from_matrix(b"XY", b"XY", S)                 # not len(alphabet) x len(alphabet)
    with pytest.raises(ValueError):
        api.profile_from_matrix(b"XY", b"XYX", S)                # a duplicate symbol
    with pytest.raises(ValueError):
        api.profile_from_matrix(b"XY", b"XYZ", np.array(S) * 100)
