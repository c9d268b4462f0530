"""The yardstick of the MSA_SW_SCORED tests (tests/sw_scored_reference.py) against two independent computations -- the
oracle's orc_sw on match / mismatch tables, a plain-Python triple loop on dense asymmetric ones --, the inputs of the
GPU tests tied to a checked answer (the walk's ops, rescored, give the score), and the host side of the new entries:
what is decided before any device call (without a GPU a valid call is MSA_ERR_NODEV, so any other status was decided
on the host).  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import alphabet8 as A8
import sw_scored_reference as SR
import wide_reference as W

ARG, ALPHABET, NODEV, UNSUPPORTED = -1, -2, -4, -5


def _mm(alphabet, match, mismatch):
    k = len(alphabet)
    S = np.full((k, k), mismatch, dtype=np.int64)
    np.fill_diagonal(S, match)
    return S


# the existing SW-affine test pairs (alphabet8's "swa" inputs, 7 symbols), a one-row and a one-column pair
def _sw_pairs():
    out = [A8.named("swa_65x70"), A8.named("swa_300x257")] + list(A8.named("swa_batch"))
    return out + [A8.pair8(91, 1, 40, 7), A8.pair8(92, 40, 1, 7), A8.pair8(93, 64, 64, 7)]


@pytest.mark.parametrize("scores", [(1, 0), (2, -3), (-1, -2)], ids=["1_0", "2_m3", "negative"])
@pytest.mark.parametrize("gaps", [(5, 2), (1, 1), (0, 0)], ids=["5_2", "1_1", "0_0"])
def test_equals_oracle_sw(oracle, scores, gaps):
    """Score, end, beg and CIGAR on match / mismatch tables; the negative-only table gives score-0 pairs."""
    for A, B in _sw_pairs():
        want = oracle.sw(A, B, *scores, *gaps, want_h=True, want_tb=True)
        got = SR.sw_scored_reference(A, B, A8.AL7, _mm(A8.AL7, *scores), *gaps)
        assert (got["score"], got["end"]) == (want["score"], tuple(want["end"]))
        assert (got["H"] == want["H"]).all()
        assert (got["beg"], got["cigar"]) == (tuple(want["beg"]), want["cigar"])
        if scores == (-1, -2):
            assert got["score"] == 0 and got["end"] == (0, 0) and got["ops"] == b""


@pytest.mark.parametrize("w", [8, 32])
@pytest.mark.parametrize("shape", [(40, 40), (37, 23), (1, 40), (40, 1), (1, 1)])
@pytest.mark.parametrize("gaps", [(5, 2), (0, 0), (3, 3)])
def test_equals_triple_loop(w, shape, gaps):
    """H, E, F, the direction byte, the first maximum and the walk on dense asymmetric tables."""
    al, T, _ = SR.width(w)
    rng = np.random.default_rng(1000 * w + 41 * shape[0] + shape[1])
    A, B = SR.homologous(rng, *shape, al) if min(shape) > 30 else (SR.rs(rng, shape[0], al), SR.rs(rng, shape[1], al))
    go, ge = gaps
    ref = SR.sw_scored_reference(A, B, al, T, go, ge)
    H, E, F = SR.sw_triple_loop(A, B, al, T, go, ge)
    m, n = shape
    best, end = 0, (0, 0)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            assert (ref["H"][i, j], ref["E"][i, j], ref["F"][i, j]) == (H[i][j], E[i][j], F[i][j])
            d = H[i - 1][j - 1] + int(T[al.index(A[i - 1:i]), al.index(B[j - 1:j])])
            hs = 0 if H[i][j] == 0 else 1 if H[i][j] == d else 2 if H[i][j] == E[i][j] else 3
            byte = hs | (4 if E[i][j] == H[i][j - 1] - go else 0) | (8 if F[i][j] == H[i - 1][j] - go else 0)
            assert ref["byte"][i, j] == byte
            if H[i][j] > best:
                best, end = H[i][j], (i, j)
    assert (ref["score"], ref["end"]) == (best, end)
    sc, e = SR.rescore(A, B, ref["beg"], ref["ops"], al, T, go, ge)
    assert (sc, e) == (best, end) or best == 0


def test_gpu_inputs_rescore():
    """Every input the GPU tests align: the yardstick's walk, rescored, gives its score and ends at its end cell."""
    for name, A, B, al, S, go, ge in SR.gpu_cases():
        ref = SR.sw_scored_reference(A, B, al, S, go, ge)
        if ref["score"] == 0:
            assert ref["ops"] == b"" and ref["end"] == (0, 0), name
            continue
        assert SR.rescore(A, B, ref["beg"], ref["ops"], al, S, go, ge) == (ref["score"], ref["end"]), name
        assert ref["cigar"] == W.cigar_of(ref["ops"]), name


def test_gpu_inputs_are_what_the_tests_say():
    """The properties the GPU tests lean on, checked where no GPU is needed."""
    for w, k in ((8, 7), (32, 31)):
        al, T, _ = SR.width(w)
        A, B = SR.every_cell(w)
        a, b = W.codes32(A, al), W.codes32(B, al)
        assert np.unique(32 * a[:, None] + b[None, :]).size == k * k and (a == k - 1).any() and (b == k - 1).any()
        zs = [SR.sw_scored_reference(x, y, al, T, SR.GO, SR.GE)["score"] for x, y in SR.ragged_batch(w)]
        assert zs[-1] == 0 and all(z > 0 for z in zs[:-1])
        q, r = SR.planted_twice(w)
        P = SR.planted_table(k)
        ref = SR.sw_scored_reference(q, r, al, P, SR.GO, SR.GE)
        assert ref["score"] == sum(int(P[c, c]) for c in W.codes32(q, al))
        assert np.argwhere(ref["H"] == ref["score"]).tolist() == [[40, 70], [40, 160]] and ref["end"] == (40, 70)
        for L, score in ((516, 65532), (517, 65659)):
            s = al[1:2] * L
            assert SR.sw_scored_reference(s, s, al, SR.self127(k), SR.GO, SR.GE, walk=False)["score"] == score
    S, A, B = SR.extreme31()
    ref = SR.sw_scored_reference(A, B, SR.AL31, S, SR.GO, SR.GE)
    plain = SR.sw_scored_reference(A, B, SR.AL31, SR.T31, SR.GO, SR.GE)
    assert ref["score"] > 19 * 127 and (ref["score"], ref["cigar"]) != (plain["score"], plain["cigar"])
    assert b"I" in ref["ops"] or b"D" in ref["ops"]  # round the -128, not through it
    A, B, (a0, a1), (b0, b1) = SR.protein_case()
    ref = SR.sw_scored_reference(A, B, W.AL20, W.protein20(), SR.PGO, SR.PGE)
    # the local alignment holds the planted regions (a few symbols may be trimmed, and it may run on into the flanks)
    assert ref["beg"][0] - 1 <= a0 + 5 and ref["end"][0] >= a1 - 5
    assert ref["beg"][1] - 1 <= b0 + 5 and ref["end"][1] >= b1 - 5
    assert ref["score"] >= 150 * 4 * 0.8


# ---- the host side of the entries -------------------------------------------------------------------------------
A, B = b"ACGTACGTAC", b"TTACGTTCGTAGG"
DNA = np.array([[2, -3, -3, -3], [-3, 2, -3, -3], [-3, -3, 2, -3], [-3, -3, -3, 2]], dtype=np.int8)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _single(name):
    def call(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, m=None, n=None):
        from cse305_parallel_sequence_alignment_amd import _lib as LB

        sc, ei, ej = C.c_int32(), C.c_int64(), C.c_int64()
        return getattr(LB.lib(), name)(a, len(a) if m is None else m, b, len(b) if n is None else n, alphabet, n_sym,
                                       _p(sub), gap_open, gap_extend, C.byref(sc), C.byref(ei), C.byref(ej), None,
                                       None, None, 0)
    return call


def _batch(name):
    def call(alphabet, n_sym, sub, a=A, b=B, gap_open=5, gap_extend=2, m=None, n=None, n_pairs=1, a_off=0,
             cigars=False):
        from cse305_parallel_sequence_alignment_amd import _lib as LB

        sc, end = np.zeros(1, dtype=np.int32), np.zeros(2, dtype=np.int64)
        ao, bo = np.array([a_off], dtype=np.int64), np.zeros(1, dtype=np.int64)
        mm = np.array([len(a) if m is None else m], dtype=np.int64)
        nn = np.array([len(b) if n is None else n], dtype=np.int64)
        cig = C.create_string_buffer(64) if cigars else None
        return getattr(LB.lib(), name)(a, len(a), b, len(b), n_pairs, _p(ao), _p(mm), _p(bo), _p(nn), alphabet, n_sym,
                                       _p(sub), gap_open, gap_extend, _p(sc), _p(end), None, cig, 64 if cigars else 0,
                                       None)
    return call


ENTRIES = {"msa_sw_align_scored": (_single, 7), "msa_sw_align_scored32": (_single, 31),
           "msa_sw_align_batch_scored": (_batch, 7), "msa_sw_align_batch_scored32": (_batch, 31)}


def test_new_symbols_exported():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    assert LB.SW_SCORED == 8
    for name in ENTRIES:
        assert name in LB.EXPORTED
        assert hasattr(LB.lib(), name), f"libmsa.so does not export {name}"


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_argument_errors(name):
    make, limit = ENTRIES[name]
    call = make(name)
    over = W.AL32[:limit + 1]  # 8 symbols for the plain entries, 32 for the wide ones
    assert call(over, limit + 1, np.zeros((limit + 1, limit + 1), dtype=np.int8)) == ARG
    assert call(b"", 0, DNA) == ARG                            # n_sym 0
    assert call(b"ACGA", 4, DNA) == ARG                        # a duplicate symbol
    assert call(None, 4, DNA) == ARG                           # no alphabet
    assert call(b"ACGT", 4, None) == ARG                       # no matrix
    assert call(b"ACGT", 4, DNA, m=0) == ARG                   # an empty A
    assert call(b"ACGT", 4, DNA, n=0) == ARG
    assert call(b"ACGT", 4, DNA, gap_open=-1) == UNSUPPORTED   # the gap rule: both >= 0 ...
    assert call(b"ACGT", 4, DNA, gap_extend=-1) == UNSUPPORTED
    # ... before the symbols are looked at, and gap_open < gap_extend is no error for a local alignment
    assert call(b"ACGT", 4, DNA, a=b"ACGNACGT", gap_open=-1) == UNSUPPORTED
    assert call(b"ACGT", 4, DNA, a=b"ACGNACGT") == ALPHABET    # a symbol of A outside the alphabet
    assert call(b"ACGT", 4, DNA, b=b"ACGTTCGTX") == ALPHABET   # ... of B
    assert call(b"ACGT", 4, DNA, a=b"ACGNACGT", gap_open=1, gap_extend=2) == ALPHABET
    if make is _batch:
        assert call(b"ACGT", 4, DNA, n_pairs=0) == ARG
        assert call(b"ACGT", 4, DNA, a_off=1) == ARG           # the range leaves A
        assert call(b"ACGT", 4, DNA, cigars=True) == ARG       # cigars without cigar_off
    # the sentinel takes a code: the largest alphabet each entry accepts reaches the device check
    ok = W.AL32[:limit]
    assert call(ok, limit, np.zeros((limit, limit), dtype=np.int8), a=ok, b=ok) in (0, NODEV)


def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_api_argument_errors():
    from cse305_parallel_sequence_alignment_amd import api

    for f, a, b in ((api.sw_align, A, B), (api.sw_align_batch, [A], [B]), (api.sw_align_batch, [A], B)):
        for ms in (8, 32):
            with pytest.raises(ValueError):
                f(a, b, matrix=DNA, max_symbols=ms)                                # matrix without alphabet
            with pytest.raises(ValueError):
                f(a, b, alphabet=b"ACGT", matrix=DNA, match=2, max_symbols=ms)     # matrix with match
            with pytest.raises(ValueError):
                f(a, b, alphabet=b"ACGT", matrix=DNA, mismatch=-1, max_symbols=ms)
            with pytest.raises(ValueError):
                f(a, b, alphabet=b"ACGT", max_symbols=ms)                          # alphabet without matrix
            with pytest.raises(ValueError):
                f(a, b, alphabet=b"ACG", matrix=DNA, max_symbols=ms)               # not len(alphabet) squared
            assert _status(lambda: f(a, b, alphabet=b"ACGA", matrix=DNA, max_symbols=ms)) == ARG
            assert _status(lambda: f(a, b, alphabet=b"ACG", matrix=DNA[:3, :3], max_symbols=ms)) == ALPHABET
            assert _status(lambda: f(a, b, alphabet=b"ACGT", matrix=DNA, gap_open=-1, max_symbols=ms)) == UNSUPPORTED
        with pytest.raises(ValueError):
            f(a, b, max_symbols=16)
    # eight symbols: one too many for the plain entry, fine for the wide one (which then asks for the device)
    al8 = b"ACGTNRYK"
    S8 = np.zeros((8, 8), dtype=np.int8)
    assert _status(lambda: api.sw_align(al8, al8, alphabet=al8, matrix=S8)) == ARG
    assert _status(lambda: api.sw_align(al8, al8, alphabet=al8, matrix=S8, max_symbols=32)) in (0, NODEV)
    # match / mismatch with max_symbols=32: the sequences' own symbols, at most 31
    assert _status(lambda: api.sw_align(W.AL32, W.AL32, match=2, max_symbols=32)) == ALPHABET
    assert _status(lambda: api.sw_align(W.AL32[:31], W.AL32[:31], match=2, max_symbols=32)) in (0, NODEV)


def test_api_default_call_is_todays(monkeypatch):
    """With nothing new passed, sw_align / sw_align_batch build exactly the msa_sw_align / msa_sw_align_batch call
    (match 1, mismatch 0 unless given); anything new reaches the matrix entries."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd import api

    calls = []

    class Spy:
        def __getattr__(self, name):
            def f(*args):
                calls.append((name, args))
                return 0
            return f

    monkeypatch.setattr(LB, "lib", lambda: Spy())
    api.sw_align(A, B)
    api.sw_align(A, B, match=2, mismatch=-3, gap_open=5, gap_extend=2)
    api.sw_align_batch([A], [B])
    api.sw_align_batch([A], B, 3, -1)
    assert [c[0] for c in calls] == ["msa_sw_align", "msa_sw_align", "msa_sw_align_batch", "msa_sw_align_batch"]
    assert calls[0][1][4:8] == (1, 0, 1, 1) and calls[1][1][4:8] == (2, -3, 5, 2)
    assert calls[2][1][9:13] == (1, 0, 1, 1) and calls[3][1][9:13] == (3, -1, 1, 1)
    del calls[:]
    api.sw_align(A, B, alphabet=b"ACGT", matrix=DNA)
    api.sw_align(A, B, alphabet=b"ACGT", matrix=DNA, max_symbols=32)
    api.sw_align(A, B, max_symbols=32)
    api.sw_align_batch([A], [B], alphabet=b"ACGT", matrix=DNA)
    api.sw_align_batch([A], [B], match=2, max_symbols=32)
    assert [c[0] for c in calls] == ["msa_sw_align_scored", "msa_sw_align_scored32", "msa_sw_align_scored32",
                                     "msa_sw_align_batch_scored", "msa_sw_align_batch_scored32"]
    # max_symbols=32 with match / mismatch: the sequences' symbols in first-seen order under +match / mismatch
    name, args = calls[2]
    assert bytes(args[4]) == b"ACGT" and args[5] == 4
