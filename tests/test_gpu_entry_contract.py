"""What the ten host alignment entries return, pinned kind by kind: msa_sw_align, msa_nw_align, msa_nw_align_scored
and msa_fit_align, and the batch entry of each.  The single entry and the batch entry of a kind must agree on every
pair (score, end / span, CIGAR), both with the project's yardsticks (oracle.sw, tests/nw_reference.py,
nw_scored_reference.py, fit_reference.py -- never with the library itself), and a CIGAR buffer one byte short is
MSA_ERR_CAPACITY with everything but the CIGAR written.

The pairs are the smallest at which the host side of an entry can go wrong: 1 x 1; 1 x 70 and 70 x 1 (a global walk
ends on the top or the left border: the completion is all 'D' or all 'I'); 63, 64 and 65 rows against 66 columns
(the 64-row stripe edge); 130 x 200 whose columns hold 40 symbols in the middle and 30 at the end that the rows lack
(three stripes: the walk crosses two stripe borders, and a 40-symbol deletion).  |130 - 200| exceeds a band of 8, so
the band-8 case runs a 130-row pair of its own (130 x 128, two symbols of the rows missing in the columns)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import fit_reference as FR
import nw_reference as R
import nw_scored_reference as RS
from nw_reference import rs

pytestmark = pytest.mark.gpu

CAPACITY = -8
KINDS = ["sw", "nw", "scored", "fit"]
SW = dict(match=2, mismatch=-1, gap_open=3, gap_extend=1)
NW_G, NW_H = 1, 2                                    # msa_nw_align: +1 / 0, gap_open 3, gap_extend 1
SC_AL, SC_S, SC_G, SC_H = RS.SCORE_SETS["asym"]      # msa_nw_align_scored: an asymmetric matrix
FIT_AL, FIT_S, FIT_G, FIT_H = RS.SCORE_SETS["dna"]   # msa_fit_align: +2 / -3, g = 2, h = 3


@functools.lru_cache(maxsize=None)
def pairs():
    rng = np.random.default_rng(9100)
    P, Q, Z, T = rs(rng, 60), rs(rng, 70), rs(rng, 40), rs(rng, 30)
    B66 = rs(rng, 66)
    out = {
        "1x1": (b"A", b"A"),
        "1x70": (b"G", b"ACGT" * 17 + b"AC"),
        "70x1": (b"ACGT" * 17 + b"AC", b"G"),
        "63x66": (B66[2:65], B66),
        "64x66": (B66[:40] + B66[42:], B66),
        "65x66": (B66[:20] + B66[21:], B66),
        "130x200": (P + Q, P + Z + Q + T),
    }
    for name, (a, b) in out.items():
        assert f"{len(a)}x{len(b)}" == name
    return out


@functools.lru_cache(maxsize=None)
def band_pair():
    """130 x 128 within a band of 8: three substitutions and a 2-symbol deletion."""
    A = bytearray(rs(np.random.default_rng(9101), 130))
    B = bytearray(A)
    for k in (7, 64, 120):
        B[k] = b"ACGT"[(b"ACGT".index(B[k]) + 1) % 4]
    del B[90:92]
    return bytes(A), bytes(B)


_WANT = {}


def want(oracle, kind, A, B, band=-1):
    """The yardstick's answer in the form the api returns it, computed once per case and shared (never modified)."""
    key = (kind, A, B, band)
    if key not in _WANT:
        if kind == "sw":
            o = oracle.sw(A, B, SW["match"], SW["mismatch"], SW["gap_open"], SW["gap_extend"], want_tb=True)
            w = dict(score=o["score"], end=tuple(o["end"]), beg=tuple(o["beg"]), cigar=o["cigar"])
        elif kind == "nw":
            r = R.nw_reference(A, B, NW_G, NW_H, band)
            w = dict(score=r["score"], cigar=R.cigar_of(r["ops"]))
        elif kind == "scored":
            r = RS.nw_scored_reference(A, B, SC_AL, SC_S, SC_G, SC_H, band)
            w = dict(score=r["score"], cigar=R.cigar_of(r["ops"]))
        else:
            r = FR.fit_reference(A, B, FIT_AL, FIT_S, FIT_G, FIT_H)
            w = dict(score=r["score"], beg=r["beg_j"], end=r["end_j"], cigar=FR.cigar_of(r["ops"]))
        _WANT[key] = w
    return _WANT[key]


def _kw(kind, band):
    if kind == "sw":
        return dict(SW)
    if kind == "nw":
        return dict(gap_open=NW_G + NW_H, gap_extend=NW_G, band=band)
    if kind == "scored":
        return dict(alphabet=SC_AL, matrix=SC_S, gap_open=SC_G + SC_H, gap_extend=SC_G, band=band)
    return dict(alphabet=FIT_AL, matrix=FIT_S, gap_open=FIT_G + FIT_H, gap_extend=FIT_G)


def single(kind, A, B, band=-1, **kw):
    from cse305_parallel_sequence_alignment_amd import api

    fn = {"sw": api.sw_align, "nw": api.nw_align, "scored": api.nw_align, "fit": api.fit_align}[kind]
    return fn(A, B, **_kw(kind, band), **kw)


def batch(kind, As, Bs, band=-1, **kw):
    from cse305_parallel_sequence_alignment_amd import api

    fn = {"sw": api.sw_align_batch, "nw": api.nw_align_batch, "scored": api.nw_align_batch,
          "fit": api.fit_align_batch}[kind]
    return fn(As, Bs, **_kw(kind, band), **kw)


def _no_cigar(kind, w):
    """What traceback=False returns: no CIGAR and no start (SW drops `beg`, fit reports None)."""
    if kind == "sw":
        return dict(score=w["score"], end=w["end"])
    if kind == "fit":
        return dict(score=w["score"], beg=None, end=w["end"])
    return dict(score=w["score"])


# ---- single entry == batch of one == yardstick ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x1", "1x70", "70x1", "63x66", "64x66", "65x66", "130x200"])
@pytest.mark.parametrize("kind", KINDS)
def test_single_equals_batch_of_one(oracle, dev, kind, name):
    A, B = pairs()[name]
    w = want(oracle, kind, A, B)
    assert single(kind, A, B) == w
    assert batch(kind, [A], [B]) == [w]
    assert single(kind, A, B, traceback=False) == _no_cigar(kind, w)
    assert batch(kind, [A], [B], traceback=False) == [_no_cigar(kind, w)]


def _runs(cigar):
    return [(int(k), op) for k, op in re.findall(r"(\d+)([MID])", cigar)]


def test_border_completions(oracle, dev):
    """(the inputs do what they are there for) The global walk of the one-row pair stops on the top border and that
    of the one-column pair on the left border: the CIGAR starts with the completion, one gap along the border; the
    130-row pair has its 40-symbol deletion."""
    c = _runs(want(oracle, "nw", *pairs()["1x70"])["cigar"])
    assert c[0][1] == "D" and {op for _, op in c} == {"M", "D"} and sum(k for k, op in c if op == "D") == 69
    c = _runs(want(oracle, "nw", *pairs()["70x1"])["cigar"])
    assert c[0][1] == "I" and {op for _, op in c} == {"M", "I"} and sum(k for k, op in c if op == "I") == 69
    c = _runs(want(oracle, "nw", *pairs()["130x200"])["cigar"])
    assert (40, "D") in c


@pytest.mark.parametrize("kind", ["nw", "scored"])
def test_bands(oracle, dev, kind):
    """No band, a band of max(m, n) (which holds every cell: treated as no band) and a band of 8."""
    A, B = pairs()["130x200"]
    w = want(oracle, kind, A, B)
    for band in (-1, 200):
        assert single(kind, A, B, band=band) == w
        assert batch(kind, [A], [B], band=band) == [w]
    A, B = band_pair()
    w8 = want(oracle, kind, A, B, 8)
    assert "2I" in w8["cigar"]
    assert single(kind, A, B, band=8) == w8
    assert batch(kind, [A], [B], band=8) == [w8]
    assert single(kind, A, B, band=8, traceback=False) == dict(score=w8["score"])


def test_fit_whole_query_inserted(oracle, dev):
    A, B = b"A" * 5, b"C" * 9
    w = want(oracle, "fit", A, B)
    assert w["cigar"] == "5I" and w["beg"] == w["end"]
    assert single("fit", A, B) == w
    assert batch("fit", [A], [B]) == [w]


def test_fit_free_reference_on_both_sides(oracle, dev):
    A, B = FR.planted(9102, 40, 120, 30)
    w = want(oracle, "fit", A, B)
    assert 0 < w["beg"] < w["end"] < len(B)
    assert single("fit", A, B) == w
    assert batch("fit", [A], [B]) == [w]


# ---- capacity --------------------------------------------------------------------------------------------------
def _i64(*v):
    return (C.c_int64 * len(v))(*v)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def raw_single(L, kind, A, B, cap):
    """One call of the kind's single entry with a CIGAR buffer of `cap` bytes and every output prefilled with -77:
    (status, score, span as the entry reports it, CIGAR)."""
    sc = C.c_int32(-77)
    v = [C.c_int64(-77) for _ in range(4)]
    cig = C.create_string_buffer(max(cap, 1))
    if kind == "sw":
        rc = L.msa_sw_align(A, len(A), B, len(B), SW["match"], SW["mismatch"], SW["gap_open"], SW["gap_extend"],
                            C.byref(sc), C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), cig, cap)
    elif kind == "nw":
        rc = L.msa_nw_align(A, len(A), B, len(B), NW_G + NW_H, NW_G, -1, C.byref(sc), cig, cap)
    elif kind == "scored":
        S = np.ascontiguousarray(SC_S, dtype=np.int8)
        rc = L.msa_nw_align_scored(A, len(A), B, len(B), SC_AL, len(SC_AL), _p(S), SC_G + SC_H, SC_G, -1, C.byref(sc),
                                   cig, cap)
    else:
        S = np.ascontiguousarray(FIT_S, dtype=np.int8)
        rc = L.msa_fit_align(A, len(A), B, len(B), FIT_AL, len(FIT_AL), _p(S), FIT_G + FIT_H, FIT_G, C.byref(sc),
                             C.byref(v[0]), C.byref(v[1]), cig, cap)
    return rc, sc.value, tuple(x.value for x in v), cig.value.decode()


@pytest.mark.parametrize("kind", KINDS)
def test_single_capacity(oracle, dev, kind):
    from cse305_parallel_sequence_alignment_amd import _lib

    L = _lib.lib()
    A, B = pairs()["65x66"]
    w = want(oracle, kind, A, B)
    need = len(w["cigar"]) + 1
    rc, score, span, cigar = raw_single(L, kind, A, B, need)
    assert (rc, score, cigar) == (0, w["score"], w["cigar"])
    rc, score, short, _ = raw_single(L, kind, A, B, need - 1)
    assert rc == CAPACITY and score == w["score"]
    if kind == "sw":
        assert span == short == w["end"] + w["beg"]
    elif kind == "fit":
        assert span == short == (w["beg"], w["end"], -77, -77)


@pytest.mark.parametrize("kind", KINDS)
def test_batch_capacity(oracle, dev, kind):
    """A cigars buffer one byte short: MSA_ERR_CAPACITY, every score and cigar_off[0..n_pairs] written."""
    from cse305_parallel_sequence_alignment_amd import _lib, api

    L = _lib.lib()
    names = ["65x66", "1x70", "63x66"]
    ps = [pairs()[k] for k in names]
    ws = [want(oracle, kind, a, b) for a, b in ps]
    A, B, a_off, m, b_off, n = api._batch_in([a for a, _ in ps], [b for _, b in ps])
    k = len(ps)
    offs = [0]
    for w in ws:
        offs.append(offs[-1] + len(w["cigar"]) + 1)

    def call(cap):
        sc = np.full(k, -77, dtype=np.int32)
        coff = np.full(k + 1, -77, dtype=np.int64)
        two = np.full((2, k, 2), -77, dtype=np.int64)
        cig = C.create_string_buffer(max(cap, 1))
        head = (A, len(A), B, len(B), k, _p(a_off), _p(m), _p(b_off), _p(n))
        if kind == "sw":
            rc = L.msa_sw_align_batch(*head, SW["match"], SW["mismatch"], SW["gap_open"], SW["gap_extend"], _p(sc),
                                      _p(two[0]), _p(two[1]), cig, cap, _p(coff))
        elif kind == "nw":
            rc = L.msa_nw_align_batch(*head, NW_G + NW_H, NW_G, -1, _p(sc), cig, cap, _p(coff))
        elif kind == "scored":
            S = np.ascontiguousarray(SC_S, dtype=np.int8)
            rc = L.msa_nw_align_batch_scored(*head, SC_AL, len(SC_AL), _p(S), SC_G + SC_H, SC_G, -1, _p(sc), cig, cap,
                                             _p(coff))
        else:
            S = np.ascontiguousarray(FIT_S, dtype=np.int8)
            rc = L.msa_fit_align_batch(*head, FIT_AL, len(FIT_AL), _p(S), FIT_G + FIT_H, FIT_G, _p(sc), _p(two[0]),
                                       cig, cap, _p(coff))
        return rc, sc.tolist(), coff.tolist(), two, cig.raw

    rc, sc, coff, two, raw = call(offs[-1])
    assert rc == 0 and sc == [w["score"] for w in ws] and coff == offs
    assert [raw[offs[p]:offs[p + 1] - 1].decode() for p in range(k)] == [w["cigar"] for w in ws]
    rc, sc, coff, short, _ = call(offs[-1] - 1)
    assert rc == CAPACITY and sc == [w["score"] for w in ws] and coff == offs
    assert (short == two).all()
    if kind == "sw":
        assert two[0].tolist() == [list(w["end"]) for w in ws] and two[1].tolist() == [list(w["beg"]) for w in ws]
    elif kind == "fit":
        assert two[0].tolist() == [[w["beg"], w["end"]] for w in ws]


# ---- chunks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_chunked_batch_equals_unchunked(oracle, dev, kind):
    """Five pairs of mixed sizes under a device budget small enough for at least two chunks."""
    from cse305_parallel_sequence_alignment_amd import _lib

    L = _lib.lib()
    ps = [pairs()[k] for k in ("130x200", "1x1", "64x66", "70x1", "65x66")]
    As, Bs = [a for a, _ in ps], [b for _, b in ps]
    ws = [want(oracle, kind, a, b) for a, b in ps]
    assert batch(kind, As, Bs) == ws

    def admitted():
        v = (C.c_int64 * 5)()
        assert L.msa_device_budget_info(v) == 0
        return int(v[4])

    try:
        budget = 256 << 20
        while True:
            assert L.msa_set_device_budget(budget) == 0
            before = admitted()
            got = batch(kind, As, Bs)
            if admitted() - before >= 2:
                break
            budget //= 2
            assert budget >= 1 << 20, "the batch never split"
        assert got == ws
    finally:
        L.msa_set_device_budget(0)
