"""Banded extension alignment with X-drop termination (msa_xdrop.hip: msa_xdrop_extend_run / msa_xdrop_extend_walk,
the msa_extend_align_xdrop entries, api.extend_align(band=, xdrop=)) against the numpy yardstick
tests/xdrop_reference.py (itself checked against a triple loop and the banded yardstick in test_xdrop_reference.py).

Every device case checks, exactly (integer DP): the score, the end cell, D (`diagonals`), H(m', n') or MSA_SCORE_NONE,
the status and the number of cells computed; bits 0-1 of every in-band interior direction byte with i + j <= D, bit 2
where E is finite and bit 3 where F is finite (the plane is pre-filled with 0xFF); the walk's ops byte for byte, its
stop cell and the CIGAR with its border gap; and that ops bytes outside a pair's n_ops keep their poison.  The shapes are
the smallest at which each mechanism can fail: bands 0 / 1 / 8 / 16 / 64 with clipped pairs and empty extensions for the
equality with the banded extension; bands around one and two lane chunks of 64; the band cap; the prototype cases of
the stopping rule at every listed xdrop; the exact threshold; a row-major tie on a later anti-diagonal; batches that
are no multiple of the four pairs of a workgroup; 24 symbols."""
import ctypes as C
import functools

import numpy as np
import pytest

import extend_band_reference as XB
import extend_reference as ER
import wide_reference as W
import xdrop_reference as XD

pytestmark = pytest.mark.gpu

UNSUPPORTED = -5
POISON_DIR, POISON_OPS = 0xFF, 0xEE


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _t(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _table32(S):
    S = np.asarray(S)
    out = np.zeros((32, 32), dtype=np.int8)
    out[:S.shape[0], :S.shape[1]] = S
    return out.reshape(-1)


def _run(LB, dev, pairs, alphabet, S, g, h, w, xdrop, mm=False):
    """msa_xdrop_extend_run and msa_xdrop_extend_walk over the CLIPPED pairs (their offsets are the unclipped
    sequences': a prefix is kept) -> per pair dict(res = the 8 result words, byte = the band-form plane, ops, stop,
    status, tail = the pair's ops bytes past n_ops).  mm: scores through match / mismatch, no table."""
    import torch

    K = len(pairs)
    sizes = [XB.clip(len(a), len(b), w) for a, b in pairs]
    ms = np.array([s[0] for s in sizes], dtype=np.int64)
    ns = np.array([s[1] for s in sizes], dtype=np.int64)
    la = np.array([len(a) for a, _ in pairs], dtype=np.int64)
    lb = np.array([len(b) for _, b in pairs], dtype=np.int64)
    ao = np.concatenate(([0], np.cumsum(la)[:-1])).astype(np.int64)
    bo = np.concatenate(([0], np.cumsum(lb)[:-1])).astype(np.int64)
    dA = _t(np.concatenate([ER.codes(a, alphabet) for a, _ in pairs]).astype(np.uint8), dev)
    dB = _t(np.concatenate([ER.codes(b, alphabet) for _, b in pairs]).astype(np.uint8), dev)
    doff = np.concatenate(([0], np.cumsum((2 * w + 1) * (ms + 1)))).astype(np.int64)
    ooff = np.concatenate(([0], np.cumsum((ms + ns + 2 + 15) // 16 * 16))).astype(np.int64)
    dm, dn, dao, dbo, ddoff, dooff = (_t(x, dev) for x in (ms, ns, ao, bo, doff, ooff))
    tab = None if mm else _t(_table32(S), dev)
    dDir = torch.full((int(doff[-1]),), POISON_DIR, dtype=torch.uint8, device=dev)
    dOps = torch.full((int(ooff[-1]),), POISON_OPS, dtype=torch.uint8, device=dev)
    dRes = torch.zeros(8 * K, dtype=torch.int64, device=dev)
    dInfo = torch.zeros(8 * K, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = LB.lib()
    LB.check(L.msa_xdrop_extend_run(_ptr(dA), _ptr(dB), K, _ptr(dm), _ptr(dn), _ptr(dao), _ptr(dbo),
                                    None if mm else _ptr(tab), int(S[0][0]), int(S[0][1]), g + h, g, w, xdrop,
                                    _ptr(dDir), _ptr(ddoff), _ptr(dRes), st), "msa_xdrop_extend_run")
    LB.check(L.msa_xdrop_extend_walk(K, w, _ptr(dDir), _ptr(ddoff), _ptr(dRes), _ptr(dOps), _ptr(dooff), _ptr(dInfo),
                                     st), "msa_xdrop_extend_walk")
    torch.cuda.synchronize(dev)
    res, info = dRes.cpu().numpy().reshape(K, 8), dInfo.cpu().numpy().reshape(K, 8)
    byte, ops = dDir.cpu().numpy(), dOps.cpu().numpy()
    out = []
    for p in range(K):
        seg = ops[ooff[p]:ooff[p + 1]]
        n_ops = int(info[p, 0])
        out.append(dict(res=[int(x) for x in res[p]], byte=byte[doff[p]:doff[p + 1]].reshape(int(ms[p]) + 1, 2 * w + 1),
                        ops=seg[:n_ops].tobytes(), stop=(int(info[p, 1]) - 1, int(info[p, 2]) - 1),
                        status=int(info[p, 3]), tail=seg[n_ops:], info=[int(x) for x in info[p]]))
    return out


def _check(LB, got, ref):
    """One pair of _run against its xdrop_reference (or, never stopping, extend_band_reference) dictionary."""
    me, ne, w = ref["m_eff"], ref["n_eff"], ref["w"]
    D = ref.get("diagonals", me + ne)
    dropped = D < me + ne
    live = ref.get("live", ref["valid"])
    score, ei, ej, gD, fin, status, cells, zero = got["res"]
    assert (score, (ei, ej), gD, status, zero) == (ref["score"], ref["end"], D, 0, 0)
    assert fin == (LB.SCORE_NONE if dropped else int(ref["H"][me, ne - me + w]))
    if not dropped and ref["global_score"] is not None:
        assert fin == ref["global_score"]
    assert cells == int(live.sum())
    b = got["byte"]
    bad = live & ((b & 3) != (ref["byte"] & 3))
    assert not bad.any(), ("bits 0-1", int(bad.sum()), np.argwhere(bad)[:4])
    bad = live & ref["efin"] & ((b & 4) != (ref["byte"] & 4))
    assert not bad.any(), ("bit 2", int(bad.sum()), np.argwhere(bad)[:4])
    bad = live & ref["ffin"] & ((b & 8) != (ref["byte"] & 8))
    assert not bad.any(), ("bit 3", int(bad.sum()), np.argwhere(bad)[:4])
    # nothing outside the band form's in-band interior is written, and no byte of a cell is left unwritten
    assert (b[~ref["valid"]] == POISON_DIR).all() and (b[live] != POISON_DIR).all()
    assert got["status"] == 0 and got["info"][4:] == [0, 0, 0, 0]
    assert got["ops"] == ref["walk_ops"] and got["stop"] == ref["stop"]
    assert XB.cigar_of(got["ops"] + b"I" * got["stop"][0] + b"D" * got["stop"][1]) == XB.cigar_of(ref["ops"])
    assert (got["tail"] == POISON_OPS).all()


def _want(ref, traceback=True):
    me, ne = ref["m_eff"], ref["n_eff"]
    D = ref.get("diagonals", me + ne)
    r = dict(score=ref["score"], a_end=ref["end"][0], b_end=ref["end"][1],
             global_score=None if D < me + ne else ref["global_score"], diagonals=D, dropped=D < me + ne)
    if traceback:
        r["cigar"] = XB.cigar_of(ref["ops"])
    return r


def _api_kw(alphabet, S, g, h, w, xdrop):
    return dict(alphabet=alphabet, matrix=S, gap_open=g + h, gap_extend=g, band=w, xdrop=xdrop,
                max_symbols=32 if len(alphabet) > 8 else 8)


# ---- 1. never stopping: the banded extension in every field ----------------------------------------------------------
EQUAL = [k for k, v in XB.CASES.items() if v[1] in (0, 1, 8, 16, 64)]
assert {"clip_rows_400x150_w16", "clip_cols_150x400_w16", "all_negative_w16", "best_zero_w8"} <= set(EQUAL)


@pytest.mark.parametrize("xdrop", [-1, 2 ** 30], ids=["neg", "huge"])
@pytest.mark.parametrize("name", EQUAL)
def test_equals_the_banded_extension(dev, LB, name, xdrop):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, alphabet, S, g, h, w, ref = XB.case(name)
    got, = _run(LB, dev, [(A, B)], alphabet, S, g, h, w, xdrop, mm=name in ("random_400_w64", "similar_150_w8"))
    _check(LB, got, ref)
    if name in XB.KNOWN:
        score, end, cigar, _ = XB.KNOWN[name]
        assert (got["res"][0], tuple(got["res"][1:3])) == (score, end)
    kw = _api_kw(alphabet, S, g, h, w, xdrop)
    r = api.extend_align(A, B, **kw)
    assert r == _want(ref)
    kw.pop("xdrop")
    banded = api.extend_align(A, B, **kw)   # the stripe kernel's banded extension on the same input
    assert {k: v for k, v in r.items() if k not in ("diagonals", "dropped")} == banded


# ---- 2. bands around one and two chunks of 64 lanes ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _similar_150x140():
    A, B = XB.similar(np.random.default_rng(410), 170)
    return A[:150], B[:140]


@pytest.mark.parametrize("w", [62, 63, 64, 65, 127, 128])
def test_lane_chunk_edges(dev, LB, w):
    A, B = _similar_150x140()
    alphabet, S, g, h = XB.score_set("dna")
    ref = XB.extend_band_reference(A, B, alphabet, S, g, h, w)
    got, = _run(LB, dev, [(A, B)], alphabet, S, g, h, w, -1)
    _check(LB, got, ref)


# ---- 3. the band cap -----------------------------------------------------------------------------------------------
def test_band_cap(dev, LB):
    import torch

    from cse305_parallel_sequence_alignment_amd import api

    cap = LB.XDROP_BAND_MAX
    assert cap >= 512
    rng = np.random.default_rng(411)
    A = XB.rs(rng, 700)
    B = A[:300] + XB.rs(rng, 30) + A[300:650]   # a 30-symbol insertion: the path leaves the main diagonal
    alphabet, S, g, h = XB.score_set("dna")
    ref = XB.extend_band_reference(A, B, alphabet, S, g, h, cap)
    got, = _run(LB, dev, [(A, B)], alphabet, S, g, h, cap, -1)
    _check(LB, got, ref)
    assert api.extend_align(A, B, **_api_kw(alphabet, S, g, h, cap, -1)) == _want(ref)
    with pytest.raises(LB.MsaError) as e:
        api.extend_align(A, B, **_api_kw(alphabet, S, g, h, cap + 1, -1))
    assert e.value.status == UNSUPPORTED
    z = torch.zeros(64, dtype=torch.int64, device=dev)
    rc = LB.lib().msa_xdrop_extend_run(_ptr(z), _ptr(z), 1, _ptr(z), _ptr(z), _ptr(z), _ptr(z), None, 2, -3, 5, 2,
                                       cap + 1, -1, None, None, _ptr(z), None)
    assert rc == UNSUPPORTED


# ---- 4. stops: the prototype cases at every listed xdrop -------------------------------------------------------------
STOP_CASES = [(name, x) for name, v in XD.STOPS.items() for x in v[3]]


@pytest.mark.parametrize("name, xdrop", STOP_CASES, ids=[f"{n}-x{x}" for n, x in STOP_CASES])
def test_stops(dev, LB, name, xdrop):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, alphabet, S, g, h, w, band_ref = XD.stop_case(name)
    score, end, D, dropped = XD.STOPS[name][3][xdrop]
    ref = XD.xdrop_reference(A, B, alphabet, S, g, h, w, xdrop, band_ref=band_ref)
    # (the reference itself stops where the prototype did: a case that no longer exercises the stop fails here)
    assert (ref["score"], ref["end"], ref["diagonals"], ref["dropped"]) == (score, end, D, dropped)
    got, = _run(LB, dev, [(A, B)], alphabet, S, g, h, w, xdrop)
    _check(LB, got, ref)
    r = api.extend_align(A, B, **_api_kw(alphabet, S, g, h, w, xdrop))
    assert r == _want(ref)
    assert r["dropped"] == dropped and (r["global_score"] is None) == dropped


# ---- 5. the exact threshold ------------------------------------------------------------------------------------------
def test_exact_threshold(dev, LB):
    A, B, alphabet, S, g, h, w, band_ref = XD.stop_case("islands_w32")
    first = XD.xdrop_reference(A, B, alphabet, S, g, h, w, 10, band_ref=band_ref)
    d_star, delta = first["diagonals"], first["delta"]
    assert first["dropped"] and delta > 10
    refs = [XD.xdrop_reference(A, B, alphabet, S, g, h, w, x, band_ref=band_ref) for x in (delta - 1, delta)]
    assert refs[0]["diagonals"] == d_star and refs[1]["diagonals"] > d_star   # > xdrop stops, == xdrop goes on
    for x, ref in zip((delta - 1, delta), refs):
        got, = _run(LB, dev, [(A, B)], alphabet, S, g, h, w, x)
        _check(LB, got, ref)
        assert got["res"][3] == ref["diagonals"]


# ---- 6. a tie that row-major order and visit order decide differently ------------------------------------------------
def test_row_major_tie(dev, LB):
    A, B, alphabet, S, g, h, w, xdrop, c1, c2 = XD.row_major_tie()
    ref = XD.xdrop_reference(A, B, alphabet, S, g, h, w, xdrop)
    H = ref["H"]
    assert ref["end"] == c1 and H[c1[0], c1[1] - c1[0] + w] == H[c2[0], c2[1] - c2[0] + w] == ref["score"] > 0
    assert c1[0] < c2[0] and sum(c1) > sum(c2) and sum(c1) <= ref["diagonals"]   # the later anti-diagonal wins
    got, = _run(LB, dev, [(A, B)], alphabet, S, g, h, w, xdrop)
    _check(LB, got, ref)
    assert tuple(got["res"][1:3]) == c1


# ---- 7. batches ------------------------------------------------------------------------------------------------------
def _batch_pairs(k):
    rng = np.random.default_rng(412)
    same = XB.rs(rng, 77)
    five = [ER._prefix(7, 40, 300, 300),      # dropped early
            (same, same),                     # never dropped
            ER._prefix(307, 100, 400, 150),   # clipped (and dropped)
            (b"A" * 64, b"C" * 70),           # the empty extension
            (b"G", b"G")]                     # 1 x 1
    more = [XB.similar(np.random.default_rng(413), 120), ER._prefix(8, 3, 90, 70), (b"T", b"TACG" * 5),
            (same[:50] + b"A" * 30, same[:50] + b"C" * 45)]
    return (five + more)[:k]


@pytest.mark.parametrize("k", [5, 9])
def test_batch(dev, LB, k):
    from cse305_parallel_sequence_alignment_amd import api

    alphabet, S, g, h = XB.score_set("dna")
    w, xdrop = 16, 10
    pairs = _batch_pairs(k)
    refs = [XD.xdrop_reference(a, b, alphabet, S, g, h, w, xdrop) for a, b in pairs]
    assert [r["dropped"] for r in refs[:5]] == [True, False, True, True, False]
    assert (refs[2]["m_eff"], refs[2]["n_eff"]) == (166, 150) and refs[3]["score"] == 0
    for got, ref in zip(_run(LB, dev, pairs, alphabet, S, g, h, w, xdrop), refs):
        _check(LB, got, ref)
    kw = _api_kw(alphabet, S, g, h, w, xdrop)
    assert api.extend_align_batch([a for a, _ in pairs], [b for _, b in pairs], **kw) == [_want(r) for r in refs]
    assert api.extend_align_batch([a for a, _ in pairs], [b for _, b in pairs], traceback=False, **kw) == \
        [_want(r, False) for r in refs]


def test_batch_shared_b(dev):
    """Many queries against one B, uploaded once (each query clips it to its own length + band)."""
    from cse305_parallel_sequence_alignment_amd import api

    alphabet, S, g, h = XB.score_set("dna")
    w, xdrop = 32, 12
    As, ref_b = XB.shared_b_batch()
    As = As + [ref_b]   # (B against itself: never dropped)
    want = [_want(XD.xdrop_reference(a, ref_b, alphabet, S, g, h, w, xdrop)) for a in As]
    assert any(x["dropped"] for x in want) and not all(x["dropped"] for x in want)
    assert api.extend_align_batch(As * 7, ref_b, **_api_kw(alphabet, S, g, h, w, xdrop)) == want * 7


# ---- 8. 24 symbols: 5-bit codes through the same table ---------------------------------------------------------------
@pytest.mark.parametrize("xdrop", [-1, 5, 8])
def test_wide_alphabet(dev, LB, xdrop):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, alphabet, S, g, h = ER.protein32()
    w = 16
    assert len(alphabet) == 24
    ref = XD.xdrop_reference(A, B, alphabet, S, g, h, w, xdrop)
    assert ref["dropped"] == (xdrop >= 0)
    got, = _run(LB, dev, [(A, B)], alphabet, S, g, h, w, xdrop)
    _check(LB, got, ref)
    kw = _api_kw(alphabet, S, g, h, w, xdrop)
    assert kw["max_symbols"] == 32
    assert api.extend_align(A, B, **kw) == _want(ref)
    cases = [ER.protein32(k) for k in range(3)]
    refs = [XD.xdrop_reference(c[0], c[1], alphabet, S, g, h, w, xdrop) for c in cases]
    assert api.extend_align_batch([c[0] for c in cases], [c[1] for c in cases], **kw) == [_want(r) for r in refs]


# ---- 9. the Python API -----------------------------------------------------------------------------------------------
def test_api(dev):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, alphabet, S, g, h, w, band_ref = XD.stop_case("islands_w32")
    DNA_KW = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2)
    for xdrop in (10, 30, 60, -1):
        ref = XD.xdrop_reference(A, B, alphabet, S, g, h, w, xdrop, band_ref=band_ref)
        assert api.extend_align(A, B, band=w, xdrop=xdrop, **DNA_KW) == _want(ref)
        assert api.extend_align(A, B, band=w, xdrop=xdrop, traceback=False, **DNA_KW) == _want(ref, False)
    # termination changes the answer: the first island alone, or both
    assert api.extend_align(A, B, band=w, xdrop=10, **DNA_KW)["score"] == 124
    assert api.extend_align(A, B, band=w, xdrop=60, **DNA_KW)["score"] == 259
    # xdrop=None is today's banded call, key for key
    assert api.extend_align(A, B, band=w, xdrop=None, **DNA_KW) == api.extend_align(A, B, band=w, **DNA_KW)
    got = api.extend_align_batch([A, A[:70], B], [B, B, B], band=w, xdrop=10, **DNA_KW)
    assert got == [_want(XD.xdrop_reference(a, B, alphabet, S, g, h, w, 10)) for a in (A, A[:70], B)]
