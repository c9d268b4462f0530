"""Alignment over alphabets of up to 32 symbols (msa_plan_create_scored32: MSA_NW_SCORED and MSA_NW_FIT plans over
5-bit codes under a 32 x 32 table; msa_nw_align_scored32, msa_nw_align_batch_scored32, msa_fit_align32,
msa_fit_align_batch32; api.* with max_symbols=32) against the yardstick tests/wide_reference.py (the 8-code
yardsticks with the symbol lookup widened, checked against them and against a plain-Python Gotoh DP by
test_wide_alphabet_host.py).

Every fill case checks, exactly (integer DP): the score (fit: and end = (m, end_j)), the plan's error word, bits 0-1
of every in-band interior direction byte, bit 2 where E is finite and bit 3 where F is finite, the walk's ops byte
for byte, its stop cell, the CIGAR, and the ops rescored.  Inputs are seeded random sequences over all 32 codes under
wide_reference.table32 (dense, asymmetric: a swapped index or a wrong 8-code group changes scores) unless a test says
otherwise.  Shapes are the smallest at which each mechanism runs: more stripes than waves (the wrap link), more than
one item (the granule hand-off), a one-row pair, an exact-stripe pair, a band narrower and wider than a stripe."""
import ctypes as C
import functools

import numpy as np
import pytest

import nw_reference as R
import wide_reference as W

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG, CAPACITY = -5, -1, -8
S32, G, H = W.table32(), 1, 2   # the table, gap_extend, gap_open - gap_extend of most cases


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _dev(x, alphabet, dev):
    import torch

    return torch.from_numpy(W.codes32(x, alphabet).astype(np.uint8)).to(dev)


def _plan(LB, alg, ms, ns, a_offs, b_offs, S, g, h, band=-1, cells=None, single=None):
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    return Plan(alg, LB.CELLS_DIR if cells is None else cells, ms, ns, a_offs, b_offs, gap_open=g + h, gap_extend=g,
                band=band, single=single, sub=W.sub32(S))


def _fill(LB, dev, alg, A, B, alphabet, S, g, h, band=-1):
    import torch

    pl = _plan(LB, alg, [len(A)], [len(B)], [0], [0], S, g, h, band=band, single=True)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev), dDir)
    return pl, dDir


def _check_bytes(pl, dDir, ref, pair):
    got = R.to_band(pl.deskew_dir(dDir.cpu().numpy(), pair, pl.stripe_meta()), ref["w"])
    v, want = ref["valid"], ref["byte"]
    bad = v & ((got & 3) != (want & 3))
    assert not bad.any(), ("bits 0-1", int(bad.sum()), np.argwhere(bad)[:4])
    bad = v & ref["efin"] & ((got & 4) != (want & 4))
    assert not bad.any(), ("bit 2", int(bad.sum()), np.argwhere(bad)[:4])
    bad = v & ref["ffin"] & ((got & 8) != (want & 8))
    assert not bad.any(), ("bit 3", int(bad.sum()), np.argwhere(bad)[:4])


def _check(pl, dDir, A, B, band, alphabet, S, g, h, ref, pair=0):
    """Everything a global fill test checks for one pair (see the module docstring)."""
    res = pl.results()[pair]
    assert (res["score"], tuple(res["end"]), res["status"]) == (ref["score"], (len(A), len(B)), 0)
    assert pl.error() == 0
    assert pl.launch_info()["mode"] == "stripe" and pl.format_info()["codes"] == 32
    _check_bytes(pl, dDir, ref, pair)
    tb = pl.traceback_nw(dDir, pair)
    assert tb["ops"] == ref["ops"]
    assert tb["stop"] == ref["stop"]
    assert tb["cigar"] == W.cigar_of(ref["ops"])
    assert W.rescore32(A, B, tb["ops"], alphabet, S, g, h, band) == ref["score"]
    return tb


def _check_fit(pl, dDir, A, B, alphabet, S, g, h, ref, pair=0):
    """... a fit fill test."""
    res = pl.results()[pair]
    assert (res["score"], tuple(res["end"]), res["status"]) == (ref["score"], (len(A), ref["end_j"]), 0)
    assert pl.error() == 0
    assert pl.launch_info()["mode"] == "stripe" and pl.format_info()["codes"] == 32
    _check_bytes(pl, dDir, ref, pair)
    tb = pl.traceback_nw(dDir, pair)
    assert tb["ops"] == ref["ops"]
    assert tb["stop"] == ref["stop"] and tb["stop"][1] == ref["beg_j"]
    assert tb["cigar"] == W.cigar_of(ref["ops"])
    assert W.fit_rescore32(A, B, tb["stop"][1], res["end"][1], tb["ops"], alphabet, S, g, h) == ref["score"]
    return tb


def _offsets(seqs):
    return np.concatenate(([0], np.cumsum([len(s) for s in seqs])[:-1]))


# ---- 1. every cell of one pair ---------------------------------------------------------------------------------
def test_single_pair_every_cell(dev, LB):
    """330 x 300: six stripes in two items of four waves (the wrap of the link rings, the granule hand-off)."""
    rng = np.random.default_rng(51)
    A, B = W.rs32(rng, 330), W.rs32(rng, 300)
    a, b = W.codes32(A, W.AL32), W.codes32(B, W.AL32)
    assert np.unique(32 * a[:, None] + b[None, :]).size == 1024  # every (row code, column code) pair is a cell
    ref = W.nw_reference32(A, B, W.AL32, S32, G, H)
    pl, dDir = _fill(LB, dev, LB.NW_SCORED, A, B, W.AL32, S32, G, H)
    assert pl.single and pl.launch_info()["items"] == 2
    _check(pl, dDir, A, B, -1, W.AL32, S32, G, H, ref)
    Hm, Em, Fm = W.gotoh_brute(A, B, W.AL32, S32, G, H)
    assert tuple(pl.results()[0]["fin"]) == (Hm[330][300], Em[330][300], Fm[330][300])


# ---- 2. a batch plan -------------------------------------------------------------------------------------------
BATCH = [(600, 150), (77, 90), (1, 40), (64, 64)]  # ten stripes > eight waves; a one-row pair; an exact stripe


@functools.lru_cache(maxsize=None)
def _batch_case():
    rng = np.random.default_rng(52)
    pairs = [(W.rs32(rng, m), W.rs32(rng, n)) for m, n in BATCH]
    return pairs, [W.nw_reference32(a, b, W.AL32, S32, G, H) for a, b in pairs]


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_batch_plan(dev, LB, cells):
    import torch

    pairs, refs = _batch_case()
    As, Bs = [a for a, _ in pairs], [b for _, b in pairs]
    ms, ns = [len(a) for a in As], [len(b) for b in Bs]
    dA, dB = _dev(b"".join(As), W.AL32, dev), _dev(b"".join(Bs), W.AL32, dev)
    if cells == "none":
        pl = _plan(LB, LB.NW_SCORED, ms, ns, _offsets(As), _offsets(Bs), S32, G, H, cells=LB.CELLS_NONE)
        assert pl.cells_elems == 0 and not pl.single
        pl.run(dA, dB)
        assert [r["score"] for r in pl.results()] == [ref["score"] for ref in refs]
        assert pl.error() == 0 and pl.launch_info()["mode"] == "stripe" and pl.format_info()["codes"] == 32
        return
    pl = _plan(LB, LB.NW_SCORED, ms, ns, _offsets(As), _offsets(Bs), S32, G, H)
    assert not pl.single
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(dA, dB, dDir)
    singles = [_check(pl, dDir, a, b, -1, W.AL32, S32, G, H, ref, pair=k) for k, ((a, b), ref) in
               enumerate(zip(pairs, refs))]
    for one, tb, ref in zip(singles, pl.traceback_batch(dDir), refs):
        assert (tb["ops"], tb["stop"], tb["cigar"]) == (one["ops"], one["stop"], W.cigar_of(ref["ops"]))


# ---- 3. a banded single pair: the exact masked stripe launch ---------------------------------------------------
# (400 x 400 with band 64 has stripes a whole stripe away from the matrix borders: the v_writelane edge fix-ups)
@pytest.mark.parametrize("m,n,band", [(65, 70, 8), (193, 193, 64), (700, 700, 1), (400, 400, 64)])
def test_banded_single_pair(dev, LB, m, n, band):
    rng = np.random.default_rng(53 + m)
    A = W.rs32(rng, m)
    B = (W.mutated(rng, A, W.AL32, 0.1) + W.rs32(rng, max(0, n - m)))[:n]  # (near the diagonal: in-band paths matter)
    ref = W.nw_reference32(A, B, W.AL32, S32, G, H, band)
    pl, dDir = _fill(LB, dev, LB.NW_SCORED, A, B, W.AL32, S32, G, H, band=band)
    _check(pl, dDir, A, B, band, W.AL32, S32, G, H, ref)


# ---- 4. fit ----------------------------------------------------------------------------------------------------
P20, GF, HF = W.protein20(), 1, 10  # a protein-shaped symmetric table, gap_open 11, gap_extend 1


@functools.lru_cache(maxsize=None)
def _fit_case():
    """A 700-symbol reference over 20 symbols; queries: a mutated copy of ref[333:433], a mutated ref[600:700] (the
    maximum at column n), and 15 random symbols in front of ref[0:85] (it overhangs the reference's start)."""
    rng = np.random.default_rng(54)
    ref = W.rs32(rng, 700, W.AL20)
    qs = [W.mutated(rng, ref[333:433], W.AL20), W.mutated(rng, ref[600:700], W.AL20),
          W.rs32(rng, 15, W.AL20) + ref[0:85]]
    return qs, ref, [W.fit_reference32(q, ref, W.AL20, P20, GF, HF) for q in qs]


def test_fit_single_pair(dev, LB):
    qs, ref, want = _fit_case()
    assert int(np.abs(P20).max()) <= 11 and int(P20.min()) == -4 and (P20 == P20.T).all()
    pl, dDir = _fill(LB, dev, LB.NW_FIT, qs[0], ref, W.AL20, P20, GF, HF)
    tb = _check_fit(pl, dDir, qs[0], ref, W.AL20, P20, GF, HF, want[0])
    assert (tb["stop"][1], want[0]["end_j"]) == (333, 433)  # the planted copy


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_fit_batch_shared_reference(dev, LB, cells):
    import torch

    qs, ref, want = _fit_case()
    ms, ns = [len(q) for q in qs], [len(ref)] * 3
    dA, dB = _dev(b"".join(qs), W.AL20, dev), _dev(ref, W.AL20, dev)
    assert want[2]["stop"][0] > 0 and want[2]["ops"].endswith(b"I")  # the overhang
    if cells == "none":
        pl = _plan(LB, LB.NW_FIT, ms, ns, _offsets(qs), [0, 0, 0], P20, GF, HF, cells=LB.CELLS_NONE)
        pl.run(dA, dB)
        assert [(r["score"], tuple(r["end"])) for r in pl.results()] == \
            [(w["score"], (m, w["end_j"])) for w, m in zip(want, ms)]
        assert pl.error() == 0 and pl.launch_info()["mode"] == "stripe" and pl.format_info()["codes"] == 32
        return
    pl = _plan(LB, LB.NW_FIT, ms, ns, _offsets(qs), [0, 0, 0], P20, GF, HF)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(dA, dB, dDir)
    singles = [_check_fit(pl, dDir, q, ref, W.AL20, P20, GF, HF, w, pair=k) for k, (q, w) in enumerate(zip(qs, want))]
    for one, tb, w in zip(singles, pl.traceback_batch(dDir), want):
        assert (tb["ops"], tb["stop"], tb["cigar"]) == (one["ops"], one["stop"], W.cigar_of(w["ops"]))


# ---- 5. the extreme bytes at codes >= 8 ------------------------------------------------------------------------
def test_extreme_bytes(dev, LB):
    """127 at S[9][17] and -128 at S[31][31] on a 40 x 40 pair whose cells use both (sign extension through the
    three permutes); inside check_ranges' bound: (128 + 2 * 3 + 2 * 1) * (80 + 256) + 2 < 2^28."""
    S = S32.copy()
    S[9, 17], S[31, 31] = 127, -128
    rng = np.random.default_rng(55)
    a, b = bytearray(W.rs32(rng, 40)), bytearray(W.rs32(rng, 40))
    a[10], b[10] = W.AL32[9], W.AL32[17]      # +127 on the main diagonal
    a[25], b[25] = W.AL32[31], W.AL32[31]     # -128 on it
    A, B = bytes(a), bytes(b)
    ref = W.nw_reference32(A, B, W.AL32, S, G, H)
    plain = W.nw_reference32(A, B, W.AL32, S32, G, H)
    assert ref["score"] != plain["score"] and (ref["byte"] != plain["byte"]).any()  # (the two entries decide)
    pl, dDir = _fill(LB, dev, LB.NW_SCORED, A, B, W.AL32, S, G, H)
    _check(pl, dDir, A, B, -1, W.AL32, S, G, H, ref)


# ---- 6. the host entries and api -------------------------------------------------------------------------------
def _p(x):
    return x.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _global20():
    """Two 20-symbol pairs (a mutated copy, lengths 150 / 150 and 90 / 97) with the yardstick's answers."""
    rng = np.random.default_rng(56)
    out = []
    for m, extra in ((150, 0), (90, 7)):
        a = W.rs32(rng, m, W.AL20)
        out.append((a, W.mutated(rng, a, W.AL20) + W.rs32(rng, extra, W.AL20)))
    return out, [W.nw_reference32(a, b, W.AL20, P20, GF, HF) for a, b in out]


def test_entries_global(dev, LB):
    from cse305_parallel_sequence_alignment_amd import api

    pairs, refs = _global20()
    sub = np.ascontiguousarray(P20, dtype=np.int8)
    (A, B), ref = pairs[0], refs[0]
    cigar = W.cigar_of(ref["ops"])
    sc = C.c_int32()
    cig = C.create_string_buffer(len(cigar) + 1)
    f = LB.lib().msa_nw_align_scored32
    args = (A, len(A), B, len(B), W.AL20, 20, _p(sub), GF + HF, GF, -1, C.byref(sc), cig)
    assert f(*args, len(cigar)) == CAPACITY  # (no room for the NUL)
    assert f(*args, len(cigar) + 1) == 0
    assert (sc.value, cig.value.decode()) == (ref["score"], cigar)
    assert W.rescore32(A, B, ref["ops"], W.AL20, P20, GF, HF) == ref["score"]
    kw = dict(gap_open=GF + HF, gap_extend=GF, alphabet=W.AL20, matrix=P20, max_symbols=32)
    assert api.nw_align(A, B, **kw) == dict(score=ref["score"], cigar=cigar)
    assert api.nw_align(A, B, traceback=False, **kw) == dict(score=ref["score"])
    # the batch entry: CAPACITY with the needed size, then that size
    As, Bs = [a for a, _ in pairs], [b for _, b in pairs]
    m, n = np.array([len(a) for a in As], dtype=np.int64), np.array([len(b) for b in Bs], dtype=np.int64)
    a_off, b_off = _offsets(As).astype(np.int64), _offsets(Bs).astype(np.int64)
    cigars = [W.cigar_of(r["ops"]) for r in refs]
    need = sum(len(c) + 1 for c in cigars)

    def batch(cap):
        scs, coff, buf = np.zeros(2, dtype=np.int32), np.zeros(3, dtype=np.int64), C.create_string_buffer(max(cap, 1))
        rc = LB.lib().msa_nw_align_batch_scored32(b"".join(As), int(m.sum()), b"".join(Bs), int(n.sum()), 2, _p(a_off),
                                                  _p(m), _p(b_off), _p(n), W.AL20, 20, _p(sub), GF + HF, GF, -1,
                                                  _p(scs), buf, cap, _p(coff))
        return rc, scs, coff, buf

    rc, _, coff, _ = batch(need - 1)
    assert rc == CAPACITY and int(coff[2]) == need
    rc, scs, coff, buf = batch(need)
    assert rc == 0 and scs.tolist() == [r["score"] for r in refs]
    assert [buf.raw[coff[q]:coff[q + 1] - 1].decode() for q in range(2)] == cigars
    assert api.nw_align_batch(As, Bs, **kw) == [dict(score=r["score"], cigar=c) for r, c in zip(refs, cigars)]
    # match / mismatch over the sequences' own (more than 8) symbols
    assert len(set(A + B)) > 8
    alpha = bytes(dict.fromkeys(A + B))
    want = W.nw_reference32(A, B, alpha, np.where(np.eye(len(alpha), dtype=bool), 3, -2), 1, 2)
    got = api.nw_align(A, B, match=3, mismatch=-2, max_symbols=32)
    assert got == dict(score=want["score"], cigar=W.cigar_of(want["ops"]))


def test_entries_fit(dev, LB):
    from cse305_parallel_sequence_alignment_amd import api

    qs, ref, want = _fit_case()
    sub = np.ascontiguousarray(P20, dtype=np.int8)
    cigars = [W.cigar_of(w["ops"]) for w in want]
    sc, bj, ej = C.c_int32(), C.c_int64(), C.c_int64()
    cig = C.create_string_buffer(len(cigars[2]) + 1)
    f = LB.lib().msa_fit_align32
    args = (qs[2], len(qs[2]), ref, len(ref), W.AL20, 20, _p(sub), GF + HF, GF, C.byref(sc), C.byref(bj), C.byref(ej),
            cig)
    assert f(*args, len(cigars[2])) == CAPACITY
    assert f(*args, len(cigars[2]) + 1) == 0
    assert (sc.value, bj.value, ej.value, cig.value.decode()) == \
        (want[2]["score"], want[2]["beg_j"], want[2]["end_j"], cigars[2])
    kw = dict(gap_open=GF + HF, gap_extend=GF, alphabet=W.AL20, matrix=P20, max_symbols=32)
    dicts = [dict(score=w["score"], beg=w["beg_j"], end=w["end_j"], cigar=c) for w, c in zip(want, cigars)]
    assert api.fit_align(qs[0], ref, **kw) == dicts[0]
    assert api.fit_align_batch(qs, ref, **kw) == dicts
    assert api.fit_align_batch(qs, ref, traceback=False, **kw) == \
        [dict(score=w["score"], beg=None, end=w["end_j"]) for w in want]
    # the batch entry's CAPACITY carries the needed size
    k = len(qs)
    m, n = np.array([len(q) for q in qs], dtype=np.int64), np.full(k, len(ref), dtype=np.int64)
    a_off, b_off = _offsets(qs).astype(np.int64), np.zeros(k, dtype=np.int64)
    need = sum(len(c) + 1 for c in cigars)
    scs, be, coff = np.zeros(k, dtype=np.int32), np.zeros((k, 2), dtype=np.int64), np.zeros(k + 1, dtype=np.int64)
    buf = C.create_string_buffer(need)
    g = LB.lib().msa_fit_align_batch32
    bargs = (b"".join(qs), int(m.sum()), ref, len(ref), k, _p(a_off), _p(m), _p(b_off), _p(n), W.AL20, 20, _p(sub),
             GF + HF, GF, _p(scs), _p(be), buf)
    assert g(*bargs, need - 1, _p(coff)) == CAPACITY and int(coff[k]) == need
    assert g(*bargs, need, _p(coff)) == 0
    assert [buf.raw[coff[q]:coff[q + 1] - 1].decode() for q in range(k)] == cigars
    assert be.tolist() == [[w["beg_j"], w["end_j"]] for w in want] and scs.tolist() == [w["score"] for w in want]


def test_four_symbols_through_either_entry(dev):
    """Up to 8 symbols a *32 entry builds its twin's plans: identical results."""
    from cse305_parallel_sequence_alignment_amd import api
    import nw_scored_reference as RS

    alphabet, S, g, h = RS.SCORE_SETS["asym"]
    rng = np.random.default_rng(57)
    A, B = R.rs(rng, 200), R.rs(rng, 190)
    kw = dict(gap_open=g + h, gap_extend=g, alphabet=alphabet, matrix=S)
    ref = RS.nw_scored_reference(A, B, alphabet, S, g, h, 16)
    want = dict(score=ref["score"], cigar=R.cigar_of(ref["ops"]))
    assert api.nw_align(A, B, band=16, **kw) == api.nw_align(A, B, band=16, max_symbols=32, **kw) == want
    assert api.nw_align_batch([A, B], [B, A], **kw) == api.nw_align_batch([A, B], [B, A], max_symbols=32, **kw)
    assert api.fit_align(A[:50], B, **kw) == api.fit_align(A[:50], B, max_symbols=32, **kw)
    assert api.fit_align_batch([A[:50], A[60:90]], B, **kw) == \
        api.fit_align_batch([A[:50], A[60:90]], B, max_symbols=32, **kw)


# ---- 7. rejections ---------------------------------------------------------------------------------------------
def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_plan_creation_errors(dev, LB):
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    mk = lambda alg, **kw: _plan(LB, alg, [100], [100], [0], [0], S32, G, H, **kw)  # noqa: E731
    for alg in (LB.SW_AFFINE, LB.NW_ALIGN, LB.REF_GOTOH, LB.SW_LINEAR, LB.NW_BANDED):
        assert _status(lambda: mk(alg)) == UNSUPPORTED
    assert _status(lambda: mk(LB.NW_SCORED, cells=LB.CELLS_H)) == UNSUPPORTED
    assert _status(lambda: mk(LB.NW_FIT, cells=LB.CELLS_TAB)) == UNSUPPORTED
    for band in (0, 64):
        assert _status(lambda: mk(LB.NW_FIT, band=band)) == UNSUPPORTED
    assert _status(lambda: mk(LB.NW_SCORED, band=64)) == 0 and _status(lambda: mk(LB.NW_FIT)) == 0
    # a NULL table
    arrs = [(C.c_int64 * 1)(v) for v in (100, 100, 0, 0)]
    d = LB.PlanDesc(alg=LB.NW_SCORED, cells=LB.CELLS_DIR, match=1, mismatch=0, gap_open=3, gap_extend=1, start_type=-1,
                    band=-1, track_end=0, single=1, n_pairs=1, m=arrs[0], n=arrs[1], a_off=arrs[2], b_off=arrs[3])
    h = C.c_void_p()
    assert LB.lib().msa_plan_create_scored32(C.byref(d), None, C.byref(h)) == ARG
    with pytest.raises(ValueError):
        Plan(LB.NW_SCORED, LB.CELLS_DIR, [100], [100], [0], [0], sub=np.zeros((16, 16), dtype=np.int8))
    # an 8 x 8 table still makes an 8-code plan
    eight = Plan(LB.NW_SCORED, LB.CELLS_DIR, [100], [100], [0], [0], gap_open=3, gap_extend=1,
                 sub=np.zeros((8, 8), dtype=np.int8))
    assert eight.format_info()["codes"] == 8


def test_value_range_bound(dev, LB):
    """check_ranges' inequality (s + 2 G + 2 g)(m + n + 256) + (G - g) < 2^28 with s over the 1,024 scores: the
    largest gap_open inside it (gap_extend 0) runs and matches the yardstick, the next one is MSA_ERR_UNSUPPORTED."""
    rng = np.random.default_rng(58)
    A = W.rs32(rng, 40)
    B = W.mutated(rng, A, W.AL32) + W.rs32(rng, 4)
    s, T = int(np.abs(S32).max()), 40 + 44 + 256
    Gin = ((1 << 28) - 1 - s * T) // (2 * T + 1)
    assert (s + 2 * Gin) * T + Gin < (1 << 28) <= (s + 2 * (Gin + 1)) * T + Gin + 1
    assert _status(lambda: _plan(LB, LB.NW_SCORED, [40], [44], [0], [0], S32, 0, Gin + 1)) == UNSUPPORTED
    # (the largest score alone decides s: the same gap costs are inside the bound under a smaller table)
    assert _status(lambda: _plan(LB, LB.NW_SCORED, [40], [44], [0], [0], S32 // 2, 0, Gin + 1)) == 0
    ref = W.nw_reference32(A, B, W.AL32, S32, 0, Gin)
    pl, dDir = _fill(LB, dev, LB.NW_SCORED, A, B, W.AL32, S32, 0, Gin)
    _check(pl, dDir, A, B, -1, W.AL32, S32, 0, Gin, ref)


def test_other_walkers_reject_the_plan(dev, LB):
    import torch

    pairs, refs = _batch_case()
    A, B = pairs[1]
    pl, dDir = _fill(LB, dev, LB.NW_SCORED, A, B, W.AL32, S32, G, H)
    ops = torch.empty(len(A) + len(B) + 2, dtype=torch.uint8, device=dev)
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    assert _status(lambda: pl.traceback_async(dDir, ops, info)) == UNSUPPORTED
    assert _status(lambda: pl.traceback_gotoh_async(dDir, ops, info)) == UNSUPPORTED
    none = _plan(LB, LB.NW_SCORED, [len(A)], [len(B)], [0], [0], S32, G, H, cells=LB.CELLS_NONE)
    assert _status(lambda: none.traceback_nw_async(dDir, ops, info)) == UNSUPPORTED
