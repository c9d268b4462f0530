"""Global alignment under match / mismatch scores or an 8 x 8 matrix (MSA_NW_SCORED, msa_plan_create_scored,
msa_nw_align_scored, msa_nw_align_batch_scored) against the numpy yardstick tests/nw_scored_reference.py (itself
checked against a triple-loop Gotoh, nw_reference and the Levenshtein distance by test_nw_scored_reference.py).

Every fill case runs test_gpu_nw_align.py::_check's checks with the yardstick in place of the oracle's score: the
score, the plan's error word, bits 0-1 of every in-band interior direction byte, bit 2 where E is finite and bit 3
where F is finite, the walk's ops byte for byte, its stop cell, the CIGAR, and the ops rescored.  Integer DP: every
comparison is exact.  Shapes are nw_reference's (the smallest at which each launch mechanism can fail).

Observed on MI355X: `converged` of the chunked cases (test_band_chunked) is 1 on similar_9001_w64 and 0 on
random_12000_w512 under both "dna" and "neg" -- what the +1 / 0 twins report on the same inputs."""
import ctypes as C
import functools

import numpy as np
import pytest

import nw_reference as R
import nw_scored_reference as RS

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG, ALPHABET = -5, -1, -2
IDENT = RS.match_mismatch(b"ACGT", 1, 0)


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _dev(x, alphabet, dev):
    import torch

    return torch.from_numpy(RS.codes(x, alphabet).astype(np.uint8)).to(dev)


@functools.lru_cache(maxsize=None)
def _case(name, set_name):
    """(A, B, band, alphabet, S, g, h, reference) of a named shape under a score set, computed once and shared
    (never modified).  Shapes: nw_reference's SMALL and CHUNKED tables; the gap costs are the score set's."""
    A, B, band = (R.SMALL[name]() if name in R.SMALL else R.chunked_case(name))[:3]
    alphabet, S, g, h = RS.SCORE_SETS[set_name]
    A, B = RS.set_input(set_name, A, B)
    return A, B, band, alphabet, S, g, h, RS.nw_scored_reference(A, B, alphabet, S, g, h, band)


def _plan(LB, ms, ns, a_offs, b_offs, band, S, g, h, cells=None, how="sub"):
    """An NW_SCORED plan; how = "sub": the 8 x 8 table, "mm": S's match / mismatch through the description."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    kw = dict(sub=RS.sub8(S)) if how == "sub" else dict(match=int(S[0][0]), mismatch=int(S[0][1]))
    return Plan(LB.NW_SCORED, LB.CELLS_DIR if cells is None else cells, ms, ns, a_offs, b_offs, gap_open=g + h,
                gap_extend=g, band=band, **kw)


def _fill(LB, dev, A, B, band, alphabet, S, g, h, how="sub"):
    import torch

    pl = _plan(LB, [len(A)], [len(B)], [0], [0], band, S, g, h, how=how)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev), dDir)
    return pl, dDir


def _check(pl, dDir, A, B, band, alphabet, S, g, h, ref, pair=0):
    """Everything a fill test checks for one pair (see the module docstring)."""
    w = ref["w"]
    assert pl.results()[pair]["score"] == ref["score"]
    assert pl.error() == 0
    got = R.to_band(pl.deskew_dir(dDir.cpu().numpy(), pair, pl.stripe_meta()), w)
    v, want = ref["valid"], ref["byte"]
    bad = v & ((got & 3) != (want & 3))
    assert not bad.any(), ("bits 0-1", int(bad.sum()), np.argwhere(bad)[:4])
    bad = v & ref["efin"] & ((got & 4) != (want & 4))
    assert not bad.any(), ("bit 2", int(bad.sum()), np.argwhere(bad)[:4])
    bad = v & ref["ffin"] & ((got & 8) != (want & 8))
    assert not bad.any(), ("bit 3", int(bad.sum()), np.argwhere(bad)[:4])
    tb = pl.traceback_nw(dDir, pair)
    assert tb["ops"] == ref["ops"]
    assert tb["stop"] == ref["stop"]
    assert tb["cigar"] == R.cigar_of(ref["ops"])
    assert RS.rescore(A, B, tb["ops"], alphabet, S, g, h, band) == ref["score"]
    return tb


def _offsets(pairs):
    a_offs = np.concatenate(([0], np.cumsum([len(a) for a, _ in pairs])[:-1]))
    b_offs = np.concatenate(([0], np.cumsum([len(b) for _, b in pairs])[:-1]))
    return a_offs, b_offs


def _batch_fill(LB, dev, pairs, band, alphabet, S, g, h, how="sub"):
    import torch

    a_offs, b_offs = _offsets(pairs)
    pl = _plan(LB, [len(a) for a, _ in pairs], [len(b) for _, b in pairs], a_offs, b_offs, band, S, g, h, how=how)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev(b"".join(a for a, _ in pairs), alphabet, dev), _dev(b"".join(b for _, b in pairs), alphabet, dev),
           dDir)
    return pl, dDir


def _check_batch(pl, dDir, pairs, band, alphabet, S, g, h):
    """Every pair's checks, and the one-launch batch walk against the per-pair walks."""
    singles = [_check(pl, dDir, A, B, band, alphabet, S, g, h, RS.nw_scored_reference(A, B, alphabet, S, g, h, band),
                      pair=k) for k, (A, B) in enumerate(pairs)]
    for one, tb in zip(singles, pl.traceback_batch(dDir)):
        assert (tb["ops"], tb["stop"], tb["cigar"]) == (one["ops"], one["stop"], one["cigar"])


# ---- 1. identity anchor: S = 1 / 0 is NW_ALIGN ------------------------------------------------------------
@pytest.mark.parametrize("how", ["mm", "sub"])
@pytest.mark.parametrize("name", ["random_1000x1030_w64", "random_500x480_noband"] + list(R.CHUNKED))
def test_identity_single(dev, LB, name, how):
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    A, B, band, g, h = R.SMALL[name]() if name in R.SMALL else R.chunked_case(name)
    ref = _identity_ref(name)
    pl, dDir = _fill(LB, dev, A, B, band, b"ACGT", IDENT, g, h, how=how)
    twin = Plan(LB.NW_ALIGN, LB.CELLS_DIR, [len(A)], [len(B)], [0], [0], match=1, mismatch=0, gap_open=g + h,
                gap_extend=g, band=band)
    assert pl.launch_info()["mode"] == twin.launch_info()["mode"]
    _check(pl, dDir, A, B, band, b"ACGT", IDENT, g, h, ref)
    if name in R.CHUNKED:
        tDir = torch.zeros(twin.cells_elems, dtype=torch.uint8, device=dev)
        twin.run(_dev(A, b"ACGT", dev), _dev(B, b"ACGT", dev), tDir)
        twin.results()
        assert pl.launch_info()["mode"] == "band_chunked"
        assert pl.run_info()["converged"] == twin.run_info()["converged"]


@functools.lru_cache(maxsize=None)
def _identity_ref(name):
    A, B, band, g, h = R.SMALL[name]() if name in R.SMALL else R.chunked_case(name)
    return R.nw_reference(A, B, g, h, band)


@pytest.mark.parametrize("how", ["mm", "sub"])
def test_identity_batch(dev, LB, how):
    pairs, band = R.batch_pairs(), 64
    pl, dDir = _batch_fill(LB, dev, pairs, band, b"ACGT", IDENT, 1, 2, how=how)
    twin = _twin_batch(LB, pairs, band)
    assert pl.launch_info()["mode"] == twin.launch_info()["mode"] == "stripe"
    for k, (A, B) in enumerate(pairs):
        _check(pl, dDir, A, B, band, b"ACGT", IDENT, 1, 2, R.nw_reference(A, B, 1, 2, band), pair=k)


def _twin_batch(LB, pairs, band):
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    a_offs, b_offs = _offsets(pairs)
    return Plan(LB.NW_ALIGN, LB.CELLS_DIR, [len(a) for a, _ in pairs], [len(b) for _, b in pairs], a_offs, b_offs,
                match=1, mismatch=0, gap_open=3, gap_extend=1, band=band)


# ---- 2. band_kernel, the exact chain -------------------------------------------------------------------------
BAND_DNA = ["random_1000x1030_w64", "random_65x70_w8", "random_193x193_w64", "random_700x700_w1",
            "ties_A400_A390_w16", "ties_A300_C300_w16", "border_25I_w40", "border_25D_w40"]


@pytest.mark.parametrize("name,set_name", [(n, "dna") for n in BAND_DNA] +
                         [("random_300x290_w32", s) for s in RS.SCORE_SETS])
def test_band_exact(dev, LB, name, set_name):
    A, B, band, alphabet, S, g, h, ref = _case(name, set_name)
    pl, dDir = _fill(LB, dev, A, B, band, alphabet, S, g, h)
    assert pl.launch_info()["mode"] == "band"
    assert pl.run_info()["mode"] == "stripe"  # (not chunked)
    _check(pl, dDir, A, B, band, alphabet, S, g, h, ref)


# ---- 3. band_kernel, chunked ---------------------------------------------------------------------------------
@pytest.mark.parametrize("set_name", ["dna", "neg"])
@pytest.mark.parametrize("name", list(R.CHUNKED))
def test_band_chunked(dev, LB, name, set_name):
    """Correct whatever `converged` says: where a chunk does not converge the exact launch behind the chunks
    writes the bytes."""
    A, B, band, alphabet, S, g, h, ref = _case(name, set_name)
    pl, dDir = _fill(LB, dev, A, B, band, alphabet, S, g, h)
    pl.results()
    info = pl.run_info()
    print(f"{name} {set_name}: converged = {info['converged']}, chunks = {info['chunks']}")
    assert pl.launch_info()["mode"] == "band_chunked"
    assert info["mode"] == "chunked" and info["chunks"] >= 4 and info["int16_cells"] == 0, info
    assert pl.format_info()["int16_cells"] == 0
    _check(pl, dDir, A, B, band, alphabet, S, g, h, ref)


# ---- 4. stripe_kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_name", ["dna", "asym"])
@pytest.mark.parametrize("name", R.NOBAND)
def test_stripe_single_unbanded(dev, LB, name, set_name):
    A, B, band, alphabet, S, g, h, ref = _case(name, set_name)
    pl, dDir = _fill(LB, dev, A, B, band, alphabet, S, g, h)
    assert pl.launch_info()["mode"] == "stripe"
    _check(pl, dDir, A, B, band, alphabet, S, g, h, ref)


@pytest.mark.parametrize("band", [64, -1])
def test_stripe_batch(dev, LB, band):
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = R.batch_pairs()
    pl, dDir = _batch_fill(LB, dev, pairs, band, alphabet, S, g, h)
    assert pl.launch_info()["mode"] == "stripe"
    _check_batch(pl, dDir, pairs, band, alphabet, S, g, h)


def test_stripe_batch_band_away_from_borders(dev, LB):
    """Five codes, and stripes whose band edges the stripe kernel fixes up with lane writes."""
    alphabet, S, g, h = RS.SCORE_SETS["titv"]
    pairs = [RS.set_input("titv", A, B) for A, B in R.batch_wide_pairs()]
    assert any(b"N" in A and b"N" in B for A, B in pairs)
    band = R.BATCH_WIDE_BAND
    pl, dDir = _batch_fill(LB, dev, pairs, band, alphabet, S, g, h)
    assert pl.launch_info()["mode"] == "stripe"
    _check_batch(pl, dDir, pairs, band, alphabet, S, g, h)


# ---- 5. score only -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random_1000x1030_w64", "random_500x480_noband"])
def test_score_only(dev, LB, name):
    A, B, band, alphabet, S, g, h, ref = _case(name, "dna")
    pl = _plan(LB, [len(A)], [len(B)], [0], [0], band, S, g, h, cells=LB.CELLS_NONE)
    assert pl.cells_elems == 0
    assert pl.launch_info()["mode"] == ("band" if band >= 0 else "stripe")
    pl.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev))
    assert pl.results()[0]["score"] == ref["score"]
    assert pl.error() == 0


# ---- 6. admission and rejection ------------------------------------------------------------------------------
def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_rejections(dev, LB):
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    def mk(alg=None, cells=None, m=1000, n=1000, band=64, **kw):
        args = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2)
        args.update(kw)
        return Plan(LB.NW_SCORED if alg is None else alg, LB.CELLS_DIR if cells is None else cells, [m], [n], [0],
                    [0], band=band, **args)

    for cells in (LB.CELLS_H, LB.CELLS_TAB):
        assert _status(lambda: mk(cells=cells)) == UNSUPPORTED, cells
    assert _status(lambda: mk(match=128)) == UNSUPPORTED
    assert _status(lambda: mk(mismatch=-129)) == UNSUPPORTED
    assert _status(lambda: mk(gap_open=1, gap_extend=2)) == UNSUPPORTED
    assert _status(lambda: mk(gap_open=1, gap_extend=-1)) == UNSUPPORTED
    assert _status(lambda: mk(m=500, n=400, band=10)) == ARG
    # a table enters through NW_SCORED alone; NW_ALIGN and NW_BANDED keep their 1 / 0
    assert _status(lambda: mk(alg=LB.NW_ALIGN, match=1, mismatch=0, gap_open=3, gap_extend=1,
                              sub=RS.sub8(IDENT))) == UNSUPPORTED
    assert _status(lambda: mk(alg=LB.NW_BANDED, cells=LB.CELLS_H, match=1, mismatch=0, sub=RS.sub8(IDENT))) \
        == UNSUPPORTED
    assert _status(lambda: mk(alg=LB.NW_ALIGN)) == UNSUPPORTED  # (match 2 / mismatch -3, as before)
    ok = mk()
    assert ok.format_info()["int16_cells"] == 0 and mk(cells=LB.CELLS_NONE).cells_elems == 0
    # the other walkers reject a scored plan before any launch
    d = torch.zeros(ok.cells_elems, dtype=torch.uint8, device=dev)
    ops = torch.zeros(64, dtype=torch.uint8, device=dev)
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    L, P = LB.lib(), lambda t: C.c_void_p(t.data_ptr())
    assert L.msa_plan_traceback(ok._h, 0, P(d), P(ops), 64, P(info), None) == UNSUPPORTED
    assert L.msa_plan_traceback_gotoh(ok._h, 0, -1, P(d), P(ops), 64, P(info), None) == UNSUPPORTED
    none = mk(cells=LB.CELLS_NONE)
    assert L.msa_plan_traceback_nw(none._h, 0, P(d), P(ops), 64, P(info), None) == UNSUPPORTED  # no bytes to walk
    off = torch.zeros(2, dtype=torch.int64, device=dev)
    assert L.msa_plan_traceback_batch(none._h, P(d), P(ops), P(off), P(info), None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert int(info.abs().sum()) == 0 and int(ops.sum()) == 0  # nothing ran


@pytest.mark.parametrize("match,mode", [(7, "band"), (8, "stripe")])
def test_band_byte_bound(dev, LB, match, mode):
    """band_kernel's profile bytes are S + 2g + h: with g = 50, h = 20 match 7 is byte 127, match 8 would be 128
    and runs the exact stripe launch (raw S).  Both are correct."""
    A, B, band, _, _ = R.SMALL["random_300x290_w32"]()
    S, g, h = RS.match_mismatch(b"ACGT", match, -3), 50, 20
    ref = RS.nw_scored_reference(A, B, b"ACGT", S, g, h, band)
    pl, dDir = _fill(LB, dev, A, B, band, b"ACGT", S, g, h, how="mm")
    assert pl.launch_info()["mode"] == mode
    _check(pl, dDir, A, B, band, b"ACGT", S, g, h, ref)


def _in_range(s, g, h, m, n):
    """The value-range rule of NW_SCORED plans, restated (check_ranges, msa_plan.inc; include/msa.h): s = the
    largest |score|, G = g + h."""
    return (s + 2 * (g + h) + 2 * g) * (m + n + 256) + h < 2 ** 28


@pytest.mark.parametrize("band", [-1, 8])
def test_value_range_bound(dev, LB, band):
    """The largest admitted gap extension for a 65 x 70 pair with mismatch -128 and h = 3, on an all-mismatch
    input: every diagonal step costs 128 and the border corner reaches -h - g max(m, n) (no band) in real cells.
    One more is rejected at creation."""
    m, n, h, s = 65, 70, 3, 128
    g = (2 ** 28 - 1 - h) // (m + n + 256)  # (s + 4g + 2h) T + h < 2^28
    g = (g - s - 2 * h) // 4
    while _in_range(s, g + 1, h, m, n):
        g += 1
    assert _in_range(s, g, h, m, n) and not _in_range(s, g + 1, h, m, n) and g > 100000
    S = RS.match_mismatch(b"ACGT", 1, -128)
    A, B = b"A" * m, b"C" * n
    assert _status(lambda: _plan(LB, [m], [n], [0], [0], band, S, g + 1, h)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, [m], [n], [0], [0], band, S, g + 1, h, how="mm")) == UNSUPPORTED
    ref = RS.nw_scored_reference(A, B, b"ACGT", S, g, h, band)
    assert ref["score"] == -128 * m - h - g * (n - m)  # the diagonal and one gap of n - m
    # (the first in-band cell of the last border row, (band + 1, 1) or (m, 1), holds -h - g (i - 1) - 128)
    assert int(ref["H"][ref["valid"] & (ref["H"] > RS.NEG // 2)].min()) < -g * ((8 if band >= 0 else m) - 1)
    pl, dDir = _fill(LB, dev, A, B, band, b"ACGT", S, g, h)
    assert pl.launch_info()["mode"] == "stripe"  # (the profile byte S + 2g + h does not fit int8)
    _check(pl, dDir, A, B, band, b"ACGT", S, g, h, ref)


# ---- 7. host entries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random_1000x1030_w64", "random_500x480_noband"])
def test_host_entry(dev, LB, name):
    from cse305_parallel_sequence_alignment_amd import api

    # match / mismatch ("dna": 2 / -3, g = 2, h = 3)
    A, B, band, alphabet, S, g, h, ref = _case(name, "dna")
    want = dict(score=ref["score"], cigar=R.cigar_of(ref["ops"]))
    assert api.nw_align(A, B, match=2, mismatch=-3, gap_open=5, gap_extend=2, band=band) == want
    assert api.nw_align(A, B, match=2, mismatch=-3, gap_open=5, gap_extend=2, band=band, traceback=False) == \
        dict(score=ref["score"])
    # S, g and h all times 3: the same alignment, three times the score
    r3 = api.nw_align(A, B, match=6, mismatch=-9, gap_open=15, gap_extend=6, band=band)
    assert r3 == dict(score=3 * ref["score"], cigar=want["cigar"])
    # alphabet + matrix ("titv")
    A, B, band, alphabet, S, g, h, ref = _case(name, "titv")
    want = dict(score=ref["score"], cigar=R.cigar_of(ref["ops"]))
    assert api.nw_align(A, B, alphabet=alphabet, matrix=S, gap_open=g + h, gap_extend=g, band=band) == want
    assert api.nw_align(A, B, alphabet=alphabet, matrix=S, gap_open=g + h, gap_extend=g, band=band,
                        traceback=False) == dict(score=ref["score"])
    r3 = api.nw_align(A, B, alphabet=alphabet, matrix=3 * S, gap_open=3 * (g + h), gap_extend=3 * g, band=band)
    assert r3 == dict(score=3 * ref["score"], cigar=want["cigar"])
    # a symbol outside the alphabet
    assert _status(lambda: api.nw_align(A, B, alphabet=b"ACGT", matrix=S[:4, :4], band=band)) == ALPHABET


def test_host_batch(dev, LB):
    from cse305_parallel_sequence_alignment_amd import api

    kw = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2)
    pairs = R.batch_pairs()
    As, Bs = [a for a, _ in pairs], [b for _, b in pairs]
    for band in (64, -1):
        assert api.nw_align_batch(As, Bs, band=band, **kw) == [api.nw_align(a, b, band=band, **kw) for a, b in pairs]
    assert api.nw_align_batch(As, Bs, band=64, traceback=False, **kw) == \
        [api.nw_align(a, b, band=64, traceback=False, **kw) for a, b in pairs]
    # three queries against one shared B, under a matrix
    alphabet, S, g, h = RS.SCORE_SETS["titv"]
    rng = np.random.default_rng(23)
    Bq = RS.with_n(R.rs(rng, 300), 303)
    Qs = [RS.with_n(Bq[10:250], 304), RS.with_n(R.rs(rng, 280), 305), Bq[:290]]
    mk = dict(alphabet=alphabet, matrix=S, gap_open=g + h, gap_extend=g, band=64)
    got = api.nw_align_batch(Qs, Bq, **mk)
    assert got == [api.nw_align(q, Bq, **mk) for q in Qs]
    for q, r in zip(Qs, got):
        ref = RS.nw_scored_reference(q, Bq, alphabet, S, g, h, 64)
        assert r == dict(score=ref["score"], cigar=R.cigar_of(ref["ops"]))
    assert _status(lambda: api.nw_align_batch(Qs, Bq + b"X", **mk)) == ALPHABET
