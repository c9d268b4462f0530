"""Banded extension alignment (MSA_NW_EXTEND_BAND plans, msa_extend_align_banded, msa_extend_align_batch_banded and
their *32 twins, api.extend_align(band=)) against the numpy yardstick tests/extend_band_reference.py (itself checked
against a triple-loop banded Gotoh, the definition by exhaustion and the unbanded yardstick in
test_extend_band_reference.py).

Every fill case checks, exactly (integer DP): the score, the end cell, fin[0] == H(m', n'), the status and the plan's
error word; the launch mode and the end-cell tracking; bits 0-1 of every in-band interior direction byte, bit 2 where E
is finite and bit 3 where F is finite, against the yardstick AND against a banded MSA_NW_SCORED plan run on the same
input (a batch of one: the stripe launch at every band); the walk's ops byte for byte, its stop cell and the CIGAR with
its border gap; and the ops rescored on the two prefixes, which asserts that the path stays inside the band.  A plan
takes clipped sizes; the host entries clip.  The shapes (extend_band_reference.CASES) are the smallest at which each
mechanism can fail: a stripe a full stripe away from the matrix borders under a band >= 64 (the v_writelane edge phases
with the tracker in them) with the end cell on either edge of the band; a better alignment one diagonal outside the
band; unmasked body phases inside a band; bands that never take that path; clipped pairs; empty extensions; one pair
over several workgroups; batches; 8 and 24 symbols."""
import functools

import numpy as np
import pytest

import extend_band_reference as XB
import extend_reference as ER
import nw_reference as R
import nw_scored_reference as RS
import wide_reference as W

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG = -5, -1


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _dev(x, alphabet, dev):
    import torch

    return torch.from_numpy(ER.codes(x, alphabet).astype(np.uint8)).to(dev)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(A, B, alphabet, S, g, h, w, reference): a named case, or "eight" / "protein", "protein1", "protein2" under
    bands 32 / 16 (both clip); computed once and shared (never modified)."""
    if name == "eight":
        A, B, alphabet, S, g, h = ER.eight_symbols()
        w = 32
    elif name.startswith("protein"):
        A, B, alphabet, S, g, h = ER.protein32(int(name[7:] or 0))
        w = 16
    else:
        return XB.case(name)
    return A, B, alphabet, S, g, h, w, XB.extend_band_reference(A, B, alphabet, S, g, h, w)


def _plan(LB, ms, ns, a_offs, b_offs, S, g, h, band, cells=None, how="sub", alg=None, single=None, profile=None):
    """An NW_EXTEND_BAND plan; how = "sub": the 8 x 8 table (32 x 32 for more than 8 symbols), "mm": S's match /
    mismatch through the description."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    if profile is not None:
        kw = dict(profile=profile)
    elif how == "mm":
        kw = dict(match=int(S[0][0]), mismatch=int(S[0][1]))
    else:
        kw = dict(sub=W.sub32(S) if len(S) > 8 else RS.sub8(S))
    return Plan(LB.NW_EXTEND_BAND if alg is None else alg, LB.CELLS_DIR if cells is None else cells, ms, ns, a_offs,
                b_offs, gap_open=g + h, gap_extend=g, band=band, single=single, **kw)


def _fill(LB, dev, A, B, alphabet, S, g, h, w, how="sub", alg=None, single=None):
    """The plan of the CLIPPED pair, run."""
    import torch

    me, ne = XB.clip(len(A), len(B), w)
    pl = _plan(LB, [me], [ne], [0], [0], S, g, h, w, how=how, alg=alg, single=single)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev(A[:me], alphabet, dev), _dev(B[:ne], alphabet, dev), dDir)
    return pl, dDir


def _bytes(pl, dDir, pair, w):
    return R.to_band(pl.deskew_dir(dDir.cpu().numpy(), pair, pl.stripe_meta()), w)


def _same_bytes(got, other, ref, what):
    v = ref["valid"]
    bad = v & ((got & 3) != (other & 3))
    assert not bad.any(), (what, "bits 0-1", int(bad.sum()), np.argwhere(bad)[:4])
    bad = v & ref["efin"] & ((got & 4) != (other & 4))
    assert not bad.any(), (what, "bit 2", int(bad.sum()), np.argwhere(bad)[:4])
    bad = v & ref["ffin"] & ((got & 8) != (other & 8))
    assert not bad.any(), (what, "bit 3", int(bad.sum()), np.argwhere(bad)[:4])


def _fin0(ref, A, B, alphabet, S, g, h):
    """H(m', n') of the clipped pair: the reference's global score, or for a clipped pair the band-form corner."""
    me, ne, w = ref["m_eff"], ref["n_eff"], ref["w"]
    return int(ref["H"][me, ne - me + w])


def _check_result(pl, ref, A, B, alphabet, S, g, h, pair=0):
    res = pl.results()[pair]
    assert res["score"] == ref["score"]
    assert tuple(res["end"]) == ref["end"]
    assert res["fin"][0] == _fin0(ref, A, B, alphabet, S, g, h)
    if ref["global_score"] is not None:
        assert res["fin"][0] == ref["global_score"]
    assert res["status"] == 0
    assert pl.error() == 0
    assert pl.launch_info()["mode"] == "stripe"
    assert pl.format_info()["tracking"] == "select"
    return res


def _check(pl, dDir, A, B, alphabet, S, g, h, ref, pair=0, scored=None):
    """Everything a fill test checks for one pair (see the module docstring); scored = (plan, bytes) of a banded
    NW_SCORED plan run on the same clipped input."""
    w = ref["w"]
    res = _check_result(pl, ref, A, B, alphabet, S, g, h, pair)
    got = _bytes(pl, dDir, pair, w)
    _same_bytes(got, ref["byte"], ref, "yardstick")
    if scored is not None:
        spl, sDir = scored
        assert spl.results()[pair]["score"] == res["fin"][0]
        _same_bytes(got, _bytes(spl, sDir, pair, w), ref, "NW_SCORED plan")
    tb = pl.traceback_nw(dDir, pair)
    assert tb["ops"] == ref["ops"]
    assert tb["stop"] == ref["stop"]
    assert tb["cigar"] == XB.cigar_of(ref["ops"])
    assert XB.rescore(A, B, tuple(res["end"]), tb["ops"], alphabet, S, g, h, w) == ref["score"]
    return tb


# ---- 1. one pair: spread over workgroups (single = 1) and as a batch of one (single = 0, the batch kernel) -------
NAMES = list(XB.CASES) + ["eight", "protein"]


@pytest.mark.parametrize("single", [True, False], ids=["single", "batch1"])
@pytest.mark.parametrize("name", NAMES)
def test_fill_and_walk(dev, LB, name, single):
    A, B, alphabet, S, g, h, w, ref = _case(name)
    me, ne = ref["m_eff"], ref["n_eff"]
    how = "mm" if name in ("random_400_w64", "similar_150_w8") else "sub"
    pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h, w, how=how, single=single)
    assert pl.single == single and pl.format_info()["codes"] == (32 if len(alphabet) > 8 else 8)
    if name == "single_1000_w100" and single:
        assert pl.launch_info()["items"] > 1
    # (the banded NW_SCORED plan as a batch of one: the stripe launch, the extension's own, at every band)
    scored = _fill(LB, dev, A, B, alphabet, S, g, h, w, how=how, alg=LB.NW_SCORED, single=False)
    assert scored[0].launch_info()["mode"] == "stripe"
    tb = _check(pl, dDir, A, B, alphabet, S, g, h, ref, scored=scored)
    if name in XB.KNOWN:
        score, end, cigar, gs = XB.KNOWN[name]
        assert (ref["score"], ref["end"], tb["cigar"]) == (score, end, cigar)
    # a score-only plan (no direction bytes) reaches the same score, end cell and fin
    none = _plan(LB, [me], [ne], [0], [0], S, g, h, w, cells=LB.CELLS_NONE, how=how, single=single)
    assert none.cells_elems == 0
    none.run(_dev(A[:me], alphabet, dev), _dev(B[:ne], alphabet, dev))
    _check_result(none, ref, A, B, alphabet, S, g, h)


@pytest.mark.parametrize("name", [k for k in ER.SHAPES if k not in ("late_zero", "single_1000x3000")])
def test_full_band_is_the_unbanded_plan(dev, LB, name):
    """w = max(m, n): score, end cell, global score and bytes equal an NW_EXTEND plan's."""
    import torch

    set_name, make = ER.SHAPES[name]
    alphabet, S, g, h = ER.score_set(set_name)
    A, B = make()
    w = max(len(A), len(B))
    ref = ER.extend_reference(A, B, alphabet, S, g, h)
    dA, dB = _dev(A, alphabet, dev), _dev(B, alphabet, dev)
    out = []
    for alg, band in ((LB.NW_EXTEND_BAND, w), (LB.NW_EXTEND, -1)):
        pl = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, band, alg=alg)
        dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
        pl.run(dA, dB, dDir)
        res = pl.results()[0]
        assert (res["score"], tuple(res["end"]), res["fin"][0], res["status"]) == \
            (ref["score"], ref["end"], ref["global_score"], 0)
        assert pl.error() == 0 and pl.launch_info()["mode"] == "stripe" and pl.format_info()["tracking"] == "select"
        out.append((_bytes(pl, dDir, 0, w), pl.traceback_nw(dDir, 0)))
    _same_bytes(out[0][0], out[1][0], ref, "NW_EXTEND plan")
    _same_bytes(out[0][0], ref["byte"], ref, "yardstick")
    assert (out[0][1]["ops"], out[0][1]["stop"]) == (out[1][1]["ops"], out[1][1]["stop"]) == (ref["ops"], ref["stop"])


# ---- 2. a batch plan (single = 0) --------------------------------------------------------------------------------
def _offsets(seqs):
    return np.concatenate(([0], np.cumsum([len(s) for s in seqs])[:-1]))


def _batch_plan(dev, LB, pairs, alphabet, S, g, h, w, cells):
    """One plan for the clipped pairs (their offsets are the unclipped sequences': a prefix is kept)."""
    import torch

    refs = [XB.extend_band_reference(a, b, alphabet, S, g, h, w) for a, b in pairs]
    ms, ns = [r["m_eff"] for r in refs], [r["n_eff"] for r in refs]
    dA = _dev(b"".join(a for a, _ in pairs), alphabet, dev)
    dB = _dev(b"".join(b for _, b in pairs), alphabet, dev)
    a_offs, b_offs = _offsets([a for a, _ in pairs]), _offsets([b for _, b in pairs])
    if cells == "none":
        pl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h, w, cells=LB.CELLS_NONE)
        pl.run(dA, dB)
        for k, ((a, b), ref) in enumerate(zip(pairs, refs)):
            _check_result(pl, ref, a, b, alphabet, S, g, h, pair=k)
        return
    pl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h, w)
    assert not pl.single
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(dA, dB, dDir)
    spl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h, w, alg=LB.NW_SCORED)
    sDir = torch.zeros(spl.cells_elems, dtype=torch.uint8, device=dev)
    spl.run(dA, dB, sDir)
    singles = [_check(pl, dDir, a, b, alphabet, S, g, h, ref, pair=k, scored=(spl, sDir))
               for k, ((a, b), ref) in enumerate(zip(pairs, refs))]
    batch = pl.traceback_batch(dDir)  # one launch for every pair
    for one, tb, ref in zip(singles, batch, refs):
        assert (tb["ops"], tb["stop"], tb["cigar"]) == (one["ops"], one["stop"], one["cigar"])
        if ref["score"] == 0:  # the empty extension: no walk
            assert (tb["ops"], tb["stop"]) == (b"", (0, 0))


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_batch_plan_mixed(dev, LB, cells):
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    _batch_plan(dev, LB, XB.batch_pairs(), alphabet, S, g, h, XB.BATCH_BAND, cells)


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_batch_plan_regular_stripes(dev, LB, cells):
    """The three 400 x 400 pairs under band 64 in one plan: every pair's stripe of rows 129..192 is regular."""
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = [_case(k)[:2] for k in ("upper_edge_w64", "lower_edge_w64", "random_400_w64")]
    _batch_plan(dev, LB, pairs, alphabet, S, g, h, 64, cells)


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_batch_plan_protein32(dev, LB, cells):
    cases = [_case(f"protein{k}") for k in range(3)]
    _, _, alphabet, S, g, h, w, _ = cases[0]
    _batch_plan(dev, LB, [(c[0], c[1]) for c in cases], alphabet, S, g, h, w, cells)


def test_plan_reuse(dev, LB):
    """One plan, run again on different inputs of its sizes: each run's results and bytes are that run's own."""
    import torch

    names = ("upper_edge_w64", "random_400_w64", "lower_edge_w64", "upper_edge_w64")
    A, B, alphabet, S, g, h, w, _ = _case(names[0])
    pl = _plan(LB, [400], [400], [0], [0], S, g, h, w)
    none = _plan(LB, [400], [400], [0], [0], S, g, h, w, cells=LB.CELLS_NONE, single=False)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    for name in names:
        A, B, alphabet, S, g, h, w, ref = _case(name)
        pl.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev), dDir)
        _check(pl, dDir, A, B, alphabet, S, g, h, ref)
        none.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev))
        _check_result(none, ref, A, B, alphabet, S, g, h)


# ---- 3. the host entries ---------------------------------------------------------------------------------------
DNA_KW = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2)


def _want(ref, traceback=True):
    r = dict(score=ref["score"], a_end=ref["end"][0], b_end=ref["end"][1], global_score=ref["global_score"])
    if traceback:
        r["cigar"] = XB.cigar_of(ref["ops"])
    return r


@pytest.mark.parametrize("name", ["upper_edge_w64", "outside_69_w64", "edge_64_w64", "clip_rows_400x150_w16",
                                  "clip_cols_150x400_w16", "clip_one_stripe_300x40_w8", "all_negative_w16",
                                  "equal_150_w0", "corner_on_edge_300x290_w10", "random_300x290_w8"])
def test_api_extend_align(dev, name):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, alphabet, S, g, h, w, ref = _case(name)
    r = api.extend_align(A, B, band=w, **DNA_KW)
    assert r == _want(ref)
    assert api.extend_align(A, B, band=w, traceback=False, **DNA_KW) == _want(ref, False)
    assert (r["global_score"] is None) == (name in XB.CLIPPED)
    # the two prefixes' banded global alignment has the extension's score, and the whole pair's the global score
    # (nw_align_batch: the stripe launch at every band)
    if r["score"] > 0:
        piece, = api.nw_align_batch([A[:r["a_end"]]], [B[:r["b_end"]]], band=w, traceback=False, **DNA_KW)
        assert piece["score"] == r["score"]
    if r["global_score"] is not None:
        whole, = api.nw_align_batch([A], [B], band=w, traceback=False, **DNA_KW)
        assert whole["score"] == r["global_score"]
    # alphabet + matrix reach the same result; a band past both lengths is the unbanded extension
    assert api.extend_align(A, B, band=w, gap_open=g + h, gap_extend=g, alphabet=alphabet, matrix=S) == r
    big = api.extend_align(A, B, band=1 << 40, **DNA_KW)
    assert big == api.extend_align(A, B, **DNA_KW)


def test_api_extend_align_symbols(dev):
    from cse305_parallel_sequence_alignment_amd import api

    cases = [_case(f"protein{k}") for k in range(3)]
    _, _, alphabet, S, g, h, w, _ = cases[0]
    kw = dict(gap_open=g + h, gap_extend=g, alphabet=alphabet, matrix=S, max_symbols=32, band=w)
    assert api.extend_align(cases[0][0], cases[0][1], **kw) == _want(cases[0][7])
    got = api.extend_align_batch([c[0] for c in cases], [c[1] for c in cases], **kw)
    assert got == [_want(c[7]) for c in cases]
    # 8 symbols or fewer under the *32 entries: the plain entries' plans and results
    A, B, al8, S8, g8, h8, w8, ref8 = _case("eight")
    kw8 = dict(gap_open=g8 + h8, gap_extend=g8, alphabet=al8, matrix=S8, band=w8)
    assert api.extend_align(A, B, max_symbols=32, **kw8) == api.extend_align(A, B, **kw8) == _want(ref8)
    assert api.extend_align_batch([A, A[:90]], [B, B], **kw8)[0] == _want(ref8)


def test_api_extend_align_batch(dev):
    from cse305_parallel_sequence_alignment_amd import api

    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    w = XB.BATCH_BAND
    pairs = XB.batch_pairs()
    want = [XB.extend_band_reference(a, b, alphabet, S, g, h, w) for a, b in pairs]
    got = api.extend_align_batch([a for a, _ in pairs], [b for _, b in pairs], band=w, **DNA_KW)
    assert got == [_want(x) for x in want]
    assert [r["global_score"] is None for r in got] == [False, True, False, False, True]
    got0 = api.extend_align_batch([a for a, _ in pairs], [b for _, b in pairs], band=w, traceback=False, **DNA_KW)
    assert got0 == [_want(x, False) for x in want]
    # many reads against one B shared by every pair (each read clips it to its own length + band)
    As, ref_b = XB.shared_b_batch()
    As = As * 8
    want = [XB.extend_band_reference(a, ref_b, alphabet, S, g, h, w) for a in As[:5]] * 8
    assert api.extend_align_batch(As, ref_b, band=w, **DNA_KW) == [_want(x) for x in want]


# ---- 4. plan creation, the walkers ------------------------------------------------------------------------------
def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_plan_creation_errors(dev, LB):
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, 16)) == 0
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, 16, how="mm")) == 0
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, -1)) == UNSUPPORTED       # a band is required
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, -2)) == UNSUPPORTED
    for cells in (LB.CELLS_H, LB.CELLS_TAB):
        assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, 16, cells=cells)) == UNSUPPORTED
    prof = np.zeros((100, 32), dtype=np.int8)
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, 16, profile=prof)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, -1, 3, 16)) == UNSUPPORTED      # g < 0
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, 2, -1, 16)) == UNSUPPORTED      # h < 0
    # a plan takes clipped sizes: |m - n| > band is every banded plan's MSA_ERR_ARG
    assert _status(lambda: _plan(LB, [100], [117], [0], [0], S, g, h, 16)) == ARG
    assert _status(lambda: _plan(LB, [117], [100], [0], [0], S, g, h, 16)) == ARG
    assert _status(lambda: _plan(LB, [100], [116], [0], [0], S, g, h, 16)) == 0
    assert _status(lambda: _plan(LB, [100, 100], [100, 117], [0, 0], [0, 0], S, g, h, 16)) == ARG
    # NW_EXTEND keeps rejecting any band
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, 16, alg=LB.NW_EXTEND)) == UNSUPPORTED
    # 5-bit codes: the same rules
    S24 = W.table32()[:24, :24]
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S24, 2, 9, 16)) == 0
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S24, 2, 9, -1)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S24, 2, 9, 16, cells=LB.CELLS_H)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, [100], [117], [0], [0], S24, 2, 9, 16)) == ARG
    # one long banded pair stays on the exact stripe launch (no band, chunked or flow launch), and a batch of equal-m
    # pairs too small to fill the chip is whole pairs per workgroup: mode 0, never split
    for ms, ns in (([9000], [9000]), ([1100] * 4, [1200] * 4)):
        for cells in (LB.CELLS_NONE, LB.CELLS_DIR):
            pl = _plan(LB, ms, ns, [0] * len(ms), [0] * len(ms), S, g, h, 128, cells=cells)
            assert pl.launch_info()["mode"] == "stripe" and pl.format_info()["tracking"] == "select"


def test_other_walkers_reject_the_plan(dev, LB):
    import torch

    A, B, alphabet, S, g, h, w, ref = _case("similar_150_w8")
    pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h, w)
    ops = torch.empty(len(A) + len(B) + 2, dtype=torch.uint8, device=dev)
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    assert _status(lambda: pl.traceback_async(dDir, ops, info)) == UNSUPPORTED
    assert _status(lambda: pl.traceback_gotoh_async(dDir, ops, info)) == UNSUPPORTED
    none = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, w, cells=LB.CELLS_NONE)
    assert _status(lambda: none.traceback_nw_async(dDir, ops, info)) == UNSUPPORTED


def test_walk_before_any_run(dev, LB):
    """A plan that has not run has no end cell: both walkers report MSA_ERR_ARG in the walk's status."""
    import torch

    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pl = _plan(LB, [70], [90], [0], [0], S, g, h, 20)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    assert _status(lambda: pl.traceback_nw(dDir)) == ARG
    bp = _plan(LB, [70, 30], [90, 40], [0, 70], [0, 90], S, g, h, 20)
    dDir = torch.zeros(bp.cells_elems, dtype=torch.uint8, device=dev)
    assert _status(lambda: bp.traceback_batch(dDir)) == ARG
