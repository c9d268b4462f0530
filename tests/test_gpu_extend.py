"""Extension (anchored-start, free-end) alignment (MSA_NW_EXTEND plans, msa_extend_align, msa_extend_align_batch and
their *32 twins) against the numpy yardstick tests/extend_reference.py (itself checked against a triple-loop Gotoh and
the definition by exhaustion in test_extend_reference.py).

Every fill case checks, exactly (integer DP): the score, the end cell, fin[0] == the global score, the status and the
plan's error word; the launch mode and the end-cell tracking; bits 0-1 of every interior direction byte, bit 2 where E
is finite and bit 3 where F is finite, against the yardstick AND against an MSA_NW_SCORED plan run on the same input;
the walk's ops byte for byte, its stop cell and the CIGAR with its border gap; and the ops rescored on the two
prefixes.  The shapes (extend_reference.SHAPES) are the smallest at which each mechanism can fail: the end cell in the
first, a middle, the last stripe, in lane 0 and lane 63, on row m, column n, column 1, at (m, n) and (1, 1); a single
row, a single column, n < 64, m = 64 and 65, column n in the last of many phases; equal maxima in two stripes, two
lanes, one row, a masked and an unmasked phase; every H negative, whole stripes negative, a best of exactly 0, zero
borders, rows past m; one pair over several workgroups; batches; 8 and 24 symbols."""
import ctypes as C
import functools

import numpy as np
import pytest

import extend_reference as ER
import nw_reference as R
import nw_scored_reference as RS
import wide_reference as W

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG, CAPACITY = -5, -1, -8


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _dev(x, alphabet, dev):
    import torch

    return torch.from_numpy(ER.codes(x, alphabet).astype(np.uint8)).to(dev)


@functools.lru_cache(maxsize=None)
def _case(name, set_name=None):
    """(A, B, alphabet, S, g, h, reference) of a named shape ("eight" / "protein", "protein1", "protein2": their own
    scoring; set_name: another score set than the shape's own), computed once and shared (never modified)."""
    if name == "eight":
        A, B, alphabet, S, g, h = ER.eight_symbols()
    elif name.startswith("protein"):
        A, B, alphabet, S, g, h = ER.protein32(int(name[7:] or 0))
    else:
        own, make = ER.SHAPES[name]
        alphabet, S, g, h = ER.score_set(set_name or own)
        A, B = make()
    return A, B, alphabet, S, g, h, ER.extend_reference(A, B, alphabet, S, g, h)


def _plan(LB, ms, ns, a_offs, b_offs, S, g, h, cells=None, how="sub", band=-1, alg=None):
    """An NW_EXTEND plan; how = "sub": the 8 x 8 table (32 x 32 for more than 8 symbols), "mm": S's match / mismatch
    through the description."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    if how == "mm":
        kw = dict(match=int(S[0][0]), mismatch=int(S[0][1]))
    else:
        kw = dict(sub=W.sub32(S) if len(S) > 8 else RS.sub8(S))
    return Plan(LB.NW_EXTEND if alg is None else alg, LB.CELLS_DIR if cells is None else cells, ms, ns, a_offs, b_offs,
                gap_open=g + h, gap_extend=g, band=band, **kw)


def _fill(LB, dev, A, B, alphabet, S, g, h, how="sub", alg=None):
    import torch

    pl = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, how=how, alg=alg)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev), dDir)
    return pl, dDir


def _bytes(pl, dDir, pair, w):
    return R.to_band(pl.deskew_dir(dDir.cpu().numpy(), pair, pl.stripe_meta()), w)


def _check(pl, dDir, A, B, alphabet, S, g, h, ref, pair=0, scored=None):
    """Everything a fill test checks for one pair (see the module docstring); scored = (plan, bytes) of an NW_SCORED
    plan run on the same input."""
    w = ref["w"]
    res = pl.results()[pair]
    assert res["score"] == ref["score"]
    assert tuple(res["end"]) == ref["end"]
    assert res["fin"][0] == ref["global_score"]
    assert res["status"] == 0
    assert pl.error() == 0
    assert pl.launch_info()["mode"] == "stripe"
    assert pl.format_info()["tracking"] == "select"
    got = _bytes(pl, dDir, pair, w)
    v, want = ref["valid"], ref["byte"]
    others = [("yardstick", want)]
    if scored is not None:
        spl, sDir = scored
        assert spl.results()[pair]["score"] == ref["global_score"]
        others.append(("NW_SCORED plan", _bytes(spl, sDir, pair, w)))
    for what, other in others:
        bad = v & ((got & 3) != (other & 3))
        assert not bad.any(), (what, "bits 0-1", int(bad.sum()), np.argwhere(bad)[:4])
        bad = v & ref["efin"] & ((got & 4) != (other & 4))
        assert not bad.any(), (what, "bit 2", int(bad.sum()), np.argwhere(bad)[:4])
        bad = v & ref["ffin"] & ((got & 8) != (other & 8))
        assert not bad.any(), (what, "bit 3", int(bad.sum()), np.argwhere(bad)[:4])
    tb = pl.traceback_nw(dDir, pair)
    assert tb["ops"] == ref["ops"]
    assert tb["stop"] == ref["stop"]
    assert tb["cigar"] == ER.cigar_of(ref["ops"])
    assert ER.rescore(A, B, tuple(res["end"]), tb["ops"], alphabet, S, g, h) == ref["score"]
    return tb


# ---- 1. one pair (single = 1) ----------------------------------------------------------------------------------
CASES = [(n, None, "sub") for n in ER.SHAPES if n != "single_1000x3000"] + \
        [("middle_stripe", "dna", "mm"), ("tie_zero_rect", "zero", "mm"), ("middle_stripe", "asym", "sub"),
         ("row65", "unit", "mm"), ("eight", None, "sub"), ("protein", None, "sub")]


@pytest.mark.parametrize("name,set_name,how", CASES, ids=lambda x: str(x))
def test_fill_and_walk(dev, LB, name, set_name, how):
    A, B, alphabet, S, g, h, ref = _case(name, set_name)
    pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h, how=how)
    assert pl.format_info()["codes"] == (32 if len(alphabet) > 8 else 8)
    scored = _fill(LB, dev, A, B, alphabet, S, g, h, how=how, alg=LB.NW_SCORED)
    tb = _check(pl, dDir, A, B, alphabet, S, g, h, ref, scored=scored)
    if set_name is None and name in ER.KNOWN:
        assert (ref["score"], ref["end"], tb["cigar"]) == ER.KNOWN[name]
    if name == "eight":
        ei, ej = ref["end"]
        assert set(A[:ei]) == set(B[:ej]) == set(alphabet)
    # a score-only plan (no direction bytes) reaches the same score, end cell and global score
    none = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, cells=LB.CELLS_NONE, how=how)
    assert none.cells_elems == 0 and none.launch_info()["mode"] == "stripe"
    assert none.format_info()["tracking"] == "select"
    none.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev))
    res = none.results()[0]
    assert (res["score"], tuple(res["end"]), res["fin"][0], res["status"]) == \
        (ref["score"], ref["end"], ref["global_score"], 0)
    assert none.error() == 0


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_one_pair_over_many_workgroups(dev, LB, cells):
    """1,000 rows: 16 stripes in several items, chained through granules; the end cell is in stripe 10."""
    A, B, alphabet, S, g, h, ref = _case("single_1000x3000")
    assert ref["end"] == (700, 700) and ref["score"] > 0 > ref["global_score"]
    if cells == "dir":
        pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h)
        assert pl.single and pl.launch_info()["items"] > 1
        _check(pl, dDir, A, B, alphabet, S, g, h, ref)
        return
    pl = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, cells=LB.CELLS_NONE)
    assert pl.cells_elems == 0 and pl.launch_info()["mode"] == "stripe" and pl.launch_info()["items"] > 1
    pl.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev))
    res = pl.results()[0]
    assert (res["score"], tuple(res["end"]), res["fin"][0], res["status"]) == \
        (ref["score"], ref["end"], ref["global_score"], 0)
    assert pl.error() == 0


# ---- 2. a batch plan (single = 0) --------------------------------------------------------------------------------
def _offsets(seqs):
    return np.concatenate(([0], np.cumsum([len(s) for s in seqs])[:-1]))


def _batch_plan(dev, LB, pairs, alphabet, S, g, h, cells):
    import torch

    ms, ns = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    dA = _dev(b"".join(a for a, _ in pairs), alphabet, dev)
    dB = _dev(b"".join(b for _, b in pairs), alphabet, dev)
    refs = [ER.extend_reference(a, b, alphabet, S, g, h) for a, b in pairs]
    a_offs, b_offs = _offsets([a for a, _ in pairs]), _offsets([b for _, b in pairs])
    if cells == "none":
        pl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h, cells=LB.CELLS_NONE)
        pl.run(dA, dB)
        for res, ref in zip(pl.results(), refs):
            assert (res["score"], tuple(res["end"]), res["fin"][0], res["status"]) == \
                (ref["score"], ref["end"], ref["global_score"], 0)
        assert pl.error() == 0 and pl.launch_info()["mode"] == "stripe"
        return
    pl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h)
    assert not pl.single
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(dA, dB, dDir)
    spl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h, alg=LB.NW_SCORED)
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
def test_batch_plan(dev, LB, cells):
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = ER.batch_pairs()
    assert ([len(a) for a, _ in pairs], [len(b) for _, b in pairs]) == (ER.BATCH_MS, ER.BATCH_NS)
    _batch_plan(dev, LB, pairs, alphabet, S, g, h, cells)


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_batch_plan_zero_gaps(dev, LB, cells):
    """g = h = 0 in a batch: zero borders, and maxima attained on whole rectangles of cells."""
    alphabet, S, g, h = ER.ZERO
    pairs = [ER.SHAPES[k][1]() for k in ("col_1", "tie_zero_rect", "zero_borders")]
    _batch_plan(dev, LB, pairs, alphabet, S, g, h, cells)


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_batch_plan_protein32(dev, LB, cells):
    cases = [_case(f"protein{k}") for k in range(3)]
    _, _, alphabet, S, g, h, _ = cases[0]
    _batch_plan(dev, LB, [(c[0], c[1]) for c in cases], alphabet, S, g, h, cells)


# ---- 3. the host entries ---------------------------------------------------------------------------------------
DNA_KW = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2)


def _want(ref, traceback=True):
    r = dict(score=ref["score"], a_end=ref["end"][0], b_end=ref["end"][1], global_score=ref["global_score"])
    if traceback:
        r["cigar"] = ER.cigar_of(ref["ops"])
    return r


@pytest.mark.parametrize("name", ["middle_stripe", "row65", "corner", "all_negative", "tie_two_stripes", "col_n"])
def test_api_extend_align(dev, name):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, alphabet, S, g, h, ref = _case(name)
    r = api.extend_align(A, B, **DNA_KW)
    assert r == _want(ref)
    assert api.extend_align(A, B, traceback=False, **DNA_KW) == _want(ref, False)
    # the two prefixes' global alignment has the extension's score, and the whole pair's the global score
    if r["score"] > 0:
        piece = api.nw_align(A[:r["a_end"]], B[:r["b_end"]], traceback=False, **DNA_KW)
        assert piece["score"] == r["score"]
    assert api.nw_align(A, B, traceback=False, **DNA_KW)["score"] == r["global_score"]
    # alphabet + matrix reach the same result
    assert api.extend_align(A, B, gap_open=g + h, gap_extend=g, alphabet=alphabet, matrix=S) == r


def test_api_extend_align_zero_gaps(dev):
    from cse305_parallel_sequence_alignment_amd import api

    for name in ("col_1", "zero_borders"):
        A, B, alphabet, S, g, h, ref = _case(name)
        assert api.extend_align(A, B, match=1, mismatch=-1, gap_open=0, gap_extend=0) == _want(ref)


def test_api_extend_align_32_symbols(dev):
    from cse305_parallel_sequence_alignment_amd import api

    cases = [_case(f"protein{k}") for k in range(3)]
    _, _, alphabet, S, g, h, _ = cases[0]
    kw = dict(gap_open=g + h, gap_extend=g, alphabet=alphabet, matrix=S, max_symbols=32)
    assert api.extend_align(cases[0][0], cases[0][1], **kw) == _want(cases[0][6])
    got = api.extend_align_batch([c[0] for c in cases], [c[1] for c in cases], **kw)
    assert got == [_want(c[6]) for c in cases]
    # 8 symbols or fewer under the *32 entries: the plain entries' plans and results
    A, B, al8, S8, g8, h8, ref8 = _case("eight")
    kw8 = dict(gap_open=g8 + h8, gap_extend=g8, alphabet=al8, matrix=S8)
    assert api.extend_align(A, B, max_symbols=32, **kw8) == api.extend_align(A, B, **kw8) == _want(ref8)


def test_api_extend_align_batch(dev):
    from cse305_parallel_sequence_alignment_amd import api

    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = ER.batch_pairs()
    want = [ER.extend_reference(a, b, alphabet, S, g, h) for a, b in pairs]
    got = api.extend_align_batch([a for a, _ in pairs], [b for _, b in pairs], **DNA_KW)
    assert got == [_want(w) for w in want]
    got0 = api.extend_align_batch([a for a, _ in pairs], [b for _, b in pairs], traceback=False, **DNA_KW)
    assert got0 == [_want(w, False) for w in want]
    # one B shared by every pair
    As, ref_b = ER.shared_b_batch()
    want = [ER.extend_reference(a, ref_b, alphabet, S, g, h) for a in As]
    assert api.extend_align_batch(As, ref_b, **DNA_KW) == [_want(w) for w in want]


def test_entry_capacity(dev, LB):
    """A cigar buffer too small: MSA_ERR_CAPACITY (the batch: with the needed size in cigar_off[n_pairs]; that size
    suffices), the scores and the end cell still reported; cigar == NULL calls; the *32 twins."""
    A, B, alphabet, S, g, h, ref = _case("middle_stripe")
    sub = np.ascontiguousarray(S, dtype=np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for entry in ("msa_extend_align", "msa_extend_align32"):
        sc, gs = C.c_int32(), C.c_int32()
        end = np.zeros(2, dtype=np.int64)
        cig = C.create_string_buffer(16)
        f = getattr(LB.lib(), entry)
        args = (A, len(A), B, len(B), alphabet, len(alphabet), p(sub), g + h, g, C.byref(sc), p(end), C.byref(gs), cig)
        assert f(*args, len("150M")) == CAPACITY  # (no room for the NUL)
        assert (sc.value, end.tolist(), gs.value) == (300, [150, 150], ref["global_score"])
        assert f(*args, len("150M") + 1) == 0
        assert (cig.value, sc.value, end.tolist(), gs.value) == (b"150M", 300, [150, 150], ref["global_score"])
        # score only through the C entry; the end cell and the global score may be NULL
        sc.value = 0
        assert f(*args[:-1], None, 0) == 0 and sc.value == 300
        assert f(*args[:10], None, None, None, 0) == 0

    pairs = ER.batch_pairs()
    want = [ER.extend_reference(a, b, alphabet, S, g, h) for a, b in pairs]
    k = len(pairs)
    Ab, Bb = b"".join(a for a, _ in pairs), b"".join(b for _, b in pairs)
    m = np.array(ER.BATCH_MS, dtype=np.int64)
    n = np.array(ER.BATCH_NS, dtype=np.int64)
    a_off, b_off = _offsets([a for a, _ in pairs]).astype(np.int64), _offsets([b for _, b in pairs]).astype(np.int64)

    def call(cap, entry="msa_extend_align_batch", cigars=True, gscore=True):
        scs, gss = np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32)
        en = np.zeros((k, 2), dtype=np.int64)
        coff = np.zeros(k + 1, dtype=np.int64)
        cg = C.create_string_buffer(max(cap, 1))
        rc = getattr(LB.lib(), entry)(Ab, len(Ab), Bb, len(Bb), k, p(a_off), p(m), p(b_off), p(n), alphabet,
                                      len(alphabet), p(sub), g + h, g, p(scs), p(en), p(gss) if gscore else None,
                                      cg if cigars else None, cap if cigars else 0, p(coff) if cigars else None)
        return rc, scs, en, gss, coff, cg

    cigars = [ER.cigar_of(w["ops"]) for w in want]
    need = sum(len(c) + 1 for c in cigars)
    rc, _, _, _, coff, _ = call(need - 1)
    assert rc == CAPACITY and int(coff[k]) == need
    for entry in ("msa_extend_align_batch", "msa_extend_align_batch32"):
        rc, scs, en, gss, coff, cg = call(need, entry)
        assert rc == 0
        assert [cg.raw[coff[q]:coff[q + 1] - 1].decode() for q in range(k)] == cigars
        assert scs.tolist() == [w["score"] for w in want] and gss.tolist() == [w["global_score"] for w in want]
        assert en.tolist() == [list(w["end"]) for w in want]
    rc, scs, en, gss, _, _ = call(0, cigars=False)
    assert rc == 0 and scs.tolist() == [w["score"] for w in want] and en.tolist() == [list(w["end"]) for w in want]
    assert gss.tolist() == [w["global_score"] for w in want]
    rc, scs, en, _, _, _ = call(0, cigars=False, gscore=False)
    assert rc == 0 and scs.tolist() == [w["score"] for w in want] and en.tolist() == [list(w["end"]) for w in want]


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
    for band in (0, 64, 1000):
        assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, band=band)) == UNSUPPORTED
    for cells in (LB.CELLS_H, LB.CELLS_TAB):
        assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, cells=cells)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, -1, 3)) == UNSUPPORTED  # g < 0
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, 2, -1)) == UNSUPPORTED  # h < 0
    # a table over the value range: (s + 2 G + 2 g)(m + n + 256) + (G - g) >= 2^28
    big = np.full((4, 4), 127)
    assert _status(lambda: _plan(LB, [1 << 20], [1 << 20], [0], [0], big, 1, 0)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], big, 1, 0)) == 0
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, how="mm")) == 0
    # 5-bit codes: the same rules
    S24 = W.table32()[:24, :24]
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S24, 2, 9, band=64)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S24, 2, 9, cells=LB.CELLS_H)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, [100], [100], [0], [0], S24, 2, 9)) == 0
    # a batch of equal-m pairs too small to fill the chip is still whole pairs per workgroup: mode 0, never split
    pl = _plan(LB, [1100] * 4, [1200] * 4, [0] * 4, [0] * 4, S, g, h, cells=LB.CELLS_NONE)
    assert pl.launch_info()["mode"] == "stripe" and pl.format_info()["tracking"] == "select"


def test_other_walkers_reject_the_plan(dev, LB):
    import torch

    A, B, alphabet, S, g, h, ref = _case("row65")
    pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h)
    ops = torch.empty(len(A) + len(B) + 2, dtype=torch.uint8, device=dev)
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    assert _status(lambda: pl.traceback_async(dDir, ops, info)) == UNSUPPORTED
    assert _status(lambda: pl.traceback_gotoh_async(dDir, ops, info)) == UNSUPPORTED
    # a score-only plan has no bytes to walk
    none = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, cells=LB.CELLS_NONE)
    assert _status(lambda: none.traceback_nw_async(dDir, ops, info)) == UNSUPPORTED


def test_walk_before_any_run(dev, LB):
    """A plan that has not run has no end cell: both walkers report MSA_ERR_ARG in the walk's status."""
    import torch

    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pl = _plan(LB, [70], [90], [0], [0], S, g, h)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    assert _status(lambda: pl.traceback_nw(dDir)) == ARG
    bp = _plan(LB, [70, 30], [90, 40], [0, 70], [0, 90], S, g, h)
    dDir = torch.zeros(bp.cells_elems, dtype=torch.uint8, device=dev)
    assert _status(lambda: bp.traceback_batch(dDir)) == ARG
