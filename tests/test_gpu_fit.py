"""Fit (query-in-reference) alignment (MSA_NW_FIT plans, msa_fit_align, msa_fit_align_batch) against the numpy
yardstick tests/fit_reference.py (itself checked against a triple-loop Gotoh, a brute force over every substring
and the global yardstick by test_fit_reference.py).

Every fill case checks, exactly (integer DP): the score, end = (m, end_j) and the plan's error word; bits 0-1 of
every interior direction byte, bit 2 where E is finite and bit 3 where F is finite; the walk's ops byte for byte,
its stop cell and the CIGAR; and the ops rescored on B[beg:end].  The shapes (fit_reference.SHAPES) are the smallest
at which each mechanism can fail: row m in the last lane of a stripe, in lane 0 of the next, as the only row; two
equal maxima on row m; the maximum at column n, at column 1, in a late phase of a long stripe; a query that
overhangs the reference's start or is longer than the reference; one pair over several workgroups; a batch."""
import ctypes as C
import functools

import numpy as np
import pytest

import fit_reference as FR
import nw_reference as R
import nw_scored_reference as RS

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG, CAPACITY = -5, -1, -8
MM_SETS = ["dna", "unit", "edit", "neg"]  # the score sets that are a match / mismatch pair


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _dev(x, alphabet, dev):
    import torch

    return torch.from_numpy(RS.codes(x, alphabet).astype(np.uint8)).to(dev)


@functools.lru_cache(maxsize=None)
def _case(name, set_name):
    """(A, B, alphabet, S, g, h, reference) of a named shape under a score set ("unit8": fit_reference.UNIT; the
    shape "eight": fit_reference.eight_symbols' own scoring), computed once and shared (never modified)."""
    if name == "eight":
        A, B, alphabet, S, g, h = FR.eight_symbols()
    else:
        alphabet, S, g, h = FR.UNIT if set_name == "unit8" else RS.SCORE_SETS[set_name]
        A, B = RS.set_input(set_name, *FR.SHAPES[name]())
    return A, B, alphabet, S, g, h, FR.fit_reference(A, B, alphabet, S, g, h)


def _plan(LB, ms, ns, a_offs, b_offs, S, g, h, cells=None, how="sub", band=-1):
    """An NW_FIT plan; how = "sub": the 8 x 8 table, "mm": S's match / mismatch through the description."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    kw = dict(sub=RS.sub8(S)) if how == "sub" else dict(match=int(S[0][0]), mismatch=int(S[0][1]))
    return Plan(LB.NW_FIT, LB.CELLS_DIR if cells is None else cells, ms, ns, a_offs, b_offs, gap_open=g + h,
                gap_extend=g, band=band, **kw)


def _fill(LB, dev, A, B, alphabet, S, g, h, how="sub"):
    import torch

    pl = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, how=how)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev), dDir)
    return pl, dDir


def _check(pl, dDir, A, B, alphabet, S, g, h, ref, pair=0):
    """Everything a fill test checks for one pair (see the module docstring)."""
    w = ref["w"]
    res = pl.results()[pair]
    assert res["score"] == ref["score"]
    assert tuple(res["end"]) == (len(A), ref["end_j"])
    assert res["status"] == 0
    assert pl.error() == 0
    assert pl.launch_info()["mode"] == "stripe"
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
    assert tb["cigar"] == FR.cigar_of(ref["ops"])
    assert FR.rescore(A, B, tb["stop"][1], res["end"][1], tb["ops"], alphabet, S, g, h) == ref["score"]
    return tb


# ---- 1. one pair (single = 1) ----------------------------------------------------------------------------------
CASES = [("q100_in_r700", s, "sub") for s in RS.SCORE_SETS] + [("q100_in_r700", s, "mm") for s in MM_SETS] + \
        [(n, "dna", "sub") for n in FR.SHAPES if n not in ("q100_in_r700", "q1000_r3000")] + \
        [("end_at_1", "unit8", "mm"), ("eight", "own", "sub")]


@pytest.mark.parametrize("name,set_name,how", CASES, ids=lambda x: x)
def test_fill_and_walk(dev, LB, name, set_name, how):
    A, B, alphabet, S, g, h, ref = _case(name, set_name)
    pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h, how=how)
    tb = _check(pl, dDir, A, B, alphabet, S, g, h, ref)
    if set_name == "dna" and name in FR.KNOWN:
        assert (ref["score"], ref["beg_j"], ref["end_j"], tb["cigar"]) == FR.KNOWN[name]
    if set_name == "unit8":
        assert (ref["score"], ref["beg_j"], ref["end_j"], tb["cigar"]) == FR.KNOWN_UNIT_END_AT_1
    if name == "eight":
        k = alphabet[7:8]
        assert k in A and k in B[ref["beg_j"]:ref["end_j"]]


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_one_pair_over_many_workgroups(dev, LB, cells):
    """1,000 rows: 16 stripes in 4 items, chained through granules; with direction bytes and score-only."""
    A, B, alphabet, S, g, h, ref = _case("q1000_r3000", "dna")
    if cells == "dir":
        pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h)
        assert pl.single and pl.launch_info()["items"] == 4
        _check(pl, dDir, A, B, alphabet, S, g, h, ref)
        return
    pl = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, cells=LB.CELLS_NONE)
    assert pl.cells_elems == 0 and pl.launch_info()["mode"] == "stripe" and pl.launch_info()["items"] == 4
    pl.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev))
    res = pl.results()[0]
    assert (res["score"], tuple(res["end"]), res["status"]) == (ref["score"], (len(A), ref["end_j"]), 0)
    assert pl.error() == 0


# ---- 2. a batch plan (single = 0) --------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", ["dir", "none"])
def test_batch_plan(dev, LB, cells):
    import torch

    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = FR.batch_pairs()
    ms, ns = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    assert (ms, ns) == (FR.BATCH_MS, FR.BATCH_NS)
    a_offs = np.concatenate(([0], np.cumsum(ms)[:-1]))
    b_offs = np.concatenate(([0], np.cumsum(ns)[:-1]))
    dA = _dev(b"".join(a for a, _ in pairs), alphabet, dev)
    dB = _dev(b"".join(b for _, b in pairs), alphabet, dev)
    refs = [FR.fit_reference(a, b, alphabet, S, g, h) for a, b in pairs]
    if cells == "none":
        pl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h, cells=LB.CELLS_NONE)
        pl.run(dA, dB)
        for res, ref, m in zip(pl.results(), refs, ms):
            assert (res["score"], tuple(res["end"]), res["status"]) == (ref["score"], (m, ref["end_j"]), 0)
        assert pl.error() == 0 and pl.launch_info()["mode"] == "stripe"
        return
    pl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h)
    assert not pl.single
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(dA, dB, dDir)
    singles = [_check(pl, dDir, a, b, alphabet, S, g, h, ref, pair=k) for k, ((a, b), ref) in enumerate(zip(pairs, refs))]
    for one, tb in zip(singles, pl.traceback_batch(dDir)):
        assert (tb["ops"], tb["stop"], tb["cigar"]) == (one["ops"], one["stop"], one["cigar"])


# ---- 3. the host entries ---------------------------------------------------------------------------------------
DNA_KW = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2)


def _want(ref):
    return dict(score=ref["score"], beg=ref["beg_j"], end=ref["end_j"], cigar=FR.cigar_of(ref["ops"]))


@pytest.mark.parametrize("name", ["q100_in_r700", "overhang_25I", "end_at_1"])
def test_api_fit_align(dev, name):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, alphabet, S, g, h, ref = _case(name, "dna")
    r = api.fit_align(A, B, **DNA_KW)
    assert r == _want(ref)
    r0 = api.fit_align(A, B, traceback=False, **DNA_KW)
    assert r0 == dict(score=ref["score"], beg=None, end=ref["end_j"])
    if r["end"] > r["beg"]:
        assert api.nw_align(A, B[r["beg"]:r["end"]], traceback=False, **DNA_KW)["score"] == r["score"]
    # alphabet + matrix reach the same result
    assert api.fit_align(A, B, gap_open=g + h, gap_extend=g, alphabet=alphabet, matrix=S) == r


@functools.lru_cache(maxsize=None)
def _shared_reference_batch():
    """Six queries (edited pieces of the reference, a random one, a reversed one) against one 2,000-symbol
    reference, with the yardstick's answers."""
    rng = np.random.default_rng(41)
    ref = R.rs(rng, 2000)
    qs = [FR.edited(rng, ref[at:at + m]) for at, m in ((0, 64), (700, 130), (1935, 65), (1200, 300))]
    qs += [R.rs(rng, 90), ref[400:480][::-1]]
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    return qs, ref, [FR.fit_reference(q, ref, alphabet, S, g, h) for q in qs]


def test_api_fit_align_batch_shared_reference(dev):
    from cse305_parallel_sequence_alignment_amd import api

    qs, ref, want = _shared_reference_batch()
    got = api.fit_align_batch(qs, ref, **DNA_KW)
    assert got == [_want(w) for w in want]
    assert (got[0]["beg"], got[0]["end"]) == (0, 64) and (got[2]["beg"], got[2]["end"]) == (1935, 2000)
    for q, r in zip(qs, got):
        assert api.nw_align(q, ref[r["beg"]:r["end"]], traceback=False, **DNA_KW)["score"] == r["score"]
    got0 = api.fit_align_batch(qs, ref, traceback=False, **DNA_KW)
    assert got0 == [dict(score=w["score"], beg=None, end=w["end_j"]) for w in want]


def test_api_fit_align_batch_list_of_references(dev):
    from cse305_parallel_sequence_alignment_amd import api

    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = FR.batch_pairs()
    got = api.fit_align_batch([a for a, _ in pairs], [b for _, b in pairs], **DNA_KW)
    assert got == [_want(FR.fit_reference(a, b, alphabet, S, g, h)) for a, b in pairs]


def test_batch_entry_capacity(dev, LB):
    """A cigars buffer too small: MSA_ERR_CAPACITY with the needed size in cigar_off[n_pairs]; that size suffices."""
    qs, ref, want = _shared_reference_batch()
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    k = len(qs)
    A = b"".join(qs)
    m = np.array([len(q) for q in qs], dtype=np.int64)
    a_off = np.concatenate(([0], np.cumsum(m)[:-1])).astype(np.int64)
    n = np.full(k, len(ref), dtype=np.int64)
    b_off = np.zeros(k, dtype=np.int64)
    sub = np.ascontiguousarray(S, dtype=np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(cap):
        sc = np.zeros(k, dtype=np.int32)
        be = np.zeros((k, 2), dtype=np.int64)
        coff = np.zeros(k + 1, dtype=np.int64)
        cig = C.create_string_buffer(max(cap, 1))
        rc = LB.lib().msa_fit_align_batch(A, len(A), ref, len(ref), k, p(a_off), p(m), p(b_off), p(n), alphabet,
                                          len(alphabet), p(sub), g + h, g, p(sc), p(be), cig, cap, p(coff))
        return rc, sc, be, coff, cig

    cigars = [FR.cigar_of(w["ops"]) for w in want]
    need = sum(len(c) + 1 for c in cigars)
    rc, _, _, coff, _ = call(need - 1)
    assert rc == CAPACITY and int(coff[k]) == need
    rc, sc, be, coff, cig = call(need)
    assert rc == 0
    assert [cig.raw[coff[q]:coff[q + 1] - 1].decode() for q in range(k)] == cigars
    assert sc.tolist() == [w["score"] for w in want]
    assert be.tolist() == [[w["beg_j"], w["end_j"]] for w in want]


def test_single_entry_capacity(dev, LB):
    A, B, alphabet, S, g, h, ref = _case("overhang_25I", "dna")
    sub = np.ascontiguousarray(S, dtype=np.int8)
    sc, bj, ej = C.c_int32(), C.c_int64(), C.c_int64()
    cig = C.create_string_buffer(16)
    f = LB.lib().msa_fit_align
    args = (A, len(A), B, len(B), alphabet, len(alphabet), sub.ctypes.data_as(C.c_void_p), g + h, g, C.byref(sc),
            C.byref(bj), C.byref(ej), cig)
    assert f(*args, len("25I105M")) == CAPACITY  # (no room for the NUL)
    assert f(*args, len("25I105M") + 1) == 0
    assert (cig.value, sc.value, bj.value, ej.value) == (b"25I105M", 157, 0, 105)


# ---- 4. plan creation --------------------------------------------------------------------------------------------
def _create_status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_plan_creation_errors(dev, LB):
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    for band in (0, 64, 1000):
        assert _create_status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, band=band)) == UNSUPPORTED
    for cells in (LB.CELLS_H, LB.CELLS_TAB):
        assert _create_status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, cells=cells)) == UNSUPPORTED
    assert _create_status(lambda: _plan(LB, [100], [100], [0], [0], S, -1, 3)) == UNSUPPORTED  # g < 0
    assert _create_status(lambda: _plan(LB, [100], [100], [0], [0], S, 2, -1)) == UNSUPPORTED  # h < 0
    # a table over the value range: (s + 2 G + 2 g)(m + n + 256) + (G - g) >= 2^28
    wide = np.full((4, 4), 127)
    assert _create_status(lambda: _plan(LB, [1 << 20], [1 << 20], [0], [0], wide, 1, 0)) == UNSUPPORTED
    assert _create_status(lambda: _plan(LB, [100], [100], [0], [0], wide, 1, 0)) == 0
    assert _create_status(lambda: _plan(LB, [100], [100], [0], [0], S, g, h, how="mm")) == 0


def test_other_walkers_reject_the_plan(dev, LB):
    import torch

    A, B, alphabet, S, g, h, ref = _case("m65_r300", "dna")
    pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h)
    ops = torch.empty(len(A) + len(B) + 2, dtype=torch.uint8, device=dev)
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    assert _create_status(lambda: pl.traceback_async(dDir, ops, info)) == UNSUPPORTED
    assert _create_status(lambda: pl.traceback_gotoh_async(dDir, ops, info)) == UNSUPPORTED
    # a score-only plan has no bytes to walk
    none = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, cells=LB.CELLS_NONE)
    assert _create_status(lambda: none.traceback_nw_async(dDir, ops, info)) == UNSUPPORTED

