"""Overlap (suffix-prefix) alignment (MSA_NW_OVERLAP plans, msa_overlap_align, msa_overlap_align_batch and their *32
twins) against the numpy yardstick tests/overlap_reference.py (itself checked against a triple-loop Gotoh and the
definition by exhaustion in test_overlap_reference.py).

Every fill case checks, exactly (integer DP): the score, the end cell and the plan's error word; bits 0-1 of every
interior direction byte, bit 2 where E is finite and bit 3 where F is finite; the walk's ops byte for byte, its stop
cell (the alignment's begin) and the CIGAR; and the ops rescored on A[a_beg:a_end] / B[b_beg:b_end].  The shapes
(overlap_reference.SHAPES) are the smallest at which each mechanism can fail: an end cell on the last row, on the
last column in the first, a middle or the last stripe, in both at once (the corner, a tie); equal column candidates
in two stripes; the empty overlap; row m in the last lane of a stripe, lane 0 of the next, the only row; a single
column; n < 64; column n in the last of many phases; one pair over several workgroups; a batch; 8 and 24 symbols."""
import ctypes as C
import functools

import numpy as np
import pytest

import fit_reference as FR
import nw_reference as R
import nw_scored_reference as RS
import overlap_reference as OR
import wide_reference as W

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG, CAPACITY = -5, -1, -8


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _dev(x, alphabet, dev):
    import torch

    return torch.from_numpy(OR.codes(x, alphabet).astype(np.uint8)).to(dev)


@functools.lru_cache(maxsize=None)
def _case(name, set_name="dna"):
    """(A, B, alphabet, S, g, h, reference) of a named shape ("eight" / "protein", "protein1", "protein2": their own
    scoring; set_name "unit8": fit_reference.UNIT), computed once and shared (never modified)."""
    if name == "eight":
        A, B, alphabet, S, g, h = OR.eight_symbols()
    elif name.startswith("protein"):
        A, B, alphabet, S, g, h = OR.protein32(int(name[7:] or 0))
    else:
        alphabet, S, g, h = OR.UNIT if set_name == "unit8" else RS.SCORE_SETS[set_name]
        A, B = OR.SHAPES[name]()
    return A, B, alphabet, S, g, h, OR.overlap_reference(A, B, alphabet, S, g, h)


def _plan(LB, ms, ns, a_offs, b_offs, S, g, h, cells=None, how="sub", band=-1, alg=None):
    """An NW_OVERLAP plan; how = "sub": the 8 x 8 table (32 x 32 for more than 8 symbols), "mm": S's match / mismatch
    through the description."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    if how == "mm":
        kw = dict(match=int(S[0][0]), mismatch=int(S[0][1]))
    else:
        kw = dict(sub=W.sub32(S) if len(S) > 8 else RS.sub8(S))
    return Plan(LB.NW_OVERLAP if alg is None else alg, LB.CELLS_DIR if cells is None else cells, ms, ns, a_offs, b_offs,
                gap_open=g + h, gap_extend=g, band=band, **kw)


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
    assert tuple(res["end"]) == ref["end"]
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
    assert tb["stop"] == ref["beg"]
    assert tb["cigar"] == OR.cigar_of(ref["ops"])
    got_res = dict(beg=tb["stop"], end=tuple(res["end"]))
    assert OR.borders_ok(got_res, len(A), len(B))
    assert OR.rescore(A, B, tb["stop"], tuple(res["end"]), tb["ops"], alphabet, S, g, h) == ref["score"]
    return tb


def _known(ref, cigar):
    return (ref["score"], ref["beg"], ref["end"], cigar)


# ---- 1. one pair (single = 1) ----------------------------------------------------------------------------------
CASES = [(n, "dna", "sub") for n in OR.SHAPES if n != "single_1000x3000"] + \
        [("dovetail_ab", "dna", "mm"), ("dovetail_ba", "asym", "sub"), ("empty", "unit8", "mm"),
         ("eight", "own", "sub"), ("protein", "own", "sub")]


@pytest.mark.parametrize("name,set_name,how", CASES, ids=lambda x: x)
def test_fill_and_walk(dev, LB, name, set_name, how):
    A, B, alphabet, S, g, h, ref = _case(name, set_name)
    pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h, how=how)
    assert pl.format_info()["codes"] == (32 if len(alphabet) > 8 else 8)
    tb = _check(pl, dDir, A, B, alphabet, S, g, h, ref)
    if set_name == "dna" and name in OR.KNOWN:
        assert _known(ref, tb["cigar"]) == OR.KNOWN[name]
    if set_name == "unit8":
        assert _known(ref, tb["cigar"]) == OR.KNOWN_UNIT_EMPTY
    if name == "eight":
        k = alphabet[7:8]
        assert k in A[ref["beg"][0]:ref["end"][0]] and k in B[ref["beg"][1]:ref["end"][1]]
    # a score-only plan (no direction bytes) reaches the same score and end cell
    none = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, cells=LB.CELLS_NONE, how=how)
    assert none.cells_elems == 0 and none.launch_info()["mode"] == "stripe"
    none.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev))
    res = none.results()[0]
    assert (res["score"], tuple(res["end"]), res["status"]) == (ref["score"], ref["end"], 0)
    assert none.error() == 0


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_one_pair_over_many_workgroups(dev, LB, cells):
    """1,000 rows: 16 stripes in 4 items, chained through granules; the end cell is a column candidate of the third."""
    A, B, alphabet, S, g, h, ref = _case("single_1000x3000")
    assert ref["end"] == (700, 3000) and ref["beg"] == (0, 2300)
    if cells == "dir":
        pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h)
        assert pl.single and pl.launch_info()["items"] == 4
        _check(pl, dDir, A, B, alphabet, S, g, h, ref)
        return
    pl = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, cells=LB.CELLS_NONE)
    assert pl.cells_elems == 0 and pl.launch_info()["mode"] == "stripe" and pl.launch_info()["items"] == 4
    pl.run(_dev(A, alphabet, dev), _dev(B, alphabet, dev))
    res = pl.results()[0]
    assert (res["score"], tuple(res["end"]), res["status"]) == (ref["score"], ref["end"], 0)
    assert pl.error() == 0


# ---- 2. a batch plan (single = 0) --------------------------------------------------------------------------------
def _offsets(seqs):
    return np.concatenate(([0], np.cumsum([len(s) for s in seqs])[:-1]))


def _batch_plan(dev, LB, pairs, alphabet, S, g, h, cells):
    import torch

    ms, ns = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    dA = _dev(b"".join(a for a, _ in pairs), alphabet, dev)
    dB = _dev(b"".join(b for _, b in pairs), alphabet, dev)
    refs = [OR.overlap_reference(a, b, alphabet, S, g, h) for a, b in pairs]
    a_offs, b_offs = _offsets([a for a, _ in pairs]), _offsets([b for _, b in pairs])
    if cells == "none":
        pl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h, cells=LB.CELLS_NONE)
        pl.run(dA, dB)
        for res, ref in zip(pl.results(), refs):
            assert (res["score"], tuple(res["end"]), res["status"]) == (ref["score"], ref["end"], 0)
        assert pl.error() == 0 and pl.launch_info()["mode"] == "stripe"
        return
    pl = _plan(LB, ms, ns, a_offs, b_offs, S, g, h)
    assert not pl.single
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(dA, dB, dDir)
    singles = [_check(pl, dDir, a, b, alphabet, S, g, h, ref, pair=k) for k, ((a, b), ref) in enumerate(zip(pairs, refs))]
    batch = pl.traceback_batch(dDir)  # one launch for every pair
    for one, tb, ref in zip(singles, batch, refs):
        assert (tb["ops"], tb["stop"], tb["cigar"]) == (one["ops"], one["stop"], one["cigar"])
        if ref["score"] == 0:  # the empty overlap: no walk
            assert (tb["ops"], tb["stop"]) == (b"", ref["end"])


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_batch_plan(dev, LB, cells):
    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = OR.batch_pairs()
    assert ([len(a) for a, _ in pairs], [len(b) for _, b in pairs]) == (OR.BATCH_MS, OR.BATCH_NS)
    _batch_plan(dev, LB, pairs, alphabet, S, g, h, cells)


@pytest.mark.parametrize("cells", ["dir", "none"])
def test_batch_plan_protein32(dev, LB, cells):
    cases = [_case(f"protein{k}") for k in range(3)]
    _, _, alphabet, S, g, h, _ = cases[0]
    _batch_plan(dev, LB, [(c[0], c[1]) for c in cases], alphabet, S, g, h, cells)


# ---- 3. the host entries ---------------------------------------------------------------------------------------
DNA_KW = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2)


def _want(ref, traceback=True):
    (bi, bj), (ei, ej) = ref["beg"], ref["end"]
    r = dict(score=ref["score"], a_beg=bi if traceback else None, a_end=ei, b_beg=bj if traceback else None, b_end=ej)
    if traceback:
        r["cigar"] = OR.cigar_of(ref["ops"])
    return r


@pytest.mark.parametrize("name", ["dovetail_ab", "dovetail_ba", "b_in_a", "empty", "tie_row_col"])
def test_api_overlap_align(dev, name):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, alphabet, S, g, h, ref = _case(name)
    r = api.overlap_align(A, B, **DNA_KW)
    assert r == _want(ref)
    assert api.overlap_align(A, B, traceback=False, **DNA_KW) == _want(ref, False)
    if r["score"] > 0:
        piece = api.nw_align(A[r["a_beg"]:r["a_end"]], B[r["b_beg"]:r["b_end"]], traceback=False, **DNA_KW)
        assert piece["score"] == r["score"]
    # alphabet + matrix reach the same result
    assert api.overlap_align(A, B, gap_open=g + h, gap_extend=g, alphabet=alphabet, matrix=S) == r


def test_api_overlap_align_32_symbols(dev):
    from cse305_parallel_sequence_alignment_amd import api

    cases = [_case(f"protein{k}") for k in range(3)]
    _, _, alphabet, S, g, h, _ = cases[0]
    kw = dict(gap_open=g + h, gap_extend=g, alphabet=alphabet, matrix=S, max_symbols=32)
    assert api.overlap_align(cases[0][0], cases[0][1], **kw) == _want(cases[0][6])
    got = api.overlap_align_batch([c[0] for c in cases], [c[1] for c in cases], **kw)
    assert got == [_want(c[6]) for c in cases]


def test_api_overlap_align_batch(dev):
    from cse305_parallel_sequence_alignment_amd import api

    alphabet, S, g, h = RS.SCORE_SETS["dna"]
    pairs = OR.batch_pairs()
    want = [OR.overlap_reference(a, b, alphabet, S, g, h) for a, b in pairs]
    got = api.overlap_align_batch([a for a, _ in pairs], [b for _, b in pairs], **DNA_KW)
    assert got == [_want(w) for w in want]
    got0 = api.overlap_align_batch([a for a, _ in pairs], [b for _, b in pairs], traceback=False, **DNA_KW)
    assert got0 == [_want(w, False) for w in want]
    # one B shared by every pair
    As, ref_b = OR.shared_b_batch()
    want = [OR.overlap_reference(a, ref_b, alphabet, S, g, h) for a in As]
    assert api.overlap_align_batch(As, ref_b, **DNA_KW) == [_want(w) for w in want]


def test_entry_capacity(dev, LB):
    """A cigar buffer too small: MSA_ERR_CAPACITY (the batch: with the needed size in cigar_off[n_pairs]; that size
    suffices), the score and the cells still reported."""
    A, B, alphabet, S, g, h, ref = _case("dovetail_ab")
    sub = np.ascontiguousarray(S, dtype=np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    sc = C.c_int32()
    beg, end = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    cig = C.create_string_buffer(16)
    f = LB.lib().msa_overlap_align
    args = (A, len(A), B, len(B), alphabet, len(alphabet), p(sub), g + h, g, C.byref(sc), p(beg), p(end), cig)
    assert f(*args, len("80M")) == CAPACITY  # (no room for the NUL)
    assert f(*args, len("80M") + 1) == 0
    assert (cig.value, sc.value, beg.tolist(), end.tolist()) == (b"80M", 160, [120, 0], [200, 80])
    # score only through the C entry: the begin cell is {-1, -1}
    assert f(*args[:-1], None, 0) == 0
    assert (sc.value, beg.tolist(), end.tolist()) == (160, [-1, -1], [200, 80])

    pairs = OR.batch_pairs()
    want = [OR.overlap_reference(a, b, alphabet, S, g, h) for a, b in pairs]
    k = len(pairs)
    Ab, Bb = b"".join(a for a, _ in pairs), b"".join(b for _, b in pairs)
    m = np.array(OR.BATCH_MS, dtype=np.int64)
    n = np.array(OR.BATCH_NS, dtype=np.int64)
    a_off, b_off = _offsets([a for a, _ in pairs]).astype(np.int64), _offsets([b for _, b in pairs]).astype(np.int64)

    def call(cap):
        scs = np.zeros(k, dtype=np.int32)
        bg, en = np.zeros((k, 2), dtype=np.int64), np.zeros((k, 2), dtype=np.int64)
        coff = np.zeros(k + 1, dtype=np.int64)
        cg = C.create_string_buffer(max(cap, 1))
        rc = LB.lib().msa_overlap_align_batch(Ab, len(Ab), Bb, len(Bb), k, p(a_off), p(m), p(b_off), p(n), alphabet,
                                              len(alphabet), p(sub), g + h, g, p(scs), p(bg), p(en), cg, cap, p(coff))
        return rc, scs, bg, en, coff, cg

    cigars = [OR.cigar_of(w["ops"]) for w in want]
    need = sum(len(c) + 1 for c in cigars)
    rc, _, _, _, coff, _ = call(need - 1)
    assert rc == CAPACITY and int(coff[k]) == need
    rc, scs, bg, en, coff, cg = call(need)
    assert rc == 0
    assert [cg.raw[coff[q]:coff[q + 1] - 1].decode() for q in range(k)] == cigars
    assert scs.tolist() == [w["score"] for w in want]
    assert bg.tolist() == [list(w["beg"]) for w in want] and en.tolist() == [list(w["end"]) for w in want]


# ---- 4. plan creation, the other walkers, the neighbouring algorithms ------------------------------------------------
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
    assert pl.launch_info()["mode"] == "stripe"


def test_other_walkers_reject_the_plan(dev, LB):
    import torch

    A, B, alphabet, S, g, h, ref = _case("m65")
    pl, dDir = _fill(LB, dev, A, B, alphabet, S, g, h)
    ops = torch.empty(len(A) + len(B) + 2, dtype=torch.uint8, device=dev)
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    assert _status(lambda: pl.traceback_async(dDir, ops, info)) == UNSUPPORTED
    assert _status(lambda: pl.traceback_gotoh_async(dDir, ops, info)) == UNSUPPORTED
    # a score-only plan has no bytes to walk
    none = _plan(LB, [len(A)], [len(B)], [0], [0], S, g, h, cells=LB.CELLS_NONE)
    assert _status(lambda: none.traceback_nw_async(dDir, ops, info)) == UNSUPPORTED


def test_fit_and_global_keep_their_left_border(dev):
    """The zero left border belongs to the overlap kernels alone: on the same pair the fit and the global entries
    still return what their own restatements give."""
    from cse305_parallel_sequence_alignment_amd import api

    A, B, alphabet, S, g, h, ref = _case("dovetail_ab")
    fit = FR.fit_reference(A, B, alphabet, S, g, h)
    assert api.fit_align(A, B, **DNA_KW) == dict(score=fit["score"], beg=fit["beg_j"], end=fit["end_j"],
                                                 cigar=FR.cigar_of(fit["ops"]))
    glob = RS.nw_scored_reference(A, B, alphabet, S, g, h)
    assert api.nw_align(A, B, **DNA_KW) == dict(score=glob["score"], cigar=RS.cigar_of(glob["ops"]))
    assert fit["score"] != ref["score"] and glob["score"] != ref["score"]  # (the three algorithms differ here)
