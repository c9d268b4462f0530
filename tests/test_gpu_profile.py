"""Alignment against a position-specific score profile (msa_plan_create_profile: MSA_SW_SCORED, MSA_NW_SCORED and
MSA_NW_FIT plans whose rows load their own 32 scores; the walkers on them; msa_profile_align / _batch;
api.profile_align / profile_align_batch) against the yardstick tests/profile_reference.py -- the table yardsticks with
the row lookup replaced by the row index --, which test_profile_reference.py checks against those yardsticks and
against a plain-Python DP, together with what every input here is meant to be.

Everything is exact integer equality.  A fill test checks the score, the end cell, the status, the plan's error word,
the launch mode, bits 0-3 of every interior direction byte (without a band every interior E and F is finite, so all four
bits are defined in the global modes too), the walk's ops, start / stop cell and CIGAR, and the ops rescored under the
profile.  Shapes are the smallest at which each mechanism runs: six stripes in two items of four waves (the granule
hand-off), ten stripes on an eight-wave workgroup (the wrap link), one row, an exact stripe, one row more."""
import ctypes as C
import functools

import numpy as np
import pytest

import nw_reference as R
import profile_reference as PR
import wide_reference as W

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG, CAPACITY = -5, -1, -8
MODES = PR.MODES
GO, GE = PR.GO, PR.GE


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _alg(LB, mode):
    return {"local": LB.SW_SCORED, "global": LB.NW_SCORED, "fit": LB.NW_FIT}[mode]


def _dev(x, alphabet, dev):
    import torch

    return torch.from_numpy(W.codes32(x, alphabet).astype(np.uint8)).to(dev)


def _offsets(seqs):
    return np.concatenate(([0], np.cumsum([len(s) for s in seqs])[:-1]))


def _plan(LB, mode, P32, rows, Bs, cells=None, single=None, go=GO, ge=GE, alg=None, **kw):
    """A profile plan: pair k = profile rows rows[k] = (a_off, m) against Bs[k]."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    return Plan(_alg(LB, mode) if alg is None else alg, LB.CELLS_DIR if cells is None else cells,
                [m for _, m in rows], [len(b) for b in Bs], [a for a, _ in rows], _offsets(Bs), gap_open=go,
                gap_extend=ge, single=single, profile=P32, **kw)


def _run(LB, dev, mode, P, rows, Bs, **kw):
    import torch

    pl = _plan(LB, mode, PR.pad32(P), rows, Bs, **kw)
    assert pl.profile and pl.format_info()["profile"] and pl.format_info()["codes"] == 32
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev) if pl.cells_elems else None
    pl.run(None, _dev(b"".join(Bs), PR.alphabet_of(mode), dev), dDir)
    return pl, dDir


def _end(mode, ref, m, n):
    """The end cell a plan reports for a yardstick dictionary."""
    return ref["end"] if mode == "local" else (m, n) if mode == "global" else (m, ref["end_j"])


def _bytes(pl, dDir, pair):
    return pl.deskew_dir(dDir.cpu().numpy(), pair, pl.stripe_meta())


def _check(mode, pl, dDir, P, B, ref, pair=0, go=GO, ge=GE):
    """Everything a fill test checks for one pair (see the module docstring); P = the pair's own rows.  Returns the
    single walker's result."""
    al = PR.alphabet_of(mode)
    m, n = len(P), len(B)
    res = pl.results()[pair]
    assert (res["score"], tuple(res["end"]), res["status"]) == (ref["score"], _end(mode, ref, m, n), 0)
    assert pl.error() == 0
    assert pl.launch_info()["mode"] == "stripe"
    got = _bytes(pl, dDir, pair)
    if mode == "local":
        bad = (got[1:, 1:] & 15) != (ref["byte"][1:, 1:] & 15)
        assert not bad.any(), ("bits 0-3", int(bad.sum()), (np.argwhere(bad)[:4] + 1).tolist())
        tb = pl.traceback(dDir, pair)
        assert (tb["ops"], tb["beg"], tb["cigar"]) == (ref["ops"], ref["beg"], ref["cigar"])
        if ref["score"] > 0:
            assert PR.rescore(mode, P, B, al, tb["ops"], beg=tb["beg"], go=go, ge=ge) == (ref["score"], ref["end"])
        return tb
    v = ref["valid"]
    assert (ref["efin"] | ~v).all() and (ref["ffin"] | ~v).all()  # all four bits are defined everywhere inside
    bad = v & (((R.to_band(got, ref["w"]) ^ ref["byte"]) & 15) != 0)
    assert not bad.any(), ("bits 0-3", int(bad.sum()), np.argwhere(bad)[:4].tolist())
    tb = pl.traceback_nw(dDir, pair)
    assert (tb["ops"], tb["stop"], tb["cigar"]) == (ref["ops"], ref["stop"], W.cigar_of(ref["ops"]))
    if mode == "global":
        assert PR.rescore(mode, P, B, al, tb["ops"], go=go, ge=ge) == ref["score"]
    else:
        assert tb["stop"][1] == ref["beg_j"]
        assert PR.rescore(mode, P, B, al, tb["ops"], span=(tb["stop"][1], res["end"][1]), go=go, ge=ge) == ref["score"]
    return tb


def _walk_key(mode, tb):
    return (tb["ops"], tb["beg"] if mode == "local" else tb["stop"], tb["cigar"])


# ---- 1. a profile made from a table is that table's plan ---------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_table_equivalence(dev, LB, mode):
    """330 x 300: six stripes in two items of four waves.  The profile whose row r is row code(A_r) of the table, and
    the 32-code table plan of the same pair: the same results, bytes and walks, and both the yardstick's."""
    import torch
    from cse305_parallel_sequence_alignment_amd import api
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    al, T = PR.alphabet_of(mode), PR.table_of(mode)
    A, B = PR.table_case(mode)
    P = api.profile_from_matrix(A, al, T)
    ref = PR.profile_reference(mode, P, B, al)
    pp, dP = _run(LB, dev, mode, P, [(0, 330)], [B], single=True)
    assert pp.single and pp.launch_info()["items"] == 2
    tp = _check(mode, pp, dP, P, B, ref)
    pt = Plan(_alg(LB, mode), LB.CELLS_DIR, [330], [300], [0], [0], gap_open=GO, gap_extend=GE, single=True,
              sub=W.sub32(T))
    assert not pt.profile and not pt.format_info()["profile"] and pt.format_info()["codes"] == 32
    dT = torch.zeros(pt.cells_elems, dtype=torch.uint8, device=dev)
    pt.run(_dev(A, al, dev), _dev(B, al, dev), dT)
    tt = _check(mode, pt, dT, P, B, ref)
    key = lambda r: (r["score"], r["status"], tuple(r["end"])) + (tuple(r["fin"]) if mode != "local" else ())  # noqa: E731
    assert [key(r) for r in pp.results()] == [key(r) for r in pt.results()]
    assert pp.launch_info() == dict(pt.launch_info(), lds_bytes=pt.launch_info()["lds_bytes"] - 1024)  # no LDS table
    assert pp.format_info() == dict(pt.format_info(), profile=True)
    assert (pp.stripe_meta()[:, :2] == pt.stripe_meta()[:, :2]).all() and pp.cells_elems == pt.cells_elems
    assert ((_bytes(pp, dP, 0) ^ _bytes(pt, dT, 0))[1:, 1:] & 15 == 0).all()
    assert _walk_key(mode, tp) == _walk_key(mode, tt)


# ---- 2. rows that no table has -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_position_specific_rows(dev, LB, mode):
    """330 rows, each its own; a run of them with the preferred column moved: row r is scored by profile row r."""
    P, B = PR.specific_case(mode)
    ref = PR.profile_reference(mode, P, B, PR.alphabet_of(mode))
    for single in (True, False):
        pl, dDir = _run(LB, dev, mode, P, [(0, 330)], [B], single=single)
        _check(mode, pl, dDir, P, B, ref)


# ---- 3. batches --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_refs(mode):
    P, Bs = PR.batch_case(mode)
    return [PR.profile_reference(mode, P, b, PR.alphabet_of(mode)) for b in Bs]


@pytest.mark.parametrize("cells", ["dir", "none"])
@pytest.mark.parametrize("mode", MODES)
def test_shared_profile_batch(dev, LB, mode, cells):
    """One 580-row profile (ten stripes on eight waves: the wrap link), a_off all zero, against ragged sequences."""
    P, Bs = PR.batch_case(mode)
    refs = _batch_refs(mode)
    rows = [(0, len(P))] * len(Bs)
    m = len(P)
    if cells == "none":
        pl, _ = _run(LB, dev, mode, P, rows, Bs, cells=LB.CELLS_NONE)
        assert pl.cells_elems == 0 and not pl.single
        want = [(r["score"], _end(mode, r, m, len(b))) for r, b in zip(refs, Bs)]
        assert [(r["score"], tuple(r["end"])) for r in pl.results()] == want
        assert pl.error() == 0 and pl.launch_info()["mode"] == "stripe"
        return
    pl, dDir = _run(LB, dev, mode, P, rows, Bs)
    assert not pl.single
    singles = [_check(mode, pl, dDir, P, b, ref, pair=p) for p, (b, ref) in enumerate(zip(Bs, refs))]
    batch = pl.traceback_batch(dDir)
    for one, tb in zip(singles, batch):
        assert _walk_key(mode, tb) == _walk_key(mode, one)
    if mode == "local":
        assert refs[4]["score"] == 0 and batch[4]["ops"] == b""  # the unrelated sequence: nothing to walk


@pytest.mark.parametrize("mode", MODES)
def test_slices_of_one_profile(dev, LB, mode):
    """(a_off, m) = (0, 580), (37, 64), (515, 65): the last slice ends exactly at the profile's last row."""
    P, Bs = PR.slice_case(mode)
    assert PR.SLICES[-1][0] + PR.SLICES[-1][1] == len(P)
    pl, dDir = _run(LB, dev, mode, P, PR.SLICES, Bs)
    walks = pl.traceback_batch(dDir)
    for p, ((a, m), B) in enumerate(zip(PR.SLICES, Bs)):
        ref = PR.profile_reference(mode, P[a:a + m], B, PR.alphabet_of(mode))
        one = _check(mode, pl, dDir, P[a:a + m], B, ref, pair=p)
        assert _walk_key(mode, walks[p]) == _walk_key(mode, one)
    # ... and the last slice alone, as a single-pair launch
    a, m = PR.SLICES[-1]
    pl, dDir = _run(LB, dev, mode, P, [(a, m)], Bs[-1:], single=True)
    _check(mode, pl, dDir, P[a:], Bs[-1], PR.profile_reference(mode, P[a:], Bs[-1], PR.alphabet_of(mode)))


# ---- 4. edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", PR.EDGE_MS)
@pytest.mark.parametrize("mode", MODES)
def test_edges(dev, LB, mode, m):
    P, B = PR.edge_case(mode, m)
    ref = PR.profile_reference(mode, P, B, PR.alphabet_of(mode))
    for single in (True, False):
        pl, dDir = _run(LB, dev, mode, P, [(0, m)], [B], single=single)
        _check(mode, pl, dDir, P, B, ref)


# ---- 5. the sentinel column --------------------------------------------------------------------------------------
def test_all_positive_profile_scores_the_sentinel(dev, LB):
    """Every entry >= 1 and the caller's own column 31 (ignored by contract) 127: were it used for the virtual columns
    left of column 1 and right of column n, H would grow there and the scores change."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan
    import torch

    P, Bs = PR.all_positive_case()
    P32 = PR.pad32(P)
    P32[:, 31] = 127
    for B in Bs:
        ref = PR.profile_reference("local", P, B, PR.AL31)
        # what a used sentinel column would give: B between two runs of a symbol that scores 127 in every row
        ext = np.concatenate((P, np.full((len(P), 1), 127)), axis=1)
        wrong = PR.profile_reference("local", ext, b"e" * 64 + B + b"e" * 64, PR.AL32)
        assert wrong["score"] != ref["score"]
        for single in (True, False):
            pl = Plan(LB.SW_SCORED, LB.CELLS_DIR, [len(P)], [len(B)], [0], [0], gap_open=GO, gap_extend=GE,
                      single=single, profile=P32)
            dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
            pl.run(None, _dev(B, PR.AL31, dev), dDir)
            _check("local", pl, dDir, P, B, ref)


# ---- 6. the end-cell formats at their bound ----------------------------------------------------------------------
@pytest.mark.parametrize("L,tracking,score", [(516, "key", 65532), (517, "select", 65659)])
def test_end_cell_format_bound(dev, LB, L, tracking, score):
    """smax min(m, n) = 127 L < 65536 packs the first maximum's step with the value; one row more: compare-select."""
    P, B = PR.self127(L)
    ref = PR.profile_reference("local", P, B, PR.AL31)
    assert (ref["score"], ref["end"]) == (score, (L, L))
    for single in (True, False):
        pl, dDir = _run(LB, dev, "local", P, [(0, L)], [B], single=single)
        assert pl.format_info()["tracking"] == tracking
        _check("local", pl, dDir, P, B, ref)


# ---- 7. extreme bytes in every lane of the upper profile dwords --------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_extreme_bytes(dev, LB, mode):
    """127 and -128 at every column code >= 8, in rows of the second stripe."""
    P, B, cs = PR.extreme_case(mode)
    assert P.max() == 127 and P.min() == -128 and PR.EXT_ROW0 >= 64 and min(cs) == 8
    ref = PR.profile_reference(mode, P, B, PR.alphabet_of(mode))
    for single in (True, False):
        pl, dDir = _run(LB, dev, mode, P, [(0, len(P))], [B], single=single)
        _check(mode, pl, dDir, P, B, ref)


# ---- 8. plan errors ----------------------------------------------------------------------------------------------
def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


@pytest.mark.parametrize("mode", MODES)
def test_plan_errors(dev, LB, mode):
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    P32 = PR.pad32(PR.edge_case(mode, 65)[0])
    B = [b"A" * 70]
    assert _status(lambda: _plan(LB, mode, P32, [(0, 65)], B)) == 0
    assert _status(lambda: _plan(LB, mode, P32, [(0, 65)], B, band=0)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, mode, P32, [(0, 65)], B, band=100)) == UNSUPPORTED
    for alg in (LB.NW_OVERLAP, LB.NW_EXTEND, LB.SW_AFFINE):
        assert _status(lambda: _plan(LB, mode, P32, [(0, 65)], B, alg=alg)) == UNSUPPORTED
    for cells in (LB.CELLS_H, LB.CELLS_TAB):
        assert _status(lambda: _plan(LB, mode, P32, [(0, 65)], B, cells=cells)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, mode, P32, [(1, 65)], B)) == ARG          # a_off + m = prof_rows + 1
    assert _status(lambda: _plan(LB, mode, P32, [(0, 66)], B)) == ARG
    assert _status(lambda: _plan(LB, mode, P32, [(-1, 10)], B)) == ARG
    assert _status(lambda: _plan(LB, mode, P32, [(1, 64), (0, 65)], B * 2)) == 0
    assert _status(lambda: _plan(LB, mode, P32, [(0, 65)], B, go=1, ge=-1)) == UNSUPPORTED
    with pytest.raises(ValueError):
        Plan(_alg(LB, mode), LB.CELLS_NONE, [65], [70], [0], [0], sub=np.zeros((32, 32)), profile=P32)
    # the value-range inequality of the alg, on sizes for which no buffer is ever asked: a small-magnitude profile of
    # the same sizes is accepted as far as the ranges go
    big, small = np.full((64, 32), 127, dtype=np.int8), np.ones((64, 32), dtype=np.int8)
    if mode == "local":
        # smax min(m, n) < 2^29 fails from 127 x 4,227,331 on.  (The accepted side cannot be created at these sizes on
        # any device -- a pair of 4.2M x 4.2M asks for a terabyte of hand-off granules --, so a local plan's acceptance
        # is the small plans' above and every other test's; the rejection itself asks for no buffer.)
        m = 4_227_331
        assert 127 * m >= 1 << 29 > 127 * (m - 1)
        assert _status(lambda: Plan(LB.SW_SCORED, LB.CELLS_NONE, [m], [m], [0], [0], gap_open=GO, gap_extend=GE,
                                    profile=np.full((m, 32), 127, dtype=np.int8))) == UNSUPPORTED
    else:
        # (s + 2 G + 2 g) (m + n + 256) + (G - g) < 2^28 with s = the largest |entry|: G = 5, g = 2
        n = (1 << 28) // (127 + 14) - 64 - 256 + 2
        assert (127 + 14) * (64 + n + 256) + 3 >= 1 << 28 > (1 + 14) * (64 + n + 256) + 3
        assert n <= 1 << 26
        for prof, want in ((big, UNSUPPORTED), (-big - 1, UNSUPPORTED), (small, 0)):
            assert _status(lambda: Plan(_alg(LB, mode), LB.CELLS_NONE, [64], [n], [0], [0], gap_open=GO,
                                        gap_extend=GE, profile=prof)) == want


def test_run_needs_no_row_codes(dev, LB):
    """msa_plan_run ignores dA for a profile plan (NULL), and still wants it for a table plan."""
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    P, B = PR.edge_case("global", 65)
    pl = _plan(LB, "global", PR.pad32(P), [(0, 65)], [B], cells=LB.CELLS_NONE)
    dB = _dev(B, PR.AL32, dev)
    assert LB.lib().msa_plan_run(pl._h, None, C.c_void_p(dB.data_ptr()), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert pl.results()[0]["score"] == PR.profile_reference("global", P, B, PR.AL32)["score"]
    pt = Plan(LB.NW_SCORED, LB.CELLS_NONE, [65], [70], [0], [0], gap_open=GO, gap_extend=GE, sub=np.zeros((32, 32)))
    assert LB.lib().msa_plan_run(pt._h, None, C.c_void_p(dB.data_ptr()), None, None, None, None) == ARG


# ---- 9. host entries and api -------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _entry_single(LB, mode, P, B, al, traceback=True):
    P8 = np.ascontiguousarray(P, dtype=np.int8)
    sc = C.c_int32()
    beg, end = np.full(2, -7, dtype=np.int64), np.full(2, -7, dtype=np.int64)
    cap = 4 * (len(P) + len(B)) + 16
    cig = C.create_string_buffer(cap) if traceback else None
    rc = LB.lib().msa_profile_align(MODES.index(mode), _p(P8), len(P8), B, len(B), al, len(al), GO, GE, C.byref(sc),
                                    _p(beg) if traceback else None, _p(end), cig, cap if traceback else 0)
    assert rc == 0, rc
    r = dict(score=sc.value, beg=tuple(int(x) for x in beg) if traceback else None, end=tuple(int(x) for x in end))
    if traceback:
        r["cigar"] = cig.value.decode()
    return r


def _want(mode, ref, m, n, traceback=True):
    r = PR.result_of(mode, ref, m, n)
    if not traceback:
        del r["cigar"]
        r["beg"] = None
    return r


@pytest.mark.parametrize("mode", MODES)
def test_host_entries_and_api(dev, LB, mode):
    from cse305_parallel_sequence_alignment_amd import api

    al = PR.alphabet_of(mode)
    P, Bs = PR.batch_case(mode)
    P, Bs = P[100:270], [b[:120] for b in Bs]          # 170 rows: three stripes; five sequences, one of them unrelated
    refs = [PR.profile_reference(mode, P, b, al) for b in Bs]
    m = len(P)
    for tb in (True, False):
        assert _entry_single(LB, mode, P, Bs[3], al, tb) == _want(mode, refs[3], m, len(Bs[3]), tb)
        assert api.profile_align(P, Bs[3], al, mode=mode, gap_open=GO, gap_extend=GE, traceback=tb) == \
            _want(mode, refs[3], m, len(Bs[3]), tb)
        got = api.profile_align_batch(P, Bs, al, mode=mode, gap_open=GO, gap_extend=GE, traceback=tb)
        assert got == [_want(mode, r, m, len(b), tb) for r, b in zip(refs, Bs)]
    if mode == "local":
        assert refs[4]["score"] == 0 and _want(mode, refs[4], m, len(Bs[4]))["cigar"] == ""
    # the batch entry itself: CAPACITY with the needed size and the scores, then success
    k = len(Bs)
    Bcat = b"".join(Bs)
    bo, n = np.asarray(_offsets(Bs), dtype=np.int64), np.asarray([len(b) for b in Bs], dtype=np.int64)
    P8 = np.ascontiguousarray(P, dtype=np.int8)
    sc, coff = np.zeros(k, np.int32), np.zeros(k + 1, np.int64)
    beg, end = np.zeros((k, 2), np.int64), np.zeros((k, 2), np.int64)

    def batch(cig, cap):
        return LB.lib().msa_profile_align_batch(MODES.index(mode), _p(P8), m, Bcat, len(Bcat), k, _p(bo), _p(n), al,
                                                len(al), GO, GE, _p(sc), _p(beg), _p(end), cig, cap, _p(coff))
    want = [PR.result_of(mode, r, m, len(b)) for r, b in zip(refs, Bs)]
    assert batch(C.create_string_buffer(4), 4) == CAPACITY
    need = int(coff[k])
    assert need == sum(len(w["cigar"]) + 1 for w in want)
    assert [int(x) for x in sc] == [w["score"] for w in want]   # the scores are the caller's all the same
    assert [tuple(int(x) for x in e) for e in end] == [w["end"] for w in want]
    cig = C.create_string_buffer(need)
    assert batch(cig, need) == 0
    for p, w in enumerate(want):
        assert (int(sc[p]), tuple(int(x) for x in beg[p]), tuple(int(x) for x in end[p])) == (w["score"], w["beg"], w["end"])
        assert cig.raw[coff[p]:coff[p + 1] - 1].decode() == w["cigar"]
    # a table's profile through the api is the matrix-scored call
    A, B = PR.table_case(mode)
    A, B, T = A[:150], B[:140], PR.table_of(mode)
    got = api.profile_align(api.profile_from_matrix(A, al, T), B, al, mode=mode, gap_open=GO, gap_extend=GE)
    kw = dict(gap_open=GO, gap_extend=GE, alphabet=al, matrix=T, max_symbols=32)
    if mode == "local":
        t = api.sw_align(A, B, **kw)
        assert got == dict(score=t["score"], beg=t["beg"], end=t["end"], cigar=t["cigar"])
    elif mode == "global":
        t = api.nw_align(A, B, **kw)
        assert got == dict(score=t["score"], beg=(0, 0), end=(150, 140), cigar=t["cigar"])
    else:
        t = api.fit_align(A, B, **kw)
        assert got == dict(score=t["score"], beg=(0, t["beg"]), end=(150, t["end"]), cigar=t["cigar"])
