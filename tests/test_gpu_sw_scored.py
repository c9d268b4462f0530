"""Local alignment under a substitution matrix (MSA_SW_SCORED plans over 3-bit and 5-bit codes, the walkers on them,
msa_sw_align_scored / _batch_scored / _scored32 / _batch_scored32, api.sw_align / sw_align_batch with alphabet= /
matrix= / max_symbols=) against the yardstick tests/sw_scored_reference.py, which test_sw_scored_reference.py checks
against the oracle's orc_sw and a plain-Python triple loop.

Everything is exact integer equality: the score, the end cell (first maximum, row-major), the plan's error word, bits
0-3 of every interior direction byte, the walks' ops, start cell and CIGAR, and the ops rescored.  Shapes are the
smallest at which each mechanism runs: more stripes than a single launch's waves (two items, the granule hand-off),
more stripes than a batch workgroup's waves (the wrap link), a one-row pair, an exact-stripe pair, the end-cell
formats on either side of their bound."""
import ctypes as C
import functools

import numpy as np
import pytest

import sw_scored_reference as SR
import wide_reference as W

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG, CAPACITY = -5, -1, -8
GO, GE = SR.GO, SR.GE
WIDTHS = [8, 32]


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _dev(x, alphabet, dev):
    import torch

    return torch.from_numpy(W.codes32(x, alphabet).astype(np.uint8)).to(dev)


def _offsets(seqs):
    return np.concatenate(([0], np.cumsum([len(s) for s in seqs])[:-1]))


def _plan(LB, pairs, sub, cells=None, single=None, go=GO, ge=GE, alg=None, **kw):
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    As, Bs = [a for a, _ in pairs], [b for _, b in pairs]
    return Plan(LB.SW_SCORED if alg is None else alg, LB.CELLS_DIR if cells is None else cells, [len(a) for a in As],
                [len(b) for b in Bs], _offsets(As), _offsets(Bs), gap_open=go, gap_extend=ge, single=single, sub=sub,
                **kw)


def _run(LB, dev, pairs, alphabet, sub, **kw):
    import torch

    pl = _plan(LB, pairs, sub, **kw)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev) if pl.cells_elems else None
    pl.run(_dev(b"".join(a for a, _ in pairs), alphabet, dev), _dev(b"".join(b for _, b in pairs), alphabet, dev), dDir)
    return pl, dDir


def _check(pl, dDir, A, B, alphabet, S, ref, w, pair=0, go=GO, ge=GE):
    """Everything a fill test checks for one pair (see the module docstring); returns the single walker's result."""
    res = pl.results()[pair]
    assert (res["score"], tuple(res["end"]), res["status"]) == (ref["score"], ref["end"], 0)
    assert pl.error() == 0
    assert pl.launch_info()["mode"] == "stripe" and pl.format_info()["codes"] == w
    got = pl.deskew_dir(dDir.cpu().numpy(), pair, pl.stripe_meta())
    bad = (got[1:, 1:] & 15) != (ref["byte"][1:, 1:] & 15)
    assert not bad.any(), ("bits 0-3", int(bad.sum()), (np.argwhere(bad)[:4] + 1).tolist())
    tb = pl.traceback(dDir, pair)
    assert (tb["ops"], tb["beg"], tb["cigar"]) == (ref["ops"], ref["beg"], ref["cigar"])
    if ref["score"] > 0:
        assert SR.rescore(A, B, tb["beg"], tb["ops"], alphabet, S, go, ge) == (ref["score"], ref["end"])
    return tb


# ---- 1, 2. every cell of one pair ------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WIDTHS)
def test_single_pair_every_cell(dev, LB, w):
    """330 x 300: six stripes in two items of four waves; every (row code, column code) pair is a cell."""
    al, T, sub = SR.width(w)
    k = len(al)
    A, B = SR.every_cell(w)
    a, b = W.codes32(A, al), W.codes32(B, al)
    assert np.unique(32 * a[:, None] + b[None, :]).size == k * k == (49 if w == 8 else 961)
    assert (a == k - 1).any() and (b == k - 1).any()
    ref = SR.sw_scored_reference(A, B, al, T, GO, GE)
    assert ref["score"] > 0 and b"M" in ref["ops"]
    pl, dDir = _run(LB, dev, [(A, B)], al, sub(T), single=True)
    assert pl.single and pl.launch_info()["items"] == 2
    _check(pl, dDir, A, B, al, T, ref, w)


# ---- 3. the sentinel column ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WIDTHS)
def test_all_positive_table_scores_the_sentinel(dev, LB, w):
    """Every entry >= 1, and the caller's own sentinel row and column (ignored by contract) positive too: were column
    7 / 31 of the table used for the virtual columns left of column 1 and right of column n, H would grow there and
    the scores change."""
    al, _, sub = SR.width(w)
    k = len(al)
    P = SR.ALL_POS7 if w == 8 else SR.ALL_POS31
    assert P.min() >= 1
    tab = sub(P)
    tab[k, :] = tab[:, k] = 127
    for A, B in SR.all_positive(w):
        ref = SR.sw_scored_reference(A, B, al, P, GO, GE)
        # what a table entry in the sentinel's place would give: the same pair with B between two runs of a symbol
        # that scores 127 against everything
        ext = np.full((k + 1, k + 1), 127, dtype=np.int64)
        ext[:k, :k] = P
        al1 = al + b"#"
        wrong = SR.sw_scored_reference(A, b"#" * 64 + B + b"#" * 64, al1, ext, GO, GE, walk=False)
        assert wrong["score"] != ref["score"]
        for single in (True, False):
            pl, dDir = _run(LB, dev, [(A, B)], al, tab, single=single)
            _check(pl, dDir, A, B, al, P, ref, w)


# ---- 4. ragged batches -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ragged(w):
    al, T, _ = SR.width(w)
    pairs = SR.ragged_batch(w)
    return pairs, [SR.sw_scored_reference(a, b, al, T, GO, GE) for a, b in pairs]


@pytest.mark.parametrize("cells", ["dir", "none"])
@pytest.mark.parametrize("w", WIDTHS)
def test_ragged_batch(dev, LB, w, cells):
    al, T, sub = SR.width(w)
    pairs, refs = _ragged(w)
    assert [(len(a), len(b)) for a, b in pairs[:4]] == SR.BATCH and refs[4]["score"] == 0
    if cells == "none":
        pl, _ = _run(LB, dev, pairs, al, sub(T), cells=LB.CELLS_NONE)
        assert pl.cells_elems == 0 and not pl.single
        assert [(r["score"], tuple(r["end"])) for r in pl.results()] == [(ref["score"], ref["end"]) for ref in refs]
        assert pl.error() == 0 and pl.launch_info()["mode"] == "stripe" and pl.format_info()["codes"] == w
        return
    pl, dDir = _run(LB, dev, pairs, al, sub(T))
    assert not pl.single
    singles = [_check(pl, dDir, a, b, al, T, ref, w, pair=p) for p, ((a, b), ref) in enumerate(zip(pairs, refs))]
    batch = pl.traceback_batch(dDir)
    for one, tb in zip(singles, batch):
        assert (tb["ops"], tb["beg"], tb["cigar"]) == (one["ops"], one["beg"], one["cigar"])
    assert batch[4]["ops"] == b""  # score 0: no walk


# ---- 5. two equal maxima ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WIDTHS)
def test_first_of_two_equal_maxima(dev, LB, w):
    al, _, sub = SR.width(w)
    P = SR.planted_table(len(al))
    q, r = SR.planted_twice(w)
    ref = SR.sw_scored_reference(q, r, al, P, GO, GE)
    assert np.argwhere(ref["H"] == ref["score"]).tolist() == [[40, 70], [40, 160]] and ref["end"] == (40, 70)
    for single in (True, False):
        pl, dDir = _run(LB, dev, [(q, r)], al, sub(P), single=single)
        tb = _check(pl, dDir, q, r, al, P, ref, w)
        assert tb["cigar"] == "40M" and tb["beg"] == (1, 31)
    # ... and with the copies in different rows: the query is the reference, the reference the query planted twice
    ref = SR.sw_scored_reference(r, q, al, P.T, GO, GE)
    assert ref["end"] == (70, 40) and ref["H"][160, 40] == ref["score"]
    pl, dDir = _run(LB, dev, [(r, q)], al, sub(P.T), single=True)
    _check(pl, dDir, r, q, al, P.T, ref, w)


# ---- 6. the end-cell formats at their bound --------------------------------------------------------------------
@pytest.mark.parametrize("L,tracking,score", [(516, "key", 65532), (517, "select", 65659)])
@pytest.mark.parametrize("w", WIDTHS)
def test_end_cell_format_bound(dev, LB, w, L, tracking, score):
    """127 L < 65536 packs the first maximum's step with the value; one symbol more and it is compare-select."""
    al, _, sub = SR.width(w)
    S = SR.self127(len(al))
    s = al[1:2] * L
    ref = SR.sw_scored_reference(s, s, al, S, GO, GE)
    assert (ref["score"], ref["end"]) == (score, (L, L))
    for single in (True, False):
        pl, dDir = _run(LB, dev, [(s, s)], al, sub(S), single=single, cells=LB.CELLS_DIR if w == 8 else LB.CELLS_NONE)
        assert pl.format_info()["tracking"] == tracking and pl.format_info()["codes"] == w
        res = pl.results()[0]
        assert (res["score"], tuple(res["end"])) == (score, (L, L)) and pl.error() == 0
        if w == 8:
            _check(pl, dDir, s, s, al, S, ref, w)


# ---- 7. extreme bytes at codes >= 8 ----------------------------------------------------------------------------
def test_extreme_bytes_wide(dev, LB):
    S, A, B = SR.extreme31()
    assert S[20, 21] == 127 and S[9, 9] == -128 and S[21, 20] != 127
    ref = SR.sw_scored_reference(A, B, SR.AL31, S, GO, GE)
    plain = SR.sw_scored_reference(A, B, SR.AL31, SR.T31, GO, GE)
    assert ref["score"] > 19 * 127 and (ref["score"], ref["cigar"]) != (plain["score"], plain["cigar"])
    assert b"I" in ref["ops"] or b"D" in ref["ops"]  # round the -128
    for single in (True, False):
        pl, dDir = _run(LB, dev, [(A, B)], SR.AL31, W.sub32(S), single=single)
        _check(pl, dDir, A, B, SR.AL31, S, ref, 32)


# ---- 8. NULL sub: the MSA_SW_AFFINE plan -----------------------------------------------------------------------
def test_null_sub_equals_affine_plan(oracle, dev, LB):
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    import alphabet8 as A8

    A, B = A8.named("swa_300x257")
    sc = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2)
    want = oracle.sw(A, B, 2, -3, 5, 2, want_tb=True)
    dA, dB = _dev(A, A8.AL7, dev), _dev(B, A8.AL7, dev)
    out = []
    for alg, kw in ((LB.SW_SCORED, {}), (LB.SW_AFFINE, dict(track_end=True))):
        for single in (True, False):
            pl = Plan(alg, LB.CELLS_DIR, [len(A)], [len(B)], [0], [0], single=single, **sc, **kw)
            D = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
            pl.run(dA, dB, D)
            res, tb = pl.results()[0], pl.traceback(D)
            assert (res["score"], tuple(res["end"]), tb["beg"], tb["cigar"]) == \
                (want["score"], tuple(want["end"]), tuple(want["beg"]), want["cigar"])
            mode = pl.launch_info()["mode"]
            assert alg == LB.SW_AFFINE or mode == "stripe"
            out.append((mode, tb["ops"], pl.deskew_dir(D.cpu().numpy(), 0, pl.stripe_meta())[1:, 1:] & 15))
    assert sum(mode == "stripe" for mode, _, _ in out) >= 3  # both scored plans and the affine batch plan
    assert [mode for mode, _, _ in out].count("flow") == 1  # the single-pair affine plan
    for mode, ops, byte in out[1:]:
        assert ops == out[0][1]
        assert (byte == out[0][2]).all()  # all four planes, the flow kernel's too (test_gpu_flow_dir.py): the contract's


# ---- 9. host entries and api -----------------------------------------------------------------------------------
def _entry_single(LB, name, A, B, al, S, go, ge, traceback=True):
    S = np.ascontiguousarray(S, dtype=np.int8)
    sc, ei, ej, bi, bj = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    cap = 4 * (len(A) + len(B)) + 16
    cig = C.create_string_buffer(cap) if traceback else None
    rc = getattr(LB.lib(), name)(A, len(A), B, len(B), al, len(al), S.ctypes.data_as(C.c_void_p), go, ge, C.byref(sc),
                                 C.byref(ei), C.byref(ej), C.byref(bi) if traceback else None,
                                 C.byref(bj) if traceback else None, cig, cap if traceback else 0)
    assert rc == 0, rc
    r = dict(score=sc.value, end=(ei.value, ej.value))
    if traceback:
        r.update(beg=(bi.value, bj.value), cigar=cig.value.decode())
    return r


def _want(ref, traceback=True):
    r = dict(score=ref["score"], end=ref["end"])
    if traceback:
        r.update(beg=ref["beg"], cigar=ref["cigar"])
    return r


def test_protein_through_every_entry(dev, LB):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, (a0, a1), (b0, b1) = SR.protein_case()
    S, go, ge = W.protein20(), SR.PGO, SR.PGE
    ref = SR.sw_scored_reference(A, B, W.AL20, S, go, ge)
    # the local alignment holds the planted regions
    assert ref["beg"][0] - 1 <= a0 + 5 and ref["end"][0] >= a1 - 5
    assert ref["beg"][1] - 1 <= b0 + 5 and ref["end"][1] >= b1 - 5
    for tb in (True, False):
        assert _entry_single(LB, "msa_sw_align_scored32", A, B, W.AL20, S, go, ge, tb) == _want(ref, tb)
        assert api.sw_align(A, B, gap_open=go, gap_extend=ge, alphabet=W.AL20, matrix=S, max_symbols=32,
                            traceback=tb) == _want(ref, tb)
    # the batch entry: this pair, its mirror image and a short pair; CAPACITY with the needed size, then success
    pairs = [(A, B), (B, A), (A[60:100], B[35:80])]
    refs = [ref, SR.sw_scored_reference(B, A, W.AL20, S, go, ge),
            SR.sw_scored_reference(*pairs[2], W.AL20, S, go, ge)]
    Acat, Bcat = b"".join(a for a, _ in pairs), b"".join(b for _, b in pairs)
    k = len(pairs)
    i64 = lambda v: np.asarray(v, dtype=np.int64)  # noqa: E731
    P = lambda x: x.ctypes.data_as(C.c_void_p)     # noqa: E731
    ao, bo = i64(_offsets([a for a, _ in pairs])), i64(_offsets([b for _, b in pairs]))
    m, n = i64([len(a) for a, _ in pairs]), i64([len(b) for _, b in pairs])
    S8 = np.ascontiguousarray(S, dtype=np.int8)
    sc, coff = np.zeros(k, np.int32), np.zeros(k + 1, np.int64)
    end, beg = np.zeros((k, 2), np.int64), np.zeros((k, 2), np.int64)

    def batch(cig, cap):
        return LB.lib().msa_sw_align_batch_scored32(Acat, len(Acat), Bcat, len(Bcat), k, P(ao), P(m), P(bo), P(n),
                                                    W.AL20, 20, P(S8), go, ge, P(sc), P(end), P(beg), cig, cap, P(coff))
    small = C.create_string_buffer(4)
    assert batch(small, 4) == CAPACITY
    need = int(coff[k])
    assert need == sum(len(r["cigar"]) + 1 for r in refs)
    assert [int(x) for x in sc] == [r["score"] for r in refs]   # the scores are the caller's all the same
    cig = C.create_string_buffer(need)
    assert batch(cig, need) == 0
    for p, r in enumerate(refs):
        assert (int(sc[p]), tuple(end[p]), tuple(beg[p])) == (r["score"], r["end"], r["beg"])
        assert cig.raw[coff[p]:coff[p + 1] - 1].decode() == r["cigar"]
    for tb in (True, False):
        got = api.sw_align_batch([a for a, _ in pairs], [b for _, b in pairs], gap_open=go, gap_extend=ge,
                                 alphabet=W.AL20, matrix=S, max_symbols=32, traceback=tb)
        assert got == [_want(r, tb) for r in refs]
    # the shared-reference form: every query against one B, uploaded once
    qs = [A, A[50:220], A[100:130]]
    got = api.sw_align_batch(qs, B, gap_open=go, gap_extend=ge, alphabet=W.AL20, matrix=S, max_symbols=32)
    assert got == [_want(SR.sw_scored_reference(q, B, W.AL20, S, go, ge)) for q in qs]


def test_four_symbols_through_either_width(oracle, dev, LB):
    from cse305_parallel_sequence_alignment_amd import api

    rng = np.random.default_rng(871)
    A, B = SR.homologous(rng, 200, 180, b"ACGT")
    # transitions cheaper than transversions, and not symmetric
    S = np.array([[3, -4, -1, -4], [-4, 3, -4, -1], [-2, -4, 3, -4], [-4, -2, -4, 3]])
    ref = SR.sw_scored_reference(A, B, b"ACGT", S, GO, GE)
    assert ref["score"] > 0
    for ms in (8, 32):
        assert api.sw_align(A, B, gap_open=GO, gap_extend=GE, alphabet=b"ACGT", matrix=S, max_symbols=ms) == _want(ref)
        assert api.sw_align_batch([A, A], [B, B[:90]], gap_open=GO, gap_extend=GE, alphabet=b"ACGT", matrix=S,
                                  max_symbols=ms)[0] == _want(ref)
    for name in ("msa_sw_align_scored", "msa_sw_align_scored32"):
        assert _entry_single(LB, name, A, B, b"ACGT", S, GO, GE) == _want(ref)
    # match / mismatch over the sequences' own symbols with max_symbols=32: today's answer
    want = oracle.sw(A, B, 2, -3, GO, GE, want_tb=True)
    got = api.sw_align(A, B, match=2, mismatch=-3, gap_open=GO, gap_extend=GE, max_symbols=32)
    assert got == dict(score=want["score"], end=tuple(want["end"]), beg=tuple(want["beg"]), cigar=want["cigar"])
    assert got == api.sw_align(A, B, match=2, mismatch=-3, gap_open=GO, gap_extend=GE)


# ---- 10. rejections --------------------------------------------------------------------------------------------
def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


@pytest.mark.parametrize("w", WIDTHS)
def test_plan_rejections(dev, LB, w):
    import torch

    al, T, sub = SR.width(w)
    pair = [(SR.rs(np.random.default_rng(5), 70, al), SR.rs(np.random.default_rng(6), 80, al))]
    for cells in (LB.CELLS_H, LB.CELLS_TAB):
        assert _status(lambda: _plan(LB, pair, sub(T), cells=cells)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, pair, sub(T), band=16)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, pair, sub(T), go=-1)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, pair, sub(T), ge=-1)) == UNSUPPORTED
    assert _status(lambda: _plan(LB, pair, sub(T), go=1, ge=3)) == 0  # (no order between the two, as MSA_SW_AFFINE)
    # a table stays unsupported for MSA_SW_AFFINE
    assert _status(lambda: _plan(LB, pair, sub(T), alg=LB.SW_AFFINE)) == UNSUPPORTED
    # 127 min(m, n) >= 2^29: rejected at creation (no buffer of that size is ever asked for)
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    S = sub(SR.self127(len(al)))
    assert _status(lambda: Plan(LB.SW_SCORED, LB.CELLS_NONE, [1 << 23], [1 << 23], [0], [0], gap_open=GO,
                                gap_extend=GE, sub=S)) == UNSUPPORTED
    # the global walkers reject the plan
    pl, dDir = _run(LB, dev, pair, al, sub(T))
    ops = torch.zeros(256, dtype=torch.uint8, device=dev)
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert LB.lib().msa_plan_traceback_nw(pl._h, 0, P(dDir), P(ops), 256, P(info), None) == UNSUPPORTED
    assert LB.lib().msa_plan_traceback_gotoh(pl._h, 0, -1, P(dDir), P(ops), 256, P(info), None) == UNSUPPORTED
    # ... and a plan without direction bytes has nothing to walk
    pn, _ = _run(LB, dev, pair, al, sub(T), cells=LB.CELLS_NONE)
    assert LB.lib().msa_plan_traceback(pn._h, 0, P(ops), P(ops), 256, P(info), None) == UNSUPPORTED


def test_entry_rejections(dev, LB):
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    A = B = W.AL32
    sc, ei, ej = C.c_int32(), C.c_int64(), C.c_int64()

    def single(name, n_sym, sub=True):
        S = np.zeros((n_sym, n_sym), dtype=np.int8)
        return getattr(LB.lib(), name)(A[:n_sym], n_sym, B[:n_sym], n_sym, W.AL32[:n_sym], n_sym,
                                       S.ctypes.data_as(C.c_void_p) if sub else None, GO, GE, C.byref(sc),
                                       C.byref(ei), C.byref(ej), None, None, None, 0)
    assert single("msa_sw_align_scored", 8) == ARG and single("msa_sw_align_scored", 7) == 0
    assert single("msa_sw_align_scored32", 32) == ARG and single("msa_sw_align_scored32", 31) == 0
    assert single("msa_sw_align_scored32", 20, sub=False) == ARG
    # msa_plan_create_scored32 with a NULL table
    arrs = [(C.c_int64 * 1)(v) for v in (70, 80, 0, 0)]
    d = LB.PlanDesc(alg=LB.SW_SCORED, cells=LB.CELLS_NONE, match=1, mismatch=0, gap_open=GO, gap_extend=GE,
                    start_type=-1, band=-1, track_end=0, single=1, n_pairs=1, m=arrs[0], n=arrs[1], a_off=arrs[2],
                    b_off=arrs[3])
    h = C.c_void_p()
    assert LB.lib().msa_plan_create_scored32(C.byref(d), None, C.byref(h)) == ARG
    # any other shape of sub is the wrapper's ValueError
    with pytest.raises(ValueError):
        Plan(LB.SW_SCORED, LB.CELLS_NONE, [70], [80], [0], [0], sub=np.zeros((7, 7)))
