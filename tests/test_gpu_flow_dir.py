"""The two-value flow kernels (msa_flow.hip: the SW-affine fill with direction bytes and the tagged reference-Gotoh
fill, pass 1 and both builds of their pass-2 bodies) cell by cell against CPU references.

Every comparison is with tests/flow_dir_reference.py -- sw_scored_reference's byte contract, the tags of the oracle's
(unswapped) tables, a plain-Python walker, the row-streaming restatements -- which test_flow_dir_reference.py checks
on the CPU together with the inputs and the shape list; nothing here compares with another GPU kernel.  Integer DP:
everything is exact, no cell is masked out.  Every plan is a single-pair flow plan with two rows per lane, and its
error word is 0 after every run.

a. The in-launch pass 2 (segments of 8 phases) at FR.SHAPES: the shapes on either side of the head / short switch of
   stripe 0 and of the later stripes, of the 8 | 9 and 16 | 17 phase counts, of the row, stripe and item boundaries,
   and stripes 16 and 17.  A mismatch is reported as (i, j, got, want, stripe, phase, lane).
b. The separate fill launch (segments of 32 phases) at the smallest m that selects it and n = 460, where every full
   stripe restarts from SNAP at phase 32: rows 1..1,100 and the last 600 rows in full (the walk of the 460 columns
   needs more than the last 300), score and end or fin, and the device walk.
c. One plan run on two inputs at (513, 193): no granule or SNAP value of the first epoch survives.
"""
import functools

import numpy as np
import pytest

import flow_dir_reference as FR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _dev(x, dev):
    import torch

    return torch.from_numpy(FR.codes(x)).to(dev)


def _plan(LB, alg, m, n, scoring):
    """The single-pair flow plan of a shape: SW affine under (match, mismatch, gap_open, gap_extend) or reference
    Gotoh under (g, h)."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    if alg == "sw":
        ma, mi, go, ge = scoring
        pl = Plan(LB.SW_AFFINE, LB.CELLS_DIR, [m], [n], [0], [0], match=ma, mismatch=mi, gap_open=go, gap_extend=ge,
                  track_end=True, single=True)
    else:
        g, h = scoring
        pl = Plan(LB.REF_GOTOH, LB.CELLS_DIR, [m], [n], [0], [0], match=1, mismatch=0, gap_open=g + h, gap_extend=g,
                  start_type=-1, single=True)
        assert pl.format_info()["values"] == "tagged4", (m, n, scoring)
    info = pl.launch_info()
    assert info["mode"] == "flow" and info["rows_per_lane"] == 2, (m, n, scoring, info)
    return pl


def _run(pl, A, B, dev):
    import torch

    D = torch.empty(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev(A, dev), _dev(B, dev), D)
    return D


def _plane(pl, D, mask):
    return pl.deskew_dir(D.cpu().numpy(), 0, pl.stripe_meta())[1:, 1:] & mask


def _check_sw(pl, D, A, B, scoring, ref, what):
    got, want = _plane(pl, D, 15), ref["byte"][1:, 1:] & 15
    print(what, "cells differing:", int((got != want).sum()))
    assert np.array_equal(got, want), (what, FR.first_bad(got, want))
    r = pl.results()[0]
    assert (r["score"], tuple(r["end"])) == (ref["score"], ref["end"]), what
    tb = pl.traceback(D)
    assert (tb["ops"], tuple(tb["beg"]), tb["cigar"]) == (ref["ops"], ref["beg"], ref["cigar"]), what
    if ref["score"] > 0:
        assert FR.sw_rescore(A, B, tb["beg"], tb["ops"], scoring) == (ref["score"], ref["end"]), what
    assert pl.error() == 0, what


@functools.lru_cache(maxsize=None)
def _gotoh_case(oracle, kind, m, n, gh, salt=0):
    """(A, B, tags, fin, walker's ops, walker's stop) of one Gotoh case; computed once, never modified."""
    g, h = gh
    A, B = FR.pair_of(kind, m, n, salt)
    T = FR.unswapped_tables(oracle, A, B, g, h)
    tags = FR.gotoh_tags(*T, float(g), float(h))
    fin = tuple(float(t[m, n]) for t in T)
    return (A, B, tags, fin) + FR.gotoh_walk(tags, fin, m, n)


def _check_gotoh(pl, D, case, what):
    A, B, want, fin, ops, stop = case
    got = _plane(pl, D, 63)
    print(what, "cells differing:", int((got != want).sum()))
    assert np.array_equal(got, want), (what, FR.first_bad(got, want))
    assert tuple(float(x) for x in pl.results()[0]["fin"]) == fin, what
    tb = pl.traceback_gotoh(D, end_type=-1)
    assert (tb["ops"], tuple(tb["stop"])) == (ops, stop), what
    assert pl.error() == 0, what


# ---- a. the in-launch pass 2, every interior cell ----------------------------------------------------------------
@pytest.mark.parametrize("m,n", FR.SHAPES)
def test_sw_affine_every_cell(dev, LB, m, n):
    """SW affine with direction bytes and the end cell: bits 0-3 of every interior byte, the score, the first-maximum
    end cell, and the device traceback's ops, beg and CIGAR equal sw_scored_reference's; the ops rescore to the
    score."""
    for ci, scoring in enumerate(FR.SW_SCORINGS):
        pl = _plan(LB, "sw", m, n, scoring)
        for kind in FR.case_kinds((m, n), ci):
            A, B, ref = FR.sw_case(kind, m, n, scoring)
            _check_sw(pl, _run(pl, A, B, dev), A, B, scoring, ref, (m, n, scoring, kind))


@pytest.mark.parametrize("m,n", FR.SHAPES)
def test_gotoh_every_cell(oracle, dev, LB, m, n):
    """Reference Gotoh, start type -1: bits 0-5 of every interior byte equal the tags of the oracle's unswapped
    tables, fin the three tables at (m, n), and the device walk for end type -1 the Python walker's ops and stop cell
    -- for the pairs with m > n too, which the oracle's own walk does not cover."""
    for ci, gh in enumerate(FR.GOTOH_GH):
        pl = _plan(LB, "gotoh", m, n, gh)
        for kind in FR.case_kinds((m, n), ci):
            case = _gotoh_case(oracle, kind, m, n, gh)
            _check_gotoh(pl, _run(pl, case[0], case[1], dev), case, (m, n, gh, kind))


# ---- b. the separate fill launch with more than one segment ------------------------------------------------------
TOP = (1, 1100)   # two items, every 32-phase segment restart and the masked tails
BOTTOM_ROWS = 600  # the partial last stripe, the phase with the final cell, and the whole walk of the 460 columns


def _tall(dev):
    import torch

    m = FR.fill_launch_min_m(torch.cuda.get_device_properties(dev).multi_processor_count)
    assert m is not None
    return m, FR.TALL_N, (TOP, (m - BOTTOM_ROWS + 1, m))


def _tall_plan(LB, alg, m, n, scoring):
    """The plan of the smallest m with a fill launch of its own: fill_grid > 0 here and 0 one row below."""
    assert _plan(LB, alg, m - 1, n, scoring).launch_info()["fill_grid"] == 0
    pl = _plan(LB, alg, m, n, scoring)
    assert pl.launch_info()["fill_grid"] > 0, pl.launch_info()
    assert FR.fl_P(0, m, n) > FR.FL_PS_FILL  # a second segment
    return pl


@functools.lru_cache(maxsize=None)
def _tall_sw(m, scoring, wins):
    A, B = FR.tall_pair(m)
    return FR.sw_stream(A, B, scoring, wins)


@functools.lru_cache(maxsize=None)
def _tall_gotoh(m, gh, wins):
    A, B = FR.tall_pair(m)
    return FR.gotoh_stream(A, B, gh[0], gh[1], wins)


def _check_windows(got, rows, what):
    for (lo, hi), want in rows.items():
        g = got[lo - 1:hi]
        print(what, (lo, hi), "cells differing:", int((g != want).sum()))
        assert np.array_equal(g, want), (what, lo, hi, FR.first_bad(g, want, i0=lo))


@pytest.mark.parametrize("scoring", FR.SW_SCORINGS[:2], ids=["floorless", "floor"])
def test_fill_launch_two_segments_sw_affine(oracle, dev, LB, scoring):
    """fill_block_aff2<1> restarted from SNAP at phase 32: the row windows against sw_stream, score and end, and the
    device traceback against the oracle's."""
    m, n, wins = _tall(dev)
    A, B = FR.tall_pair(m)
    pl = _tall_plan(LB, "sw", m, n, scoring)
    D = _run(pl, A, B, dev)
    st = _tall_sw(m, scoring, wins)
    _check_windows(_plane(pl, D, 15), st["rows"], scoring)
    r = pl.results()[0]
    assert (r["score"], tuple(r["end"])) == (st["score"], st["end"])
    tb = pl.traceback(D)
    o = oracle.sw(A, B, *scoring, want_tb=True)
    assert (r["score"], tuple(r["end"]), tuple(tb["beg"]), tb["cigar"]) == \
        (o["score"], tuple(o["end"]), tuple(o["beg"]), o["cigar"])
    assert FR.sw_rescore(A, B, tb["beg"], tb["ops"], scoring) == (st["score"], st["end"])
    assert pl.error() == 0


def test_fill_launch_two_segments_gotoh(dev, LB):
    """fill_block_got2<1> restarted from SNAP at phase 32: the row windows and fin against gotoh_stream, and the
    device walk against the Python walker over the bottom rows, which it leaves at column 0."""
    gh = FR.GOTOH_GH[0]
    m, n, wins = _tall(dev)
    A, B = FR.tall_pair(m)
    pl = _tall_plan(LB, "gotoh", m, n, gh)
    D = _run(pl, A, B, dev)
    st = _tall_gotoh(m, gh, wins)
    _check_windows(_plane(pl, D, 63), st["rows"], gh)
    assert tuple(int(x) for x in pl.results()[0]["fin"]) == st["fin"]
    lo = wins[1][0]
    ops, stop = FR.gotoh_walk(st["rows"][wins[1]], st["fin"], m, n, i0=lo)
    assert stop[1] == 0 and stop[0] >= lo
    tb = pl.traceback_gotoh(D, end_type=-1)
    assert (tb["ops"], tuple(tb["stop"])) == (ops, stop)
    assert pl.error() == 0


# ---- c. one plan, two inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sw_floorless", "sw_floor", "gotoh"])
def test_one_plan_two_inputs(oracle, dev, LB, which):
    """The second run of a plan writes the second input's bytes: the equal pair first (the largest values in the
    granules and SNAP), then a random one."""
    m, n = FR.REUSE_SHAPE
    inputs = [("equal", 0), ("random", 1)]
    if which == "gotoh":
        gh = FR.GOTOH_GH[0]
        pl = _plan(LB, "gotoh", m, n, gh)
        for kind, salt in inputs:
            case = _gotoh_case(oracle, kind, m, n, gh, salt)
            _check_gotoh(pl, _run(pl, case[0], case[1], dev), case, (which, kind))
    else:
        scoring = FR.SW_SCORINGS[0 if which == "sw_floorless" else 1]
        pl = _plan(LB, "sw", m, n, scoring)
        for kind, salt in inputs:
            A, B, ref = FR.sw_case(kind, m, n, scoring, salt)
            _check_sw(pl, _run(pl, A, B, dev), A, B, scoring, ref, (which, kind))
