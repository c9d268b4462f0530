"""Every kernel family on inputs that use all eight symbol codes (Smith-Waterman: seven, code 7 being its virtual
column code), and the global-alignment plans on edge shapes.

A cell's score is one byte of the row's 8-byte profile: codes 0-3 pick from its low dword, codes 4-7 from its high
dword.  ACGT inputs never read the high dword, the `else hi = ...` branch of the profile builders, steps 5-7 of the
NW_SCORED select chain or rows / columns 5-7 of a plan's table.  The inputs are tests/alphabet8.py's (seeded;
test_alphabet8_inputs.py shows on the CPU that every symbol and every table entry decides the expected result); the
checks are the existing ones of test_gpu_parity.py, test_gpu_nw_align.py and test_gpu_nw_scored.py, reused.  Every
test asserts the kernel family it reached (launch_info / format_info / rows_per_lane); a host entry is shown by a
twin plan of the description the entry creates.  Integer DP: every comparison is exact.

Found by this file: the reference-Gotoh flow kernel scored the column code 7 as 0 against every row
(fl_profile_got cleared that profile byte as a "virtual code", which only the Smith-Waterman kernels have), so an
eight-symbol pair got wrong tables, tag bytes and a wrong printed alignment.  Before the fix
test_gotoh_flow_dir_bytes[got_65x66, g = 1, h = 2] had the flow kernel's final cell (65, 66) at (T1, T2, T3) =
(-12, -16, -15) where the stripe kernel and the oracle have (6, 5, 1); 1,424 of its 4,290 tag bytes differed from
the oracle's, the first at cell (2, 2) (row G, column K = code 7: 47 for 63).  test_main_alignment_text,
test_subproblem_nodes and test_gotoh_flow_fill_launch failed with it (main_65x66: score -14 for 8)."""
import functools

import numpy as np
import pytest

import alphabet8 as A8
import nw_reference as R
import nw_scored_reference as RS
import test_gpu_nw_align as NA
import test_gpu_nw_scored as NS
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

ALPHABET = -2
SWL_SCORINGS = [(2, -1, 1), (1, 0, 1)]          # floored (virtual score -100) and floor-free (virtual score 0)
SWA_SCORINGS = [(2, -3, 5, 2), (1, 0, 3, 1)]
SC8 = (A8.AL8, A8.TABLE8, A8.G8, A8.H8)         # alphabet, S, g, h of the NW_SCORED cases
IDENT8 = RS.match_mismatch(A8.AL8, 1, 0)


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _dev8(x, dev):
    import torch

    return torch.from_numpy(A8.enc8(x)).to(dev)


def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def _offs(lens):
    return np.concatenate(([0], np.cumsum(lens)[:-1]))


# ---- Smith-Waterman, linear gap ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sw(name, sc, **kw):
    from oracle import oracle as O

    A, B = A8.named(name)
    return O.sw(A, B, *sc, **kw)


@pytest.mark.parametrize("scoring", SWL_SCORINGS)
@pytest.mark.parametrize("name", ["swl_65x100", "swl_130x70"])
def test_sw_linear_stripe(oracle, dev, LB, name, scoring):
    """The stripe kernel as a one-pair batch (H cells, score, end cell, checksum) and as a single pair that wants
    the end cell without cells."""
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ma, mi, g = scoring
    A, B = A8.named(name)
    o = _sw(name, (ma, mi, g, g), want_h=True)
    dA, dB = _dev8(A, dev), _dev8(B, dev)
    pl = Plan(LB.SW_LINEAR, LB.CELLS_H, [len(A)], [len(B)], [0], [0], match=ma, mismatch=mi, gap_open=g,
              gap_extend=g, track_end=True, single=False)
    assert pl.launch_info()["mode"] == "stripe" and pl.format_info()["values"] == "int32"
    H = torch.empty(pl.cells_elems, dtype=torch.int32, device=dev)
    pl.run(dA, dB, H)
    res = pl.results()[0]
    assert res["score"] == o["score"] and tuple(res["end"]) == tuple(o["end"])
    Hd = pl.deskew(H.cpu().numpy(), 0, pl.stripe_meta())
    bad = np.argwhere(Hd[1:, 1:] != o["H"][1:, 1:])
    assert len(bad) == 0, (len(bad), bad[:4] + 1)
    assert pl.checksum(H) == oracle.checksum_h(o["H"])
    one = Plan(LB.SW_LINEAR, LB.CELLS_NONE, [len(A)], [len(B)], [0], [0], match=ma, mismatch=mi, gap_open=g,
               gap_extend=g, track_end=True, single=True)
    assert one.launch_info()["mode"] == "stripe"
    one.run(dA, dB)
    res = one.results()[0]
    assert res["score"] == o["score"] and tuple(res["end"]) == tuple(o["end"])
    assert pl.error() == 0 and one.error() == 0


@pytest.mark.parametrize("scoring", SWL_SCORINGS)
def test_sw_linear_flow(oracle, dev, LB, scoring):
    """The two-pass flow kernel: H cells of a 1500 x 1203 pair (two rows per lane), and pass 1 alone (score only)."""
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ma, mi, g = scoring
    A, B = A8.named("swl_flow_1500x1203")
    o = _sw("swl_flow_1500x1203", (ma, mi, g, g), want_h=True)
    pl = Plan(LB.SW_LINEAR, LB.CELLS_H, [len(A)], [len(B)], [0], [0], match=ma, mismatch=mi, gap_open=g,
              gap_extend=g, track_end=True, single=True)
    assert pl.launch_info()["mode"] == "flow" and pl.geom[0].rows_per_lane == 2
    H = torch.empty(pl.cells_elems, dtype=torch.int32, device=dev)
    pl.run(_dev8(A, dev), _dev8(B, dev), H)
    res = pl.results()[0]
    assert res["score"] == o["score"] and tuple(res["end"]) == tuple(o["end"])
    bad = np.argwhere(pl.deskew(H.cpu().numpy(), 0, pl.stripe_meta())[1:, 1:] != o["H"][1:, 1:])
    assert len(bad) == 0, (len(bad), bad[:4] + 1)
    assert pl.checksum(H) == oracle.checksum_h(o["H"])
    A, B = A8.named("swl_score_300x1200")
    p1 = Plan(LB.SW_LINEAR, LB.CELLS_NONE, [len(A)], [len(B)], [0], [0], match=ma, mismatch=mi, gap_open=g,
              gap_extend=g, track_end=False, single=True)
    assert p1.launch_info()["mode"] == "flow"
    p1.run(_dev8(A, dev), _dev8(B, dev))
    assert p1.results()[0]["score"] == _sw("swl_score_300x1200", (ma, mi, g, g))["score"]
    assert pl.error() == 0 and p1.error() == 0


@pytest.mark.parametrize("c4_kernel", sorted(P.C4_KERNELS))
@pytest.mark.parametrize("scoring", [(1, 0, 1), (5, 2, 3)])
def test_sw_linear_packed_couples(oracle, dev, LB, scoring, c4_kernel, monkeypatch):
    """Packed int16 couples on cflow_kernel and on the lock-step stripe kernel (forced per plan)."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    monkeypatch.setenv("MSA_C4_KERNEL", c4_kernel)
    ma, mi, g = scoring
    As, Bs, ao, bo, Bcat = A8.packed_batch()
    pl = Plan(LB.SW_LINEAR, LB.CELLS_NONE, [len(a) for a in As], [len(b) for b in Bs], ao, bo, match=ma,
              mismatch=mi, gap_open=g, gap_extend=g, single=False)
    assert pl.launch_info()["mode"] in P.C4_KERNELS[c4_kernel] and pl.format_info()["values"] == "packed16"
    pl.run(_dev8(b"".join(As), dev), _dev8(Bcat, dev))
    res = pl.results()
    for k, (A, B) in enumerate(zip(As, Bs)):
        assert res[k]["score"] == oracle.sw(A, B, ma, mi, g, g)["score"], (k, len(A), len(B))
    assert pl.error() == 0


@pytest.mark.parametrize("kind", ["packed", "packed_lockstep"])
def test_sw_linear_split_batch(oracle, dev, LB, kind, monkeypatch):
    """37 packed pairs against one B: fewer couples than two per CU, so every pair is split into chained items."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    if kind == "packed_lockstep":
        monkeypatch.setenv("MSA_C4_KERNEL", "lockstep")
    As, B = A8.split_batch()
    K, m, n = len(As), len(As[0]), len(B)
    pl = Plan(LB.SW_LINEAR, LB.CELLS_NONE, [m] * K, [n] * K, [k * m for k in range(K)], [0] * K, match=1, mismatch=0,
              gap_open=1, gap_extend=1, single=False)
    assert pl.launch_info()["mode"] == ("cflow" if kind == "packed" else "split")
    assert pl.format_info()["values"] == "packed16"
    pl.run(_dev8(b"".join(As), dev), _dev8(B, dev))
    res = pl.results()
    for k in range(K):
        assert res[k]["score"] == oracle.sw(As[k], B, 1, 0, 1, 1)["score"], k
    assert pl.error() == 0


# ---- Smith-Waterman, affine gap ------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", SWA_SCORINGS)
@pytest.mark.parametrize("name,m,n", [("swa_65x70", 65, 70), ("swa_300x257", 300, 257)])
def test_sw_affine_dir_bytes(oracle, dev, LB, name, m, n, scoring):
    """test_sw_affine_flow_dir_bytes' comparison (flow kernel against the stripe kernel's one-pair batch, every
    byte) and both kernels' score and end cell against the oracle."""
    pl = P.check_sw_affine_flow_dir_bytes(dev, LB, m, n, scoring, pair=A8.named(name), to_dev=_dev8)
    info = pl.launch_info()
    assert info["mode"] == "flow" and info["rows_per_lane"] == 2, info
    r = pl.results()[0]
    o = oracle.sw(*A8.named(name), *scoring)
    assert (r["score"], tuple(r["end"])) == (o["score"], tuple(o["end"]))


@pytest.mark.parametrize("scoring", SWA_SCORINGS)
def test_sw_affine_walks(oracle, dev, LB, scoring):
    """The single walker over a flow fill, and the stripe kernel's batch bytes under the per-pair and the batch
    walker: begin cell and CIGAR against the oracle's traceback."""
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ma, mi, go, ge = scoring
    A, B = A8.named("swa_300x257")
    pl = Plan(LB.SW_AFFINE, LB.CELLS_DIR, [len(A)], [len(B)], [0], [0], match=ma, mismatch=mi, gap_open=go,
              gap_extend=ge, track_end=True)
    assert pl.launch_info()["mode"] == "flow"
    D = torch.empty(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev8(A, dev), _dev8(B, dev), D)
    tb, r, o = pl.traceback(D), pl.results()[0], oracle.sw(A, B, *scoring, want_tb=True)
    assert (r["score"], tuple(r["end"]), tuple(tb["beg"]), tb["cigar"]) == \
        (o["score"], tuple(o["end"]), tuple(o["beg"]), o["cigar"])
    pairs = A8.named("swa_batch")
    ms, ns = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    bp = Plan(LB.SW_AFFINE, LB.CELLS_DIR, ms, ns, _offs(ms), _offs(ns), match=ma, mismatch=mi, gap_open=go,
              gap_extend=ge, track_end=True, single=False)
    assert bp.launch_info()["mode"] == "stripe"
    D = torch.empty(bp.cells_elems, dtype=torch.uint8, device=dev)
    bp.run(_dev8(b"".join(a for a, _ in pairs), dev), _dev8(b"".join(b for _, b in pairs), dev), D)
    res, walks = bp.results(), bp.traceback_batch(D)
    for k, (A, B) in enumerate(pairs):
        o = oracle.sw(A, B, *scoring, want_tb=True)
        one = bp.traceback(D, pair=k)
        assert (res[k]["score"], tuple(res[k]["end"])) == (o["score"], tuple(o["end"])), k
        assert (tuple(one["beg"]), one["cigar"]) == (tuple(o["beg"]), o["cigar"]), k
        assert (tuple(walks[k]["beg"]), walks[k]["cigar"]) == (tuple(o["beg"]), o["cigar"]), k
    assert pl.error() == 0 and bp.error() == 0


# ---- the reference's Gotoh -----------------------------------------------------------------------------------
@pytest.mark.parametrize("gh", [(1, 2), (3, 5)])
@pytest.mark.parametrize("name,m,n", [("got_65x66", 65, 66), ("got_129x700", 129, 700)])
def test_gotoh_flow_dir_bytes(oracle, dev, LB, name, m, n, gh):
    """The tagged flow kernel on eight codes: test_gotoh_flow_dir_bytes' comparison with the stripe kernel, then
    every tag byte against the one derived from the oracle's tables."""
    import torch

    A, B = A8.named(name)
    pl = P.check_gotoh_flow_dir_bytes(dev, LB, gh, m, n, pair=(A, B), to_dev=_dev8)
    assert pl.launch_info()["mode"] == "flow" and pl.format_info()["values"] == "tagged4"
    g, h = gh
    T1, T2, T3, inv = oracle.subproblem_tables(A, B, -1, float(g), float(h))
    assert not inv
    D = torch.empty(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev8(A, dev), _dev8(B, dev), D)
    assert tuple(float(x) for x in pl.results()[0]["fin"]) == tuple(float(T[m, n]) for T in (T1, T2, T3))
    d = pl.deskew_dir(D.cpu().numpy(), 0, pl.stripe_meta())
    bad = np.argwhere((d[1:, 1:] & 63) != P._gotoh_tags(T1, T2, T3, float(g), float(h)))
    assert len(bad) == 0, (len(bad), bad[:4] + 1)
    assert pl.error() == 0


def _ref_twin(LB, m, n, cells, start_type, alg=None):
    """The plan a host entry of the reference API creates for an m x n pair (run_one / run_ref_walk)."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    if alg == LB.PARTIAL:
        return Plan(LB.PARTIAL, cells, [m], [n], [0], [0], match=0, mismatch=1, gap_open=3, gap_extend=1,
                    start_type=start_type, single=True)
    return Plan(LB.REF_GOTOH, cells, [min(m, n)], [max(m, n)], [0], [0], match=1, mismatch=0, gap_open=3,
                gap_extend=1, start_type=start_type, single=True)


@pytest.mark.parametrize("name", ["main_65x66", "main_300x290"])
def test_main_alignment_text(oracle, dev, LB, name):
    """msa_main_alignment on eight symbols: the fill is the tagged flow kernel, the eighth symbol seen has code 7."""
    from cse305_parallel_sequence_alignment_amd import api

    A, B = A8.named(name)
    twin = _ref_twin(LB, len(A), len(B), LB.CELLS_DIR, -1)
    assert twin.launch_info()["mode"] == "flow" and twin.format_info()["values"] == "tagged4"
    assert api.main_alignment_text(b"\0" + A, b"\0" + B, len(A), len(B), 8, 1, 2) == \
        oracle.main_alignment_text(A, B, 1.0, 2.0)


@pytest.mark.parametrize("en", [-1, 2])
@pytest.mark.parametrize("name", ["main_65x66", "main_300x290"])
def test_subproblem_nodes(oracle, dev, LB, name, en):
    """msa_subproblem's node list (find_alignment's walk over the flow kernel's bytes), end types -1 and 2."""
    from cse305_parallel_sequence_alignment_amd import api

    A, B = A8.named(name)
    o = oracle.subproblem_align(A, B, -1, en, 1.0, 2.0)
    sp = api.Subproblem(b"\0" + A, b"\0" + B, len(A), len(B), 0, 0, 1, -1, en, 1, 2)
    sp.find_alignment()
    assert sp.alignment_list() == o["nodes"]
    assert sp.alignment_end.as_tuple() == o["end"]


def test_gotoh_flow_fill_launch(oracle, dev, LB):
    """The separate pass-2 launch (flow_fill_kernel) of a 70,000 x 300 pair."""
    pl = P.check_flow_fill_launch_tall_pair(oracle, dev, LB, "gotoh", pair=A8.tall_pair8(*P.TALL_PAIR),
                                            to_dev=_dev8)
    info = pl.launch_info()
    assert info["mode"] == "flow" and info["fill_grid"] > 0 and pl.format_info()["values"] == "tagged4", info


@pytest.mark.parametrize("st", [-1, 2, -3])
@pytest.mark.parametrize("name", ["sub_65x70", "sub_129x129"])
def test_subproblem_tables(oracle, dev, LB, name, st):
    """The stripe kernel's three table planes (msa_subproblem with tables) for three start types."""
    from cse305_parallel_sequence_alignment_amd import api

    A, B = A8.named(name)
    m, n = len(A), len(B)
    twin = _ref_twin(LB, m, n, LB.CELLS_TAB, st)
    assert twin.launch_info()["mode"] == "stripe" and twin.format_info()["values"] == "int32"
    sp = api.Subproblem(b"\0" + A, b"\0" + B, m, n, 0, 0, 1, st, -1, 1, 2)
    sp.compute_tables()
    for k, (x, y) in enumerate(zip((sp.T1, sp.T2, sp.T3), oracle.subproblem_tables(A, B, st, 1.0, 2.0)[:3])):
        bad = np.argwhere(x != y)
        assert len(bad) == 0, (f"T{k + 1}", len(bad), bad[:4])


def test_partial(oracle, dev, LB):
    """msa_partial_tables (forward and reverse fills) and msa_partial_partition at 130 x 129, p = 4."""
    from cse305_parallel_sequence_alignment_amd import api

    A, B = A8.named("partial_130x129")
    m, n = len(A), len(B)
    twin = _ref_twin(LB, m, n, LB.CELLS_TAB, 1, alg=LB.PARTIAL)
    assert twin.launch_info()["mode"] == "stripe" and twin.format_info()["values"] == "int32"
    T, Rv = api.partial_tables(A, B, m, n, 1, 2, 1, 1)
    To, Ro = oracle.partial_tables(A, B, 1.0, 2.0, 1, 1)
    for k, (x, y) in enumerate(zip(T + Rv, To + Ro)):
        bad = np.argwhere(x != y)
        assert len(bad) == 0, (k, len(bad), bad[:4])
    got = [a.as_tuple() for a in api.findPartialBalancedPartitionParallel(A, B, m, n, 4, 1, 2, 1, 1)]
    assert got == oracle.partial_partition(A, B, 4, 1.0, 2.0, 1, 1)


# ---- global alignment ----------------------------------------------------------------------------------------
def test_nw_banded_h_cells(oracle, dev, LB):
    """band_kernel writing H (NW_BANDED) at 300 x 290, band 32: every in-band cell."""
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    A, B = A8.named("banded_300x290")
    m, n, w = len(A), len(B), 32
    pl = Plan(LB.NW_BANDED, LB.CELLS_H, [m], [n], [0], [0], match=1, mismatch=0, gap_open=3, gap_extend=1, band=w)
    assert pl.launch_info()["mode"] == "band"
    H = torch.empty(pl.cells_elems, dtype=torch.int32, device=dev)
    pl.run(_dev8(A, dev), _dev8(B, dev), H)
    score, Ho = oracle.banded_ref(A, B, w, 1.0, 2.0, want_h=True)
    Hd = pl.deskew(H.cpu().numpy(), 0, pl.stripe_meta())
    i, j = np.indices(Ho.shape)
    inb = (np.abs(i - j) <= w) & (i > 0) & (j > 0)
    bad = np.argwhere(inb & (Hd != Ho))
    assert len(bad) == 0, (len(bad), bad[:4])
    assert pl.checksum(H) == oracle.checksum_h(Ho, w)
    assert pl.results()[0]["score"] == int(score) and pl.error() == 0


def _nw_align_fill(LB, dev, A, B, band, g, h):
    import torch

    pl = NA._plan(LB, [len(A)], [len(B)], [0], [0], band, g, h)
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev8(A, dev), _dev8(B, dev), dDir)
    return pl, dDir


@pytest.mark.parametrize("name,band,mode", [("banded_300x290", 32, "band"), ("nw_500x480", -1, "stripe")])
def test_nw_align(oracle, dev, LB, name, band, mode):
    """NW_ALIGN (+1 / 0) on eight symbols: test_gpu_nw_align.py's checks against nw_reference."""
    A, B = A8.named(name)
    pl, dDir = _nw_align_fill(LB, dev, A, B, band, 1, 2)
    assert pl.launch_info()["mode"] == mode
    NA._check(oracle, pl, dDir, A, B, band, 1, 2, R.nw_reference(A, B, 1, 2, band))


@functools.lru_cache(maxsize=None)
def _scored(seed_or_name, band, wide=False, g=A8.G8, h=A8.H8):
    """(A, B, reference) of an NW_SCORED case, computed once and shared (never modified)."""
    A, B = A8.named(seed_or_name) if isinstance(seed_or_name, str) else A8.pair8(seed_or_name, 300, 290)
    S = A8.TABLE8_WIDE if wide else A8.TABLE8
    return A, B, RS.nw_scored_reference(A, B, A8.AL8, S, g, h, band)


def test_nw_scored_band_exact(dev, LB):
    """band_kernel under the dense table (the input test_alphabet8_inputs.py proves sensitive to all 64 entries)."""
    A, B, ref = _scored(5, 32)
    pl, dDir = NS._fill(LB, dev, A, B, 32, *SC8)
    assert pl.launch_info()["mode"] == "band" and pl.run_info()["mode"] == "stripe"
    NS._check(pl, dDir, A, B, 32, *SC8, ref)


def test_nw_scored_stripe_single(dev, LB):
    A, B, ref = _scored("nw_500x480", -1)
    pl, dDir = NS._fill(LB, dev, A, B, -1, *SC8)
    assert pl.launch_info()["mode"] == "stripe"
    NS._check(pl, dDir, A, B, -1, *SC8, ref)


@pytest.mark.parametrize("band", [64, -1])
def test_nw_scored_stripe_batch(dev, LB, band):
    pairs = A8.batch8(91, R.BATCH_MS, R.BATCH_NS)
    pl, dDir = NS._batch_fill(LB, dev, pairs, band, *SC8)
    assert pl.launch_info()["mode"] == "stripe"
    NS._check_batch(pl, dDir, pairs, band, *SC8)


def test_nw_scored_band_chunked(dev, LB):
    """similar_9001_w64's scheme over eight symbols: the chunked launch (or the exact one behind it) writes the
    bytes."""
    A, B = A8.chunked8()
    ref = RS.nw_scored_reference(A, B, *SC8, 64)
    pl, dDir = NS._fill(LB, dev, A, B, 64, *SC8)
    pl.results()
    info = pl.run_info()
    print(f"chunked8: converged = {info['converged']}, chunks = {info['chunks']}")
    assert pl.launch_info()["mode"] == "band_chunked"
    assert info["mode"] == "chunked" and info["chunks"] >= 4 and info["int16_cells"] == 0, info
    NS._check(pl, dDir, A, B, 64, *SC8, ref)


@pytest.mark.parametrize("band,mode", [(32, "band"), (-1, "stripe")])
def test_nw_scored_score_only(dev, LB, band, mode):
    A, B, ref = _scored(5, band)
    pl = NS._plan(LB, [len(A)], [len(B)], [0], [0], band, A8.TABLE8, A8.G8, A8.H8, cells=LB.CELLS_NONE)
    assert pl.cells_elems == 0 and pl.launch_info()["mode"] == mode
    pl.run(_dev8(A, dev), _dev8(B, dev))
    assert pl.results()[0]["score"] == ref["score"] and pl.error() == 0


@pytest.mark.parametrize("g,h,mode", [(1, 2, "band"), (20, 10, "stripe")])
def test_nw_scored_wide_table(dev, LB, g, h, mode):
    """TABLE8_WIDE's largest entry is 80: band_kernel's profile byte S + 2g + h is 84 under g = 1, h = 2 and 130
    under g = 20, h = 10, which must take the exact stripe launch."""
    A, B, ref = _scored(5, 32, wide=True, g=g, h=h)
    pl, dDir = NS._fill(LB, dev, A, B, 32, A8.AL8, A8.TABLE8_WIDE, g, h)
    assert pl.launch_info()["mode"] == mode
    NS._check(pl, dDir, A, B, 32, A8.AL8, A8.TABLE8_WIDE, g, h, ref)


@pytest.mark.parametrize("band,mode", [(32, "band"), (-1, "stripe")])
@pytest.mark.parametrize("perm", A8.PERMS, ids=["swap07", "mixed"])
def test_nw_scored_code_permutation(dev, LB, perm, band, mode):
    """Renaming the codes (rows and columns of the table with them) changes nothing: the same score, the same
    byte at every cell and the same ops."""
    import torch

    A, B = A8.pair8(5, 300, 290)
    out = []
    for p in (tuple(range(8)), perm):
        pl = NS._plan(LB, [len(A)], [len(B)], [0], [0], band, A8.permuted(p, S=A8.TABLE8), A8.G8, A8.H8)
        assert pl.launch_info()["mode"] == mode
        dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
        pl.run(torch.from_numpy(A8.permuted(p, codes=A8.enc8(A))).to(dev),
               torch.from_numpy(A8.permuted(p, codes=A8.enc8(B))).to(dev), dDir)
        tb = pl.traceback_nw(dDir)
        out.append((pl.results()[0]["score"], pl.deskew_dir(dDir.cpu().numpy(), 0, pl.stripe_meta()), tb["ops"],
                    tb["stop"]))
        assert pl.error() == 0
    (s0, d0, o0, e0), (s1, d1, o1, e1) = out
    assert s0 == s1 and o0 == o1 and e0 == e1
    # every in-band interior cell, all eight bits (what a band plan leaves outside the band is not specified)
    w = R.band_width(len(A), len(B), band)
    _, valid = R.band_cols(len(A), len(B), w)
    bad = np.argwhere(valid & (R.to_band(d0, w) != R.to_band(d1, w)))
    assert valid.sum() > 0 and len(bad) == 0, (len(bad), bad[:4])


# ---- host entries --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [32, -1])
def test_host_nw_align(oracle, dev, LB, band):
    """api.nw_align / nw_align_batch under alphabet = AL8 and the dense table, and msa_nw_align (+1 / 0), whose
    own symbol map hands out codes 4-7."""
    from cse305_parallel_sequence_alignment_amd import api

    A, B, ref = _scored(5, band)
    kw = dict(alphabet=A8.AL8, matrix=A8.TABLE8, gap_open=A8.G8 + A8.H8, gap_extend=A8.G8, band=band)
    assert api.nw_align(A, B, **kw) == dict(score=ref["score"], cigar=R.cigar_of(ref["ops"]))
    assert api.nw_align(A, B, traceback=False, **kw) == dict(score=ref["score"])
    pairs = A8.batch8(91, R.BATCH_MS, R.BATCH_NS)
    kw["band"] = 64 if band >= 0 else -1
    got = api.nw_align_batch([a for a, _ in pairs], [b for _, b in pairs], **kw)
    for (a, b), r in zip(pairs, got):
        o = RS.nw_scored_reference(a, b, *SC8, kw["band"])
        assert r == dict(score=o["score"], cigar=R.cigar_of(o["ops"]))
    A, B = A8.named("nw10_300x290")
    o = R.nw_reference(A, B, 1, 2, band)
    assert o["score"] == int(oracle.banded_ref(A, B, o["w"], 1.0, 2.0))
    assert api.nw_align(A, B, gap_open=3, gap_extend=1, band=band) == dict(score=o["score"],
                                                                          cigar=R.cigar_of(o["ops"]))


@pytest.mark.parametrize("scoring", SWA_SCORINGS)
def test_host_sw_align(oracle, dev, LB, scoring):
    """msa_sw_align / msa_sw_align_batch with seven symbols (codes 0-6); an eighth is MSA_ERR_ALPHABET."""
    from cse305_parallel_sequence_alignment_amd import api

    A, B = A8.named("swa_300x257")
    assert len(set(A + B)) == 7
    o = oracle.sw(A, B, *scoring, want_tb=True)
    r = api.sw_align(A, B, *scoring)
    assert (r["score"], r["end"], r["beg"], r["cigar"]) == (o["score"], o["end"], o["beg"], o["cigar"])
    pairs = A8.named("swa_batch")
    got = api.sw_align_batch([a for a, _ in pairs], [b for _, b in pairs], *scoring)
    for (a, b), r in zip(pairs, got):
        o = oracle.sw(a, b, *scoring, want_tb=True)
        assert (r["score"], r["end"], r["beg"], r["cigar"]) == (o["score"], o["end"], o["beg"], o["cigar"])
    assert _status(lambda: api.sw_align(A + b"K", B, *scoring)) == ALPHABET
    assert _status(lambda: api.sw_align_batch([a for a, _ in pairs], [b + b"K" for _, b in pairs], *scoring)) \
        == ALPHABET


# ---- edge shapes of NW_ALIGN / NW_SCORED ---------------------------------------------------------------------
EDGE_CASES = [(s, (A8.G8, A8.H8)) for s in A8.EDGE_SHAPES] + A8.EDGE_EXTRA


def _consumed(cigar):
    import re

    runs = [(int(k), op) for k, op in re.findall(r"(\d+)([MID])", cigar)]
    return sum(k for k, op in runs if op in "MI"), sum(k for k, op in runs if op in "MD")


@pytest.mark.parametrize("shape,gh", EDGE_CASES, ids=[f"{s[0]}x{s[1]}_w{s[2]}_g{g}h{h}" for s, (g, h) in EDGE_CASES])
def test_edge_shape(oracle, dev, LB, shape, gh):
    """Fewer rows than a stripe, exactly 64 or 128 rows, one row or one column, band 0, walks that stop at a
    border cell with a long border gap: the full comparison under the dense table (NW_SCORED) and under +1 / 0
    (NW_ALIGN), and the host entries' CIGARs, which must consume exactly m and n."""
    from cse305_parallel_sequence_alignment_amd import api

    (m, n, band), (g, h) = shape, gh
    A, B = A8.edge_pair(m, n)
    ref = RS.nw_scored_reference(A, B, A8.AL8, A8.TABLE8, g, h, band)
    pl, dDir = NS._fill(LB, dev, A, B, band, A8.AL8, A8.TABLE8, g, h)
    assert pl.launch_info()["mode"] in ("band", "stripe")
    NS._check(pl, dDir, A, B, band, A8.AL8, A8.TABLE8, g, h, ref)
    r = api.nw_align(A, B, alphabet=A8.AL8, matrix=A8.TABLE8, gap_open=g + h, gap_extend=g, band=band)
    assert r == dict(score=ref["score"], cigar=R.cigar_of(ref["ops"])) and _consumed(r["cigar"]) == (m, n)
    ref = R.nw_reference(A, B, g, h, band)
    pl, dDir = _nw_align_fill(LB, dev, A, B, band, g, h)
    assert pl.launch_info()["mode"] in ("band", "stripe")
    NA._check(oracle, pl, dDir, A, B, band, g, h, ref)
    r = api.nw_align(A, B, gap_open=g + h, gap_extend=g, band=band)
    assert r == dict(score=ref["score"], cigar=R.cigar_of(ref["ops"])) and _consumed(r["cigar"]) == (m, n)


@pytest.mark.parametrize("band", sorted({s[2] for s in A8.EDGE_SHAPES}))
def test_edge_shapes_batch(oracle, dev, LB, band):
    """The edge shapes of one band value as one ragged batch: every pair's checks and the one-launch batch walk,
    under the dense table and under +1 / 0."""
    import torch

    pairs = [A8.edge_pair(m, n) for m, n, w in A8.EDGE_SHAPES if w == band]
    if len(pairs) == 1:
        pairs.append(A8.edge_pair(6, 6))  # (a plan of one pair would be a single-pair plan)
    pl, dDir = NS._batch_fill(LB, dev, pairs, band, *SC8)
    assert pl.launch_info()["mode"] == "stripe"
    NS._check_batch(pl, dDir, pairs, band, *SC8)
    ms, ns = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    pl = NA._plan(LB, ms, ns, _offs(ms), _offs(ns), band, A8.G8, A8.H8)
    assert pl.launch_info()["mode"] == "stripe"
    dDir = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev8(b"".join(a for a, _ in pairs), dev), _dev8(b"".join(b for _, b in pairs), dev), dDir)
    singles = [NA._check(oracle, pl, dDir, a, b, band, A8.G8, A8.H8, R.nw_reference(a, b, A8.G8, A8.H8, band), pair=k)
               for k, (a, b) in enumerate(pairs)]
    for one, tb in zip(singles, pl.traceback_batch(dDir)):
        assert (tb["ops"], tb["stop"], tb["cigar"]) == (one["ops"], one["stop"], one["cigar"])
