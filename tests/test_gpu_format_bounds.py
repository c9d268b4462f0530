"""Every narrow number format at its admission bound, on worst-case inputs.

Plan creation (csrc/msa_plan.inc) decides on the host whether a pair may run in a narrow format: packed int16
couples, the packed first-maximum key, int8 profile bytes, the x4 tagged Gotoh values, int16 chunk cells.  Each
decision is a hand-derived inequality; a kernel run past what its format holds wraps silently.  Every test here runs
the largest admitted size or score (the format asserted through Plan.format_info()) and the one a step past it (the
wide format asserted), on inputs that reach the bound's maximum in a real cell, and compares with the oracle
exactly: integer DP, no tolerances.  The edges are located by the helpers below, which restate the documented
inequalities; test_case_table_sits_on_the_edges (no GPU) checks the table against them and against the sizes
worked out by hand.
"""
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def enc(s: bytes) -> np.ndarray:
    return np.frombuffer(s.translate(bytes.maketrans(b"ACGT", b"\x00\x01\x02\x03")), dtype=np.uint8).copy()


def rs(rng, n):
    return rng.choice(ACGT, n).tobytes()


def _dev(x, dev):
    import torch

    return torch.from_numpy(enc(x)).to(dev)


# ---- the documented inequalities (msa_plan.inc: choose_algorithm, choose_mode, shape_band) ---------------------
def swlp_ok(m, n, ma, mi, g):
    """Packed int16 couples: G = H + g (i + j) and the profile byte score + 2g stay inside int16 / int8."""
    return g * (m + n + 2) + max(0, ma, mi) * min(m, n) + 2 * g + 127 < 32000 and ma + 2 * g <= 127


def key_ok(m, n, ma, mi):
    """Packed first-maximum key (value << 15) + (32767 - step): scores below 2^16, steps below 2^15."""
    return max(0, ma, mi) * min(m, n) < 65536 and n + 512 < 32768


def ref1_ok(m, n, go, ge):
    """x4 tagged Gotoh values (start type -1): 4 (g + h + 1) (m + n + 2) stays below 2^28."""
    return ge >= 0 and go >= ge and 4 * (go + 1) * (m + n + 2) < (1 << 28)


def affine_flow_ok(ma, mi, go, ge):
    """SW-affine flow kernel: the profile bytes score + open + extend fit int8."""
    return ge >= 0 and go >= ge and max(ma, mi) + go + ge <= 127 and min(ma, mi) + go + ge >= -128


def linear_flow_ok(ma, mi, g):
    """SW-linear flow kernel: with a negative score it runs in X-space, whose profile bytes are score + g."""
    return min(ma, mi) >= 0 or min(ma, mi) + g >= -128


def gotoh_flow_ok(ge):
    """Gotoh flow kernel: the profile bytes 4 (f + 2g) fit int8."""
    return 4 * (1 + 2 * ge) <= 127


def h16_ok(g, h, band, warm=20, chunk=12):
    """int16 chunk cells of the banded kernel at the default warm-up and chunk stripes."""
    return (warm + chunk) * 64 + 64 + h + g * band <= 30000


def largest(ok, hi=1 << 22):
    """The largest x in [1, hi] with ok(x) (ok is monotone: true up to the edge, false past it)."""
    assert ok(1) and not ok(hi)
    lo = 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


# ---- the case table ---------------------------------------------------------------------------------------------
SWLP_SCORINGS = [(47, 0, 40), (5, 2, 3), (1, 0, 1)]  # (match, mismatch, g); the first has match + 2g = 127
SWLP_THIN_M = 193   # 63 padded rows in its last stripe
SWLP_ODD_N = 129    # n = 1 (mod 64)


def swlp_shapes(ma, mi, g):
    """The three shapes at the packed bound: the largest square, the widest at m = 193, the tallest at n = 129."""
    return [(largest(lambda x: swlp_ok(x, x, ma, mi, g)),) * 2,
            (SWLP_THIN_M, largest(lambda x: swlp_ok(SWLP_THIN_M, x, ma, mi, g))),
            (largest(lambda x: swlp_ok(x, SWLP_ODD_N, ma, mi, g)), SWLP_ODD_N)]


def swlp_past(shapes):
    """One step past each shape: one more diagonal step of the square, one more row of the other two."""
    (sq, _), thin, tall = shapes
    return [(sq + 1, sq + 1), (thin[0] + 1, thin[1]), (tall[0] + 1, tall[1])]


# (alg, match, mismatch, gap_open, gap_extend): identical pairs; all-mismatch pairs swap match and mismatch
KEY_SCORINGS = {"linear": (125, 0, 1, 1), "affine": (120, -1, 4, 3)}
KEY_STEP_M, KEY_STEP_SCORING = 70, (2, -1, 1, 1)


def key_square(alg):
    ma, mi, _, _ = KEY_SCORINGS[alg]
    return largest(lambda x: key_ok(x, x, ma, mi))


def key_step_n():
    return largest(lambda x: key_ok(KEY_STEP_M, x, *KEY_STEP_SCORING[:2]))


REF1_GAPS = (32767, 15)  # gap_open = g + h, gap_extend = g


def ref1_shapes():
    """(m, n) at the largest admitted span m + n + 2: the squarest pair and a one-row pair."""
    go, ge = REF1_GAPS
    span = largest(lambda s: ref1_ok(s - 2, 0, go, ge))
    return [((span - 2) // 2, span - 2 - (span - 2) // 2), (1, span - 3)]


BAND_H16 = dict(h=1, band=512)


def test_case_table_sits_on_the_edges():
    """Every 'at the bound' case satisfies its inequality and the next size does not; the sizes are the ones
    worked out by hand for these scorings."""
    for (ma, mi, g) in SWLP_SCORINGS:
        shapes = swlp_shapes(ma, mi, g)
        for (m, n), (m1, n1) in zip(shapes, swlp_past(shapes)):
            assert swlp_ok(m, n, ma, mi, g) and not swlp_ok(m1, n1, ma, mi, g), (ma, mi, g, m, n)
        assert not swlp_ok(SWLP_THIN_M, shapes[1][1] + 1, ma, mi, g)
    assert SWLP_SCORINGS[0][0] + 2 * SWLP_SCORINGS[0][2] == 127
    assert not swlp_ok(4, 4, 48, 0, 40)  # match + 2g = 128
    assert [swlp_shapes(*s)[0][0] for s in SWLP_SCORINGS] == [249, 2896, 10622]
    assert swlp_shapes(47, 0, 40) == [(249, 249), (193, 373), (512, 129)]
    assert SWLP_THIN_M % 64 == 1 and SWLP_ODD_N % 64 == 1
    for alg, want in (("linear", 524), ("affine", 546)):
        ma, mi, _, _ = KEY_SCORINGS[alg]
        L = key_square(alg)
        assert L == want and key_ok(L, L, ma, mi) and not key_ok(L + 1, L + 1, ma, mi)
        assert key_ok(L, L, mi, ma) and not key_ok(L + 1, L + 1, mi, ma)  # all-mismatch: the scores swapped
    assert (125 * 524, 120 * 546) == (65500, 65520)
    n = key_step_n()
    assert n == 32255 and key_ok(KEY_STEP_M, n, 2, -1) and not key_ok(KEY_STEP_M, n + 1, 2, -1)
    for (m, n) in ref1_shapes():
        assert m + n + 2 == 2047 and ref1_ok(m, n, *REF1_GAPS) and not ref1_ok(m, n + 1, *REF1_GAPS), (m, n)
    assert ref1_shapes() == [(1022, 1023), (1, 2044)]
    assert h16_ok(54, **BAND_H16) and not h16_ok(55, **BAND_H16)
    # int8 profile bytes at both ends
    assert affine_flow_ok(100, -128, 20, 7) and not affine_flow_ok(101, -128, 20, 7)
    assert 100 + 20 + 7 == 127 and not affine_flow_ok(127, -128, 3, 1)
    assert gotoh_flow_ok(15) and not gotoh_flow_ok(16)
    (ma, mi, g), (ma1, mi1, g1) = PROFILE_LINEAR
    assert (ma + 2 * g, mi + g) == (127, -128) and linear_flow_ok(ma, mi, g)
    assert (ma1 + 2 * g1, mi1 + 2 * g1) == (127, -128) and not linear_flow_ok(ma1, mi1, g1)


# ---- inputs -----------------------------------------------------------------------------------------------------
def identical_pair(rng, m, n):
    """A and B equal along the diagonal that ends in the last cell: every one of its min(m, n) steps gains the
    match score, so cell (m, n) holds the bound's maximum."""
    if m <= n:
        B = rs(rng, n)
        return B[n - m:], B
    A = rs(rng, m)
    return A, A[m - n:]


def mismatch_pair(rng, m, n):
    return b"A" * m, b"C" * n


def one_mismatch_pair(rng, m, n):
    """identical_pair with one letter of the diagonal changed: the best path crosses a mismatch."""
    A, B = identical_pair(rng, m, n)
    k = len(A) - min(m, n) // 2
    return A[:k] + bytes([ACGT[(list(ACGT).index(A[k]) + 1) % 4]]) + A[k + 1:], B


def late_maximum_pair(rng, m, n):
    """A random B whose last m letters equal A: the first maximum lies at the largest step index."""
    B = rs(rng, n)
    return B[n - m:], B


INPUTS = {"identical": identical_pair, "all_mismatch": mismatch_pair, "one_mismatch": one_mismatch_pair}


# ---- the references, computed once per distinct input -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sw(A, B, ma, mi, go, ge, want_h=False, want_tb=False):
    from oracle import oracle as O

    return O.sw(A, B, ma, mi, go, ge, want_h=want_h, want_tb=want_tb)


@functools.lru_cache(maxsize=None)
def _gotoh(A, B, g, h):
    """The reference's double tables and node list (start / end type -1), the tag fields of every cell
    (find_alignment's first maximum among T1, T2, T3: table k), and the walk's ops end -> start."""
    from oracle import oracle as O

    o = O.subproblem_align(A, B, -1, -1, float(g), float(h))
    assert not o["invert"]
    T1, T2, T3 = o["T1"], o["T2"], o["T3"]

    def first(c):
        return np.argmax(np.stack(c), axis=0).astype(np.uint8) + 1

    k1 = first([T1[:-1, :-1], T2[:-1, :-1], T3[:-1, :-1]])
    k2 = first([T1[1:, :-1] - g - h, T2[1:, :-1] - g, T3[1:, :-1] - g - h])
    k3 = first([T1[:-1, 1:] - g - h, T2[:-1, 1:] - g - h, T3[:-1, 1:] - g])
    ts = [t for (_, _, t) in o["nodes"]]
    ops = "".join("MDI"[t - 1] for t in reversed(ts)) if ts else "MDI"[o["end"][2] - 1]
    m, n = len(A), len(B)
    fin = tuple(int(T[m, n]) for T in (T1, T2, T3))
    assert all(abs(x) < (1 << 29) for x in fin)
    return dict(tables=(k1, k2, k3), ops=ops, fin=fin)


def _check_gotoh(pl, dev, A, B, g, h, tagged):
    """Runs a REF_GOTOH direction-byte plan and compares the byte of every cell, the final state, the score and the
    device walk with the reference.  The tagged format stores 4 - k per field, the untagged one the table k."""
    import torch

    m, n = len(A), len(B)
    D = torch.empty(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev(A, dev), _dev(B, dev), D)
    r = pl.results()[0]
    o = _gotoh(A, B, g, h)
    assert tuple(r["fin"]) == o["fin"], (m, n)
    assert r["score"] == max(o["fin"]), (m, n)
    k1, k2, k3 = o["tables"]
    want = (4 - k1) | ((4 - k2) << 2) | ((4 - k3) << 4) if tagged else k1 | (k2 << 2) | (k3 << 4)
    d = pl.deskew_dir(D.cpu().numpy(), 0, pl.stripe_meta())
    assert np.array_equal(d[1:, 1:] & 63, want), (m, n)
    assert pl.traceback_gotoh(D, end_type=-1)["ops"].decode() == o["ops"], (m, n)
    assert pl.error() == 0


def _check_sw(pl, dev, A, B, scoring, cells):
    """Runs a single-pair SW plan with the end cell tracked and compares score, first row-major end cell, and what
    its cells allow -- every H cell, or the device traceback's begin cell and CIGAR -- with the oracle."""
    import torch
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    dt = {LB.CELLS_NONE: None, LB.CELLS_H: torch.int32, LB.CELLS_DIR: torch.uint8}[cells]
    out = None if dt is None else torch.empty(pl.cells_elems, dtype=dt, device=dev)
    pl.run(_dev(A, dev), _dev(B, dev), out)
    r = pl.results()[0]
    o = _sw(A, B, *scoring, want_h=(cells == LB.CELLS_H), want_tb=(cells == LB.CELLS_DIR))
    what = (len(A), len(B), scoring, cells)
    assert r["score"] == o["score"], what
    if o["score"] > 0:  # (a zero maximum has no end cell)
        assert tuple(r["end"]) == tuple(o["end"]), what
    if cells == LB.CELLS_H:
        Hd = pl.deskew(out.cpu().numpy(), 0, pl.stripe_meta())
        assert np.array_equal(Hd[1:, 1:], o["H"][1:, 1:]), what
    if cells == LB.CELLS_DIR and o["score"] > 0:
        tb = pl.traceback(out)
        assert (tuple(tb["beg"]), tb["cigar"]) == (tuple(o["beg"]), o["cigar"]), what
    assert pl.error() == 0
    return o


# ---- a. packed int16 couples ------------------------------------------------------------------------------------
C4_KERNELS = {"cflow": ("cflow",), "lockstep": ("stripe", "split")}


def cflow_fits(n):
    """cflow_kernel holds 8 byte-shifted copies of the code row in LDS (msa_plan.inc, cflow_lds_bytes): wider
    couples run the lock-step kernel whatever MSA_C4_KERNEL says."""
    return (128 + 5 * 256) * 4 + 8 * (((n + 208 + 15) & ~15) + 16) <= 96 * 1024


def _couples(rng, shapes):
    """One couple per shape: an identical pair and a random one (the other int16 half) over one column sequence."""
    As, Bs, ms, ns, ao, bo = [], [], [], [], [], []
    for (m, n) in shapes:
        A0, B = identical_pair(rng, m, n)
        for A in (A0, rs(rng, m)):
            ao.append(sum(ms))
            bo.append(sum(len(b) for b in Bs))
            As.append(A)
            ms.append(m)
            ns.append(n)
        Bs.append(B)
    return As, Bs, ms, ns, ao, bo


def _run_couples(dev, shapes, scoring, seed):
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ma, mi, g = scoring
    As, Bs, ms, ns, ao, bo = _couples(np.random.default_rng(seed), shapes)
    pl = Plan(LB.SW_LINEAR, LB.CELLS_NONE, ms, ns, ao, bo, match=ma, mismatch=mi, gap_open=g, gap_extend=g,
              single=False)
    pl.run(_dev(b"".join(As), dev), _dev(b"".join(Bs), dev))
    res = pl.results()
    for k, A in enumerate(As):
        want = _sw(A, Bs[k // 2], ma, mi, g, g)["score"]
        assert res[k]["score"] == want, (scoring, k, ms[k], ns[k], pl.format_info(), pl.launch_info()["mode"])
        if k % 2 == 0:  # the identical pair reaches the bound's maximum
            assert want == max(ma, mi) * min(ms[k], ns[k])
    assert pl.error() == 0
    return pl


@gpu
@pytest.mark.parametrize("c4_kernel", sorted(C4_KERNELS))
@pytest.mark.parametrize("scoring", SWLP_SCORINGS)
def test_packed_couples_at_the_bound(dev, scoring, c4_kernel, monkeypatch):
    """The three shapes at g (m + n + 2) + smax min(m, n) + 2g + 127 < 32000 -- the largest square, the widest pair
    of 193 rows (63 padded rows), the tallest of 129 columns -- as couples of an identical pair (cell (m, n) holds
    smax min(m, n), the bound's maximum) and a random one, in one plan per kernel: packed int16, every score the
    oracle's.  One step more (a diagonal step of the square, a row of the other two) takes each shape to int32
    values, with the same scores."""
    monkeypatch.setenv("MSA_C4_KERNEL", c4_kernel)
    shapes = swlp_shapes(*scoring)
    seed = 1000 + scoring[0]
    # (couples too wide for cflow's LDS code rows form a plan of their own, which runs the lock-step kernel)
    for fits in (True, False):
        group = [s for s in shapes if cflow_fits(s[1]) == fits]
        if group:
            pl = _run_couples(dev, group, scoring, seed)
            assert pl.format_info()["values"] == "packed16", group
            assert pl.launch_info()["mode"] in C4_KERNELS[c4_kernel if fits else "lockstep"], group
    for past in swlp_past(shapes):
        pl = _run_couples(dev, [past], scoring, seed + 1)
        assert pl.format_info()["values"] == "int32", past


# ---- b. the packed first-maximum key ----------------------------------------------------------------------------
def _sw_plan(alg, cells, m, n, scoring, single=True, track_end=True):
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ma, mi, go, ge = scoring
    return Plan({"linear": LB.SW_LINEAR, "affine": LB.SW_AFFINE}[alg], cells, [m], [n], [0], [0], match=ma,
                mismatch=mi, gap_open=go, gap_extend=ge, track_end=track_end, single=single)


@gpu
@pytest.mark.parametrize("kernel", ["flow", "stripe"])
@pytest.mark.parametrize("inputs", ["identical", "all_mismatch"])
@pytest.mark.parametrize("alg", ["linear", "affine"])
def test_packed_key_score_side(dev, alg, inputs, kernel):
    """smax min(m, n) at the largest value below 2^16 the scoring reaches (linear 125 x 524 = 65,500, affine 120 x
    546 = 65,520), in the last cell of an identical pair, and of an all-mismatch pair with mismatch > match: the
    packed key, through the flow kernel (cells written) and the stripe kernel (no cells).  One more diagonal step
    takes the plan to compare-select tracking.  Score, first row-major end cell and (affine, direction bytes) the
    device traceback equal the oracle's either way."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    ma, mi, go, ge = KEY_SCORINGS[alg]
    if inputs == "all_mismatch":
        ma, mi = mi, ma
    cells = LB.CELLS_NONE if kernel == "stripe" else (LB.CELLS_H if alg == "linear" else LB.CELLS_DIR)
    L = key_square(alg)
    for size, tracking in ((L, "key"), (L + 1, "select")):
        A, B = INPUTS[inputs](np.random.default_rng(size), size, size)
        pl = _sw_plan(alg, cells, size, size, (ma, mi, go, ge))
        assert pl.format_info()["tracking"] == tracking, size
        assert pl.launch_info()["mode"] == kernel, size
        o = _check_sw(pl, dev, A, B, (ma, mi, go, ge), cells)
        assert o["score"] == max(ma, mi) * size and tuple(o["end"]) == (size, size)


@gpu
@pytest.mark.parametrize("kernel", ["flow", "stripe"])
def test_packed_key_step_side(dev, kernel):
    """n + 512 < 32768: 70 x 32,255 packs the step of the first maximum, 70 x 32,256 does not; the maximum lies in
    the last column (B ends in A), at the largest step index a stripe has."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    cells = LB.CELLS_NONE if kernel == "stripe" else LB.CELLS_H
    m, n_at = KEY_STEP_M, key_step_n()
    for n, tracking in ((n_at, "key"), (n_at + 1, "select")):
        A, B = late_maximum_pair(np.random.default_rng(n), m, n)
        pl = _sw_plan("linear", cells, m, n, KEY_STEP_SCORING)
        assert pl.format_info()["tracking"] == tracking, n
        assert pl.launch_info()["mode"] == kernel, n
        o = _check_sw(pl, dev, A, B, KEY_STEP_SCORING, cells)
        assert o["score"] == 2 * m and tuple(o["end"]) == (m, n)


# ---- c. int8 profile bytes --------------------------------------------------------------------------------------
def _leave_codes_in_lds(dev):
    """Runs a single-pair stripe-kernel plan over all-'A' columns: its workgroups leave code 0 in every slot of their
    LDS code rings (n > 2 rings), which is what a later kernel on those CUs finds in slots it does not stage."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    m, n = 300, 2100
    pl = _sw_plan("linear", LB.CELLS_NONE, m, n, (2, -1, 1, 1))
    assert pl.launch_info()["mode"] == "stripe"
    pl.run(_dev(b"A" * m, dev), _dev(b"A" * n, dev))
    assert pl.results()[0]["score"] == 2 * m


PROFILE_SHAPES = [(65, 70), (130, 257)]
# match + 2g = 127 in both; mismatch + g = -128 (the flow kernel's X-space byte), mismatch + 2g = -128 (the stripe
# kernel's G-space byte: one past the flow kernel's bound)
PROFILE_LINEAR = [(125, -129, 1), (125, -130, 1)]


@gpu
@pytest.mark.parametrize("inputs", sorted(INPUTS))
@pytest.mark.parametrize("m,n", PROFILE_SHAPES)
@pytest.mark.parametrize("scoring", PROFILE_LINEAR)
def test_profile_bytes_sw_linear(dev, scoring, m, n, inputs):
    """SW linear's profile bytes at 127 and -128.  The stripe kernel's are score + 2g: mismatch -130 with g = 1 is
    the lowest it takes.  The flow kernel's are score + g when a score is negative: mismatch -129 is the lowest a
    single pair runs there, and -130 (which wrapped to +127 there: an all-mismatch pair scored 126 min(m, n)) runs
    the stripe kernel.  Every H cell, score and end cell of the single pair and of the pair as a batch of one equal
    the oracle's.  (A match worth more than ~68 gaps also shows a stale column code in the virtual columns left of
    column 1: one match there reaches the matrix.)"""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    ma, mi, g = scoring
    A, B = INPUTS[inputs](np.random.default_rng(m), m, n)
    flow = "flow" if linear_flow_ok(ma, mi, g) else "stripe"
    _leave_codes_in_lds(dev)
    # (a single pair without cells but with the end cell runs the stripe kernel as well)
    for single, cells, mode in ((True, LB.CELLS_H, flow), (False, LB.CELLS_H, "stripe"), (True, LB.CELLS_NONE, "stripe")):
        pl = _sw_plan("linear", cells, m, n, (ma, mi, g, g), single=single)
        assert pl.launch_info()["mode"] == mode
        assert pl.format_info()["values"] == "int32"
        _check_sw(pl, dev, A, B, (ma, mi, g, g), cells)


@gpu
@pytest.mark.parametrize("inputs", sorted(INPUTS))
@pytest.mark.parametrize("m,n", PROFILE_SHAPES)
@pytest.mark.parametrize("scoring,mode", [((127, -128, 3, 1), "stripe"), ((100, -128, 20, 7), "flow"),
                                          ((101, -128, 20, 7), "stripe")])
def test_profile_bytes_sw_affine(dev, scoring, mode, m, n, inputs):
    """SW affine's profile bytes: the stripe kernel's are the scores (127 and -128); the flow kernel's are score +
    open + extend, so (100, -128, 20, 7) is the last scoring it takes (127) and match 101 runs the stripe kernel.
    Score, end cell and the device traceback equal the oracle's."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    A, B = INPUTS[inputs](np.random.default_rng(m), m, n)
    pl = _sw_plan("affine", LB.CELLS_DIR, m, n, scoring)
    assert pl.launch_info()["mode"] == mode == ("flow" if affine_flow_ok(*scoring) else "stripe")
    _check_sw(pl, dev, A, B, scoring, LB.CELLS_DIR)


@gpu
@pytest.mark.parametrize("inputs", sorted(INPUTS))
@pytest.mark.parametrize("m,n", PROFILE_SHAPES)
def test_profile_bytes_gotoh_flow(dev, m, n, inputs):
    """The Gotoh flow kernel's profile bytes 4 (f + 2g) at g = 15 (124; g = 16 runs the stripe kernel): direction
    bytes, final state, score and walk equal the reference's."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    g, h = 15, 3
    A, B = INPUTS[inputs](np.random.default_rng(n), m, n)
    pl = Plan(LB.REF_GOTOH, LB.CELLS_DIR, [m], [n], [0], [0], match=1, mismatch=0, gap_open=g + h, gap_extend=g,
              start_type=-1)
    assert pl.launch_info()["mode"] == "flow" and pl.format_info()["values"] == "tagged4"
    _check_gotoh(pl, dev, A, B, g, h, tagged=True)


@gpu
@pytest.mark.parametrize("what,alg,shape,kw", [
    ("linear single, match + 2g = 128", "linear", [(65, 70)], dict(match=126, mismatch=0, gap_open=1, gap_extend=1)),
    ("linear couples, match + 2g = 128", "linear", [(65, 70)] * 4,
     dict(match=48, mismatch=0, gap_open=40, gap_extend=40)),
    ("linear, mismatch + 2g = -129", "linear", [(65, 70)], dict(match=1, mismatch=-131, gap_open=1, gap_extend=1)),
    ("linear, g < 0", "linear", [(65, 70)], dict(match=1, mismatch=0, gap_open=-1, gap_extend=-1)),
    ("affine, match = 128", "affine", [(65, 70)], dict(match=128, mismatch=0, gap_open=3, gap_extend=1)),
    ("affine, mismatch = -129", "affine", [(65, 70)], dict(match=1, mismatch=-129, gap_open=3, gap_extend=1)),
    ("affine, 127 min(m, n) >= 2^29", "affine", [(4300000, 4300000)],
     dict(match=127, mismatch=0, gap_open=3, gap_extend=1)),
    ("linear, 127 min(m, n) >= 2^29", "linear", [(4300000, 4300000)],
     dict(match=127, mismatch=0, gap_open=0, gap_extend=0)),
])
def test_out_of_range_scorings_are_rejected(dev, what, alg, shape, kw):
    """Scores no profile byte holds, and sizes whose scores leave the int32 working range, are
    MSA_ERR_UNSUPPORTED at plan creation (before anything is allocated or run).  A batch of couples with match +
    2g = 128 is rejected like a single pair: the int32 kernels read the same int8 profile."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    assert 127 * 4300000 >= (1 << 29)
    ms, ns = [m for m, _ in shape], [n for _, n in shape]
    with pytest.raises(LB.MsaError) as e:
        Plan({"linear": LB.SW_LINEAR, "affine": LB.SW_AFFINE}[alg], LB.CELLS_NONE, ms, ns,
             [k * ms[0] for k in range(len(ms))], [0] * len(ms), single=(len(ms) == 1), **kw)
    assert e.value.status == -5, what


# ---- d. the x4 tagged Gotoh values ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("inputs", ["all_mismatch", "identical"])
@pytest.mark.parametrize("shape", [0, 1])
def test_tagged_gotoh_at_the_bound(dev, shape, inputs):
    """gap_open 32,767 / gap_extend 15 at span m + n + 2 = 2,047 (4 x 32,768 x 2,047 < 2^28): the tagged format;
    direction bytes of every cell, final state, score and the device walk equal those of the reference's double
    tables.  Span 2,048 runs the untagged int32 kernel, equal as well."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    go, ge = REF1_GAPS
    m, n_at = ref1_shapes()[shape]
    for n, values in ((n_at, "tagged4"), (n_at + 1, "int32")):
        A, B = INPUTS[inputs](np.random.default_rng(n), m, n)
        pl = Plan(LB.REF_GOTOH, LB.CELLS_DIR, [m], [n], [0], [0], match=1, mismatch=0, gap_open=go, gap_extend=ge,
                  start_type=-1)
        assert pl.format_info()["values"] == values, (m, n)
        if values == "tagged4":
            assert pl.launch_info()["mode"] == "flow"
        _check_gotoh(pl, dev, A, B, ge, go - ge, tagged=(values == "tagged4"))


# ---- e. int16 chunk cells of the banded kernel ------------------------------------------------------------------
def _similar(rng, m, sub=0.02, indel=0.002):
    """A random A and B = A with substitutions and short indels (length ~m): every chunk converges."""
    A = rs(rng, m)
    b = bytearray(A)
    for k in rng.choice(m, size=int(m * sub), replace=False):
        b[k] = ACGT[rng.integers(4)]
    for k in sorted(rng.choice(m - 16, size=int(m * indel), replace=False), reverse=True):
        if rng.integers(2):
            del b[k:k + int(rng.integers(1, 8))]
        else:
            b[k:k] = rs(rng, int(rng.integers(1, 8)))
    return A, bytes(b)


@gpu
@pytest.mark.parametrize("g", [54, 55])
def test_banded_chunked_int16_bound_adjacent(oracle, dev, g):
    """rows + h + g band <= 30,000 at the default warm-up and chunk (2,112 rows, h = 1, band 512): g = 54 (29,761) is
    the last value whose chunks write int16 cells, g = 55 (30,273) the first that keeps int32 (test_gpu_parity's
    test_banded_chunked_int16_bound tries 50 and 60; same pair construction, same assertions, plus format_info).
    Score and every in-band cell equal the banded oracle's.  At gap costs this high the chunks of this pair do not
    converge (run_info: converged 0), so the cells compared come from the exact launch behind the chunks: what sits on
    the edge here is the admission and the int16 buffers' allocation, not an int16 value at -h - g band."""
    import os

    import torch
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    h, w = BAND_H16["h"], BAND_H16["band"]
    # (MSA_BAND_H16=0, the library's diagnostic switch, keeps int32 cells whatever the bound says)
    int16 = int(h16_ok(g, h, w)) if os.environ.get("MSA_BAND_H16") != "0" else 0
    A, B = _similar(np.random.default_rng(g), 12000)
    if abs(len(A) - len(B)) > w:
        B = B[:len(A) + w // 2]
    pl = Plan(LB.NW_BANDED, LB.CELLS_H, [len(A)], [len(B)], [0], [0], match=1, mismatch=0, gap_open=g + h,
              gap_extend=g, band=w)
    assert pl.format_info()["int16_cells"] == int16
    H = torch.empty(pl.cells_elems, dtype=torch.int32, device=dev)
    score, digest = oracle.banded_ref(A, B, w, float(g), float(h), want_digest=True)
    pl.run(_dev(A, dev), _dev(B, dev), H)
    assert pl.results()[0]["score"] == int(score)
    assert pl.checksum(H) == digest
    info = pl.run_info()
    assert info["mode"] == "chunked" and info["chunks"] >= 4, info
    assert info["int16_cells"] == int16, info
    assert pl.error() == 0
