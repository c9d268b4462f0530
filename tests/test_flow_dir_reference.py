"""The CPU yardsticks of test_gpu_flow_dir.py (tests/flow_dir_reference.py) against independent restatements, and
the inputs and shapes against the mechanisms they are named for -- all on the CPU, on the references alone.

* gotoh_tags and unswapped_tables against a per-cell Python triple loop; gotoh_walk against the oracle's node list,
  its ops rescored to max(T1, T2, T3)(m, n); sw_stream and gotoh_stream against the full-matrix references, every
  emitted row.
* periodic planes hold ties between the diagonal term and E or F; the gaps pairs' optimal walks cross rows 128 | 129
  and 512 | 513 with an 'I' run and column 128 with a 'D' run; both values of bits 2 and 3 occur on either side of
  every stripe link; mismatch planes are all floor.
* The flow kernels' stripe arithmetic, restated in Python, classifies every stripe of every GPU shape, and the shape
  list holds every boundary the GPU test is there for: a later edit of the lists cannot silently lose one."""
import numpy as np
import pytest

import flow_dir_reference as FR

SMALL_GH = FR.GOTOH_GH


def _tables_equal(T, L):
    return all(np.array_equal(np.asarray(t), np.asarray(l, dtype=np.float64)) for t, l in zip(T, L))


# ---- the Gotoh helpers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gh", SMALL_GH)
@pytest.mark.parametrize("m,n", [(1, 1), (1, 6), (3, 5), (9, 9), (12, 31)])
def test_gotoh_tags_against_triple_loop(oracle, gh, m, n):
    g, h = gh
    for kind in ("random", "periodic", "equal", "mismatch"):
        A, B = FR.pair_of(kind, m, n)
        T1, T2, T3, inv = oracle.subproblem_tables(A, B, -1, float(g), float(h))
        assert not inv
        L1, L2, L3, tags = FR.gotoh_triple_loop(A, B, g, h)
        assert _tables_equal((T1, T2, T3), (L1, L2, L3)), (kind, m, n)
        assert np.array_equal(FR.gotoh_tags(T1, T2, T3, float(g), float(h)), np.asarray(tags, dtype=np.uint8)), kind


@pytest.mark.parametrize("gh", SMALL_GH)
@pytest.mark.parametrize("m,n", [(2, 1), (6, 1), (9, 4), (31, 12)])
def test_unswapped_tables_against_triple_loop(oracle, gh, m, n):
    g, h = gh
    for kind in ("random", "periodic", "equal"):
        A, B = FR.pair_of(kind, m, n)
        T = FR.unswapped_tables(oracle, A, B, g, h)
        assert T[0].shape == (m + 1, n + 1)
        L1, L2, L3, tags = FR.gotoh_triple_loop(A, B, g, h)
        assert _tables_equal(T, (L1, L2, L3)), (kind, m, n)
        assert np.array_equal(FR.gotoh_tags(*T, float(g), float(h)), np.asarray(tags, dtype=np.uint8)), kind


WALK_SHAPES = [(1, 1), (1, 40), (5, 30), (64, 64), (150, 300), (540, 560)]


@pytest.mark.parametrize("gh", SMALL_GH)
@pytest.mark.parametrize("kind", FR.KINDS)
def test_gotoh_walk_against_oracle_nodes(oracle, gh, kind):
    """m <= n pairs (the oracle does not swap them): the walker's ops over gotoh_tags' plane are the tables of the
    oracle's node list, end node first (test_gotoh_device_walk's conversion), and rescore to the best of the three
    tables at (m, n)."""
    g, h = gh
    shapes = [s for s in WALK_SHAPES if FR.gap_room(kind, *s)]
    assert shapes
    for m, n in shapes[-3:]:
        A, B = FR.pair_of(kind, m, n)
        o = oracle.subproblem_align(A, B, -1, -1, float(g), float(h))
        assert not o["invert"]
        fin = tuple(float(T[m, n]) for T in (o["T1"], o["T2"], o["T3"]))
        ops, stop = FR.gotoh_walk(FR.gotoh_tags(o["T1"], o["T2"], o["T3"], float(g), float(h)), fin, m, n)
        ts = [t for (_, _, t) in o["nodes"]]
        want = "".join("MDI"[t - 1] for t in reversed(ts)) if ts else "MDI"[o["end"][2] - 1]
        assert ops.decode() == want, (kind, m, n)
        assert min(stop) == 0
        assert FR.gotoh_rescore(A, B, ops, g, h) == max(fin), (kind, m, n)


# ---- the row-streaming restatements ------------------------------------------------------------------------------
STREAM_SHAPES = [(1, 1), (1, 9), (9, 1), (5, 9), (40, 17), (130, 70), (70, 130)]


@pytest.mark.parametrize("scoring", FR.SW_SCORINGS)
@pytest.mark.parametrize("m,n", STREAM_SHAPES)
def test_sw_stream_against_full_matrix(scoring, m, n):
    for kind in ("random", "equal", "periodic", "mismatch"):
        A, B, ref = FR.sw_case(kind, m, n, scoring)
        wins = ((1, m), (max(1, m - 3), m), (1, min(m, 2)))
        st = FR.sw_stream(A, B, scoring, wins)
        assert (st["score"], st["end"]) == (ref["score"], ref["end"]), (kind, m, n)
        for lo, hi in wins:
            assert np.array_equal(st["rows"][(lo, hi)], ref["byte"][lo:hi + 1, 1:] & 15), (kind, m, n, lo, hi)


@pytest.mark.parametrize("gh", FR.GOTOH_GH)
@pytest.mark.parametrize("m,n", STREAM_SHAPES)
def test_gotoh_stream_against_full_matrix(oracle, gh, m, n):
    g, h = gh
    for kind in ("random", "equal", "periodic", "mismatch"):
        A, B = FR.pair_of(kind, m, n)
        T = FR.unswapped_tables(oracle, A, B, g, h)
        tags = FR.gotoh_tags(*T, float(g), float(h))
        wins = ((1, m), (max(1, m - 3), m))
        st = FR.gotoh_stream(A, B, g, h, wins)
        assert tuple(float(x) for x in st["fin"]) == tuple(float(t[m, n]) for t in T), (kind, m, n)
        for lo, hi in wins:
            assert np.array_equal(st["rows"][(lo, hi)], tags[lo - 1:hi]), (kind, m, n, lo, hi)


def test_stream_walk_window():
    """A walk over a window of bottom rows equals the walk over the whole plane where it stays inside, and says so
    where it does not."""
    m, n = 300, 40
    A, B = FR.tall_pair(m, n)
    g, h = 1, 2
    full = FR.gotoh_stream(A, B, g, h, ((1, m),))
    ops, stop = FR.gotoh_walk(full["rows"][(1, m)], full["fin"], m, n)
    assert stop[1] == 0 and stop[0] > m - 100
    win = FR.gotoh_stream(A, B, g, h, ((m - 99, m),))
    assert FR.gotoh_walk(win["rows"][(m - 99, m)], win["fin"], m, n, i0=m - 99) == (ops, stop)
    with pytest.raises(ValueError):
        FR.gotoh_walk(full["rows"][(1, m)][m - 10:], full["fin"], m, n, i0=m - 9)
    assert FR.gotoh_rescore(A, B, ops, g, h) == max(full["fin"])


# ---- the inputs reach the mechanisms they are named for ----------------------------------------------------------
def _ties(A, B, ref, scoring):
    """Interior cells (a) whose diagonal term equals E or F, (b) of them those where it is H too -- the tie decides
    bits 0-1 --, (c) whose E equals F."""
    ma, mi, _, _ = scoring
    S = FR.table4(ma, mi)
    dg = ref["H"][:-1, :-1] + S[FR.codes(A)][:, FR.codes(B)]
    H, E, F = ref["H"][1:, 1:], ref["E"][1:, 1:], ref["F"][1:, 1:]
    tie = (dg == E) | (dg == F)
    return int(tie.sum()), int((tie & (H == dg) & (H > 0)).sum()), int((E == F).sum())


@pytest.mark.parametrize("scoring", FR.SW_SCORINGS)
def test_periodic_planes_hold_ties(scoring):
    """ACGT... against CGTA...: the sequences match again after a shift by one or by the period, so values recur
    along and across the diagonals.  E ties F under every scoring.  The diagonal term ties E or F under every scoring
    but (100, -128, 20, 7), whose mismatch puts a mismatching cell's diagonal term more than a hundred below any gap
    value next to it and whose match puts a matching cell's above them; with zero gap costs the tie is for H
    itself."""
    m, n = FR.REUSE_SHAPE
    A, B, ref = FR.sw_case("periodic", m, n, scoring)
    tie, tie_h, ef = _ties(A, B, ref, scoring)
    assert ef > 0
    if scoring[1] > -128:
        assert tie > 0
    if scoring[2:] == (0, 0):
        assert tie_h > 0


@pytest.mark.parametrize("gh", FR.GOTOH_GH)
def test_periodic_tags_hold_ties(oracle, gh):
    """Gotoh: cells whose T1 candidates tie between T1 and a gap table."""
    g, h = gh
    m, n = FR.REUSE_SHAPE
    A, B = FR.pair_of("periodic", m, n)
    T1, T2, T3 = FR.unswapped_tables(oracle, A, B, g, h)
    d = T1[:-1, :-1]
    assert int(((d == T2[:-1, :-1]) | (d == T3[:-1, :-1])).sum()) > 0


def _crosses(runs, at):
    return any(lo <= at and hi >= at + 1 for lo, hi in runs)


GAP_SHAPES = [s for s in FR.SHAPES if any(k.startswith("gaps") for k in FR.kinds_for(*s))]


@pytest.mark.parametrize("m,n", GAP_SHAPES)
def test_gaps_walks_cross_the_boundaries(oracle, m, n):
    """Every gaps pair of every GPU shape: the optimal local walk (SW affine, GAP_SW_SCORING) and the optimal global
    walk (Gotoh, GAP_GH) hold an 'I' run consuming rows 128 and 129 (gaps_a128), rows 512 and 513 (gaps_a512), or a
    'D' run consuming columns 128 and 129 (gaps_b128)."""
    g, h = FR.GAP_GH
    for kind in FR.kinds_for(m, n):
        if not kind.startswith("gaps"):
            continue
        letter, at = (b"I", int(kind[6:])) if kind[5] == "a" else (b"D", 128)
        A, B, ref = FR.sw_case(kind, m, n, FR.GAP_SW_SCORING)
        assert _crosses(FR.ops_runs(ref["ops"], ref["end"], letter), at), (kind, "sw", ref["cigar"])
        T = FR.unswapped_tables(oracle, A, B, g, h)
        fin = tuple(float(t[m, n]) for t in T)
        ops, _ = FR.gotoh_walk(FR.gotoh_tags(*T, float(g), float(h)), fin, m, n)
        assert _crosses(FR.ops_runs(ops, (m, n), letter), at), (kind, "gotoh")


def test_gaps_kinds_all_occur():
    """A gap across rows 512 | 513 needs m >= 532 (the insert's last row is 516, and 16 equal symbols follow it): m =
    513 has no room, 640 and 2200 have.
    Each gaps kind occurs among the GPU cases of some shape, under both algorithms' case lists."""
    for scorings in (FR.SW_SCORINGS, FR.GOTOH_GH):
        seen = {kind for s in FR.SHAPES for _, kind in FR.cases(s, scorings)}
        assert seen == set(FR.KINDS)
    for s in FR.SHAPES:  # the four scorings together use every kind of the shape
        assert {kind for _, kind in FR.cases(s, FR.SW_SCORINGS)} == set(FR.kinds_for(*s)), s
    assert all(FR.gap_room("gaps_a128", m, n) for m, n in FR.SHAPES if m >= 257 and n >= 32)
    assert all(FR.gap_room("gaps_a512", m, n) for m, n in FR.SHAPES if m >= 640 and n >= 32)
    assert all(FR.gap_room("gaps_b128", m, n) for m, n in FR.SHAPES if m >= 257 and n >= 192)


@pytest.mark.parametrize("m,n", [s for s in FR.SHAPES if s[0] > 128 and s[1] >= 16])
def test_bits_2_and_3_on_both_sides_of_every_link(m, n):
    """Over the shape's SW cases, bit 2 and bit 3 are each set somewhere and clear somewhere in the last row of every
    stripe and in the first row of the next one: a link that drops or invents a gap opening changes a byte."""
    planes = [FR.sw_case(kind, m, n, sc)[2]["byte"] for sc, kind in FR.cases((m, n), FR.SW_SCORINGS)]
    for k in range(1, FR.n_stripes(m)):
        for i in (128 * k, 128 * k + 1):
            for bit in (4, 8):
                vals = {bool(v) for p in planes for v in (p[i, 1:] & bit)}
                assert vals == {False, True}, (k, i, bit)


@pytest.mark.parametrize("scoring", FR.SW_SCORINGS)
def test_mismatch_planes_are_all_floor(scoring):
    for m, n in FR.SHAPES:
        A, B, ref = FR.sw_case("mismatch", m, n, scoring)
        assert (ref["score"], ref["end"], ref["ops"]) == (0, (0, 0), b"")
        assert not (ref["H"] != 0).any() and not (ref["byte"] & 3).any()


# ---- the shapes reach the kernels' boundaries --------------------------------------------------------------------
def test_stripe_arithmetic():
    """fl_P / fl_bmax / fl_dq restated: the switch points derived in the kernel's terms."""
    c = FR.stripe_class
    assert [FR.fl_cs(k) for k in (0, 1, 2, 15, 16, 17)] == [0, -15, -14, -1, 0, -15]
    assert [FR.fl_dq(k) for k in (1, 2, 15, 16, 17, 18)] == [3, 4, 4, 4, 3, 4]
    # a full stripe 0 turns from the short to the head path at n = 32 -> 33
    assert (c(0, 128, 32)["path"], c(0, 128, 33)["path"]) == ("short", "head")
    assert (c(0, 128, 32)["P"], c(0, 128, 33)["P"]) == (6, 7)
    # stripes 1 and 17 (the link lags three phases) at n = 80 -> 81; stripe k = 2..16 (it lags four, and stripe k - 1
    # starts at column k - 17) at n = 79 + k -> 80 + k: at n = 81 stripes 1 and 17 alone are on the head path
    for k, n in [(1, 80), (17, 80), (2, 81), (3, 82), (16, 95)]:
        assert (c(k, 2200, n)["path"], c(k, 2200, n + 1)["path"]) == ("short", "head"), k
    assert [k for k in range(18) if c(k, 2200, 81)["path"] == "head"] == [0, 1, 17]
    # stripe 0: 8 -> 9 phases at n = 64 -> 65, 16 -> 17 at 192 -> 193; a second 8-phase segment from 9 phases on
    assert [c(0, 129, n)["P"] for n in (64, 65, 192, 193)] == [8, 9, 16, 17]
    assert [c(0, 129, n)["segs"] for n in (64, 65, 192, 193)] == [1, 2, 2, 3]
    # one row, the last lane's one row, its two rows, a second stripe of one row (it starts at column -15)
    assert [c(0, m, 33)["P"] for m in (1, 127, 128)] == [3, 7, 7]
    assert (FR.n_stripes(128), FR.n_stripes(129), c(1, 129, 33)["P"]) == (1, 2, 4)
    assert FR.fill_launch_min_m(256) == 65537 and FR.fill_launch_min_m(304) is not None
    # the tall pair: every full stripe has a second 32-phase segment
    assert {c(k, 65537, FR.TALL_N)["P"] for k in range(512)} == {33, 34}


def test_every_shape_is_classified():
    """Every stripe of every GPU shape is on the head or the short path with a positive phase count; the classes
    follow from n alone for full stripes below stripe 0."""
    for m, n in FR.SHAPES:
        assert m in FR.MS and n in FR.NS
        for k in range(FR.n_stripes(m)):
            cl = FR.stripe_class(k, m, n)
            assert cl["P"] >= 1 and cl["path"] in ("head", "short") and cl["segs"] == -(-cl["P"] // 8)
            if cl["path"] == "head":
                assert cl["P"] >= 7


def test_shape_list_holds_every_boundary():
    cl = {s: [FR.stripe_class(k, *s) for k in range(FR.n_stripes(s[0]))] for s in FR.SHAPES}
    paths = {s: [c["path"] for c in v] for s, v in cl.items()}
    # a stripe >= 1 on the short path below a head stripe 0
    assert any(p[0] == "head" and "short" in p[1:] for p in paths.values())
    # ... every later stripe of such a pair, at more than two stripes too
    assert any(p[0] == "head" and len(p) > 2 and set(p[1:]) == {"short"} for p in paths.values())
    # a stripe >= 1 on the head path
    assert any("head" in p[1:] for p in paths.values())
    # stripe 0 on the short path
    assert any(p[0] == "short" for p in paths.values())
    # stripe 0 with exactly 8, 9, 16 and 17 phases
    p0 = {v[0]["P"] for v in cl.values()}
    assert {8, 9, 16, 17} <= p0
    # stripes 16 and 17 (fl_cs wraps, the link's lag changes)
    assert any(len(v) >= 18 for v in cl.values())
    assert {v[k]["dq"] for v in cl.values() if len(v) >= 18 for k in (16, 17)} == {3, 4}
    # the pairs on either side of each boundary, m > n and m < n, the row boundaries
    for s in [(1, 97), (129, 64), (129, 65), (257, 192), (257, 193), (513, 17), (640, 300), (2200, 300)]:
        assert s in FR.SHAPES
    for n in (33, 81):
        assert {m for m, nn in FR.SHAPES if nn == n} == set(FR.MS)
    assert any(m > n for m, n in FR.SHAPES) and any(m < n for m, n in FR.SHAPES)
    assert any(m < n and n >= 192 for m, n in FR.SHAPES) and any(m > n and n <= 17 for m, n in FR.SHAPES)
    assert 2 * len(FR.MS) <= len(FR.SHAPES) <= 36 and len(set(FR.SHAPES)) == len(FR.SHAPES)
    assert FR.REUSE_SHAPE in FR.SHAPES
    # the one-plan-two-inputs shape has a second item (granules, io-in) and three 8-phase segments
    assert FR.n_stripes(FR.REUSE_SHAPE[0]) == 5 and cl[FR.REUSE_SHAPE][0]["segs"] == 3


def test_tall_pair_shape():
    A, B = FR.tall_pair(3000)
    assert (len(A), len(B)) == (3000, FR.TALL_N)
    st = FR.sw_stream(A, B, (1, 0, 3, 1))
    assert st["end"][0] >= 2990 and st["score"] > 300  # the local alignment ends in the last rows and spans B
