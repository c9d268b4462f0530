"""tests/walk_reference.py on the CPU: the yardsticks, builders, geometry model and case lists of
test_gpu_walk_planes.py.

* The reference walkers against the three walkers the suite already has, on the planes those modules make for their
  own inputs: sw_scored_reference.walk_bytes, nw_reference.walk_bytes (with and without a band) and
  flow_dir_reference.gotoh_walk (tags, and the same planes as table numbers).
* skew_dir against a cell-by-cell restatement of Plan.deskew_dir's index rule, one and two rows per lane, with a band,
  every pad value; layout_indices against it; the model's stripe geometry against plan.stripe_geom and
  flow_dir_reference's fl_cs / fl_P.
* plane_from_ops makes exactly its ops; random planes are valid and end on the border.
* Every case list reaches the boundary it is named for, asserted from the geometry model: a later edit of the lists
  cannot silently lose one.
"""
import functools

import numpy as np
import pytest

import flow_dir_reference as FR
import nw_reference as NW
import sw_scored_reference as SR
import walk_reference as W


# ---- the walkers against the existing ones -----------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(1, 1), (7, 9), (65, 70), (129, 64), (257, 193)])
def test_walk_sw_against_sw_scored_reference(m, n):
    for scoring in FR.SW_SCORINGS[:3]:
        for kind in ("random", "equal", "periodic", "gaps_a128", "gaps_b128"):
            if not FR.gap_room(kind, m, n):
                continue
            _, _, ref = FR.sw_case(kind, m, n, scoring)
            if ref["score"] == 0:
                continue
            w = W.walk_sw(ref["byte"], ref["end"], local=True)
            ops, beg = SR.walk_bytes(ref["byte"], ref["end"])
            assert (w.ops, (w.stop[0] + 1, w.stop[1] + 1), w.status) == (ops, beg, 0), (m, n, scoring, kind)
            assert w.cells[0] == tuple(ref["end"]) and len(set(w.cells)) == len(w.cells)


def _full(band_form, m, n, w):
    out = np.zeros((m + 1, n + 1), dtype=np.uint8)
    j, valid = NW.band_cols(m, n, w)
    ii = np.broadcast_to(np.arange(m + 1)[:, None], j.shape)
    out[ii[valid], j[valid]] = band_form[valid]
    return out


@pytest.mark.parametrize("band", [-1, 8, 40])
@pytest.mark.parametrize("m", [1, 9, 70, 300])
def test_walk_sw_against_nw_reference(m, band):
    rng = np.random.default_rng(1000 + m + 5 * band)
    A, B = NW.similar(rng, max(m, 20), sub=0.1, indel=0.05) if m >= 20 else (NW.rs(rng, m), NW.rs(rng, m))
    if band >= 0 and abs(len(A) - len(B)) > band:
        k = min(len(A), len(B)) + band
        A, B = A[:k], B[:k]
    for g, h in ((1, 2), (1, 0), (3, 5)):
        ref = NW.nw_reference(A, B, g, h, band)
        mm, nn = len(A), len(B)
        w = W.walk_sw(_full(ref["byte"], mm, nn, ref["w"]), (mm, nn), local=False)
        assert w.status == 0 and w.stop == ref["stop"]
        assert w.ops + b"I" * w.stop[0] + b"D" * w.stop[1] == ref["ops"]
        assert W.inside(W.Geom(mm, nn, 0, 1, 0), w.cells, band)


def _numbers(tags):
    """A tag plane as table numbers (every field 4 - tag)."""
    t = tags.astype(np.int64)
    f = [4 - ((t >> sh) & 3) for sh in (0, 2, 4)]
    return (f[0] | (f[1] << 2) | (f[2] << 4)).astype(np.uint8)


@pytest.mark.parametrize("m,n", [(1, 1), (5, 30), (64, 64), (150, 300), (300, 150)])
def test_walk_gotoh_against_flow_dir_reference(oracle, m, n):
    for g, h in FR.GOTOH_GH[:3]:
        for kind in ("random", "equal", "periodic"):
            A, B = FR.pair_of(kind, m, n)
            T = FR.unswapped_tables(oracle, A, B, g, h)
            tags = np.zeros((m + 1, n + 1), dtype=np.uint8)
            tags[1:, 1:] = FR.gotoh_tags(*T, float(g), float(h))
            fin = tuple(float(t[m, n]) for t in T)
            ops, stop = FR.gotoh_walk(tags[1:, 1:], fin, m, n)
            et = b"MDI".index(ops[:1]) + 1
            for tagged, plane in ((True, tags), (False, _numbers(tags))):
                w = W.walk_gotoh(plane, m, n, et, tagged)
                assert (w.ops, w.stop, w.status) == (ops, stop, 0), (m, n, g, h, kind, tagged)


def test_no_predecessor_codes():
    p = W.random_plane("nw", 30, 40, 0.6, 0)
    W.apply_path("nw", p, b"MMDMM", (30, 40), nomatch=True)
    w = W.walk_sw(p, (30, 40), local=False)
    assert (w.ops, w.stop, w.status) == (b"MMDMM", (26, 35), W.ERR_NOMATCH)
    assert W.walk_sw(p, (30, 40), local=True).status == 0
    for kind, tagged in (("tag", True), ("ref", False)):
        q = W.random_plane(kind, 30, 40, 0.6, 0)
        q[28, 38] &= 0xFC   # T1's field of the third cell of the diagonal
        q[30, 40] = (q[30, 40] & 0xFC) | (3 if tagged else 1)
        q[29, 39] = (q[29, 39] & 0xFC) | (3 if tagged else 1)
        w = W.walk_gotoh(q, 30, 40, 1, tagged)
        assert (w.ops, w.stop, w.status) == (b"MMM", (27, 37), W.ERR_NOMATCH)


# ---- the layout ----------------------------------------------------------------------------------------------------
LAYOUTS = [(1, 1, 1, -1), (7, 9, 1, -1), (65, 70, 1, -1), (130, 40, 1, -1), (1, 1, 2, -1), (127, 33, 2, -1),
           (129, 20, 2, -1), (300, 17, 2, -1), (150, 150, 1, 16), (200, 190, 1, 5)]


@pytest.mark.parametrize("m,n,R,band", LAYOUTS)
def test_skew_dir_is_the_inverse_of_the_deskew_rule(m, n, R, band):
    g, cs = W.model_geom(m, n, R, band, out_off=2048)
    rng = np.random.default_rng(m + n)
    M = rng.integers(0, 256, (m + 1, n + 1)).astype(np.uint8)
    M[0, :] = 0
    M[:, 0] = 0
    held = np.zeros_like(M, dtype=bool)   # the cells the layout holds: all of them, or a band's
    for i in range(1, m + 1):
        s, r, _ = W.locate(g, cs, i, 1)
        for j in range(1, n + 1):
            held[i, j] = 0 <= j - cs[s] + r // R < 16 * g.pmax
    assert held[1:, 1:].all() if band < 0 else held[W.inside_mask(m, n, band)].all()
    for pad in W.PADS:
        flat = W.skew_dir(g, cs, M, pad)
        assert flat.size == g.out_off + W.block_bytes(g) and (flat[:g.out_off] == pad).all()
        assert np.array_equal(W.deskew_rule(g, cs, flat), np.where(held, M, 0))
        # every byte that is no matrix cell is the pad
        cells = [(i, j) for i in range(1, m + 1) for j in range(1, n + 1) if held[i, j]]
        idx = W.layout_indices(g, cs, cells)
        assert len(set(idx.tolist())) == len(cells)
        assert [int(x) for x in idx[:50]] == [W.layout_index(g, cs, i, j) for i, j in cells[:50]]
        rest = np.ones(flat.size, dtype=bool)
        rest[idx] = False
        assert (flat[rest] == pad).all()
        # written in place into a larger tensor
        big = np.full(flat.size + 4096, 0x77, dtype=np.uint8)
        W.skew_dir(g, cs, M, pad, out=big)
        assert np.array_equal(big[g.out_off:flat.size], flat[g.out_off:]) and (big[flat.size:] == 0x77).all()
        assert (big[:g.out_off] == 0x77).all()


def test_model_geometry_against_the_existing_restatements():
    from cse305_parallel_sequence_alignment_amd import plan

    for m, n, band in [(1, 1, -1), (65, 300, -1), (600, 700, -1), (700, 900, -1), (700, 700, 16), (700, 700, 64)]:
        g, cs = W.model_geom(m, n, 1, band)
        geo = [plan.stripe_geom(k, m, n, band) for k in range((m + 63) // 64)]
        assert cs == [c for c, _ in geo] and g.pmax == max(p for _, p in geo)
    for m, n in W.flow_shapes() + W.SHAPES_B:
        g, cs = W.model_geom(m, n, 2)
        assert cs == [FR.fl_cs(k) for k in range(FR.n_stripes(m))]
        assert g.pmax == max([FR.fl_P(k, m, n) for k in range(FR.n_stripes(m))] +
                             [plan.stripe_geom(k, m, n, -1)[1] for k in range((m + 63) // 64)])
        for i, j in ((1, 1), (m, n), (m, 1), ((m + 1) // 2, n)):
            s, r, t = W.locate(g, cs, i, j)
            assert (s, t // 16, r >> 1) == FR.locate(i, j)
    assert [W.fl_cs(k) for k in (0, 1, 15, 16, 17)] == [0, -15, -1, 0, -15]


def test_group_b0_rule():
    for pmax in (3, 15, 16, 17, 40):
        for t in range(16 * pmax):
            b0 = W.group_b0(t, pmax)
            assert 0 <= b0 and (b0 + W.GROUP_BLOCKS <= pmax or b0 == 0)
            assert 16 * b0 <= t < 16 * b0 + W.GT   # it covers t
            if 0 < b0 < pmax - W.GROUP_BLOCKS:     # unclamped: it ends 16..31 steps right of t
                assert 16 <= 16 * b0 + W.GT - 1 - t <= 31
    assert W.group_b0(100, 40) == 0 and W.group_b0(639, 40) == 24 and W.group_b0(500, 40) == 17


# ---- the builders ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sw", "nw", "tag", "ref"])
def test_random_planes_are_valid(kind):
    for share in W.SHARES:
        p = W.random_plane(kind, 90, 120, share, 3)
        assert (p[0, :] == 0).all() and (p[:, 0] == 0).all()
        q = p[1:, 1:].astype(np.int64)
        if kind in ("sw", "nw"):
            assert ((q & 3) != 0).all()
            assert abs(((q & 3) == 1).mean() - share) < 0.03
            assert 0.4 < ((q & 4) != 0).mean() < 0.6 and 0.4 < ((q & 8) != 0).mean() < 0.6
        else:
            for sh in (0, 2, 4):
                assert (((q >> sh) & 3) != 0).all()
            assert abs((((q & 3) == (3 if kind == "tag" else 1))).mean() - share) < 0.03
        assert (q >> (4 if kind in ("sw", "nw") else 6)).max() > 0   # the unread bits are not all 0
        for st in (1, 2, 3):
            w = W.walk_plane(kind, p, (90, 120), st)
            assert w.status == 0 and min(w.stop) == 0 and W.inside(W.Geom(90, 120, 0, 1, 0), w.cells)
    assert not np.array_equal(W.random_plane(kind, 9, 9, 0.6, 0), W.random_plane(kind, 9, 9, 0.6, 1))


@functools.lru_cache(maxsize=4)
def _base(kind, m, n):
    p = W.random_plane(kind, m, n, 0.5, "base")
    return p, p.copy()


def _walk_case(kind, m, n, c):
    """The reference walk of a constructed path over the kind's background plane (restored afterwards)."""
    ops, reopen = W.expand(c["segs"])
    local = c["local_stop"]
    base, work = _base(kind, m, n)
    cells = W.apply_path(kind, work, ops, (m, n), reopen, local_stop=local)
    w = W.walk_plane(kind, work, (m, n), b"MDI".index(ops[:1]) + 1 if ops else 1)
    if cells:
        ij = np.asarray(cells)
        work[ij[:, 0], ij[:, 1]] = base[ij[:, 0], ij[:, 1]]
    assert w.ops == ops and w.status == 0, (kind, m, n)
    assert (min(w.stop) > 0) == local
    return w, reopen


def test_plane_from_ops_makes_its_path_alone():
    m, n = 200, 260
    segs = W.to_border([("M", 3), ("D", 2), ("D", 4), ("I", 1), ("I", 3), ("M", 9), ("D", 1), ("I", 1)], (m, n))
    ops, reopen = W.expand(segs)
    assert ops[:14] == b"MMMDDDDDDIIIIM" and reopen == {4, 9}
    for kind in ("sw", "nw", "tag", "ref"):
        p = W.plane_from_ops(kind, m, n, ops, (m, n), reopen, seed=1)
        w = W.walk_plane(kind, p, (m, n), 1)
        assert w.ops == ops and min(w.stop) == 0
        if kind in ("sw", "nw"):
            # the reopened gaps close: H is held between them
            k = w.cells.index((m - 3, n - 5))
            assert w.states[k] == {0, 1}
        # one flipped path byte sends the walk elsewhere: the neighbours are random, not a copy of the path
        q = p.copy()
        q[m - 1, n - 1] ^= 2 if kind in ("sw", "nw") else 1
        assert W.walk_plane(kind, q, (m, n), 1).ops != ops


# ---- the case lists reach their boundaries -----------------------------------------------------------------------
def test_shapes_a_sit_on_their_boundaries():
    geo = {s: W.model_geom(*s)[0] for s in W.SHAPES_A}
    assert geo[(130, 150)].pmax < W.GROUP_BLOCKS <= geo[(200, 260)].pmax and geo[(65, 300)].pmax >= W.GROUP_BLOCKS
    assert W.n_stripes(geo[(130, 150)]) == 3 and geo[(130, 190)].pmax == W.GROUP_BLOCKS + 1
    assert all(geo[s].pmax < W.GROUP_BLOCKS for s in [(1, 1), (7, 9), (63, 70), (64, 64)])
    assert W.n_stripes(geo[(63, 70)]) == 1 == W.n_stripes(geo[(64, 64)]) and W.n_stripes(geo[(65, 300)]) == 2
    assert W.n_stripes(geo[(600, 700)]) > 2 * 4   # every one of the four slots is used more than once
    assert len(W.BATCH_SHAPES) >= 9 and len(set(W.BATCH_SHAPES)) == len(W.BATCH_SHAPES)
    assert len(W.BATCH_SHAPES) % W.TBB_WPB != 0
    # (200, 260): over the seeds, groups clamped at 0, at pmax - 16, and unclamped ones
    g, cs = W.model_geom(200, 260)
    seen = set()
    for kind in ("nw", "tag"):
        for share in W.SHARES:
            for seed in range(W.SEEDS):
                w = W.walk_plane(kind, W.random_plane(kind, 200, 260, share, seed), (200, 260), 1 + seed % 3)
                assert w.status == 0 and W.steps_in_range(g, cs, w.cells)
                tr = []
                W.batch_groups(g, cs, w.cells, tr)
                for k, s, b0, left in tr:
                    t = W.locate(g, cs, *w.cells[k])[2]
                    raw = ((t + 16) >> 4) - 15
                    seen.add("low" if raw < 0 else "high" if raw > g.pmax - 16 else "free")
                    if left:
                        seen.add("left")
    assert seen >= {"low", "high", "free"}, seen
    # every share gives every transition of the SW byte and of the Gotoh fields, over the (600, 700) walks
    for kind in ("nw", "tag"):
        pairs = set()
        for share in W.SHARES:
            for seed in range(W.SEEDS):
                w = W.walk_plane(kind, W.random_plane(kind, 600, 700, share, seed), (600, 700), 1 + seed % 3)
                pairs |= set(zip(w.ops, w.ops[1:]))
        assert len(pairs) == 9, (kind, pairs)


def test_flow_shapes_sit_on_their_boundaries():
    shapes = W.flow_shapes()
    assert {m for m, _ in shapes} == set(W.FLOW_MS) and len(shapes) >= 15
    assert [FR.n_stripes(m) for m in W.FLOW_MS] == [1, 1, 2, 5, 18]
    assert FR.n_stripes(2200) > 16 and W.fl_cs(16) == 0 == W.fl_cs(0) and W.fl_cs(17) == W.fl_cs(1)
    pm = {W.model_geom(m, n, 2)[0].pmax >= W.GROUP_BLOCKS for m, n in shapes}
    assert pm == {True, False}   # both staging paths
    for m, n in shapes:
        g, cs = W.model_geom(m, n, 2)
        for seed in range(3):
            w = W.walk_plane("tag", W.random_plane("tag", m, n, 0.6, seed), (m, n), 1 + seed)
            assert W.steps_in_range(g, cs, w.cells) and W.inside(g, w.cells)


def _first_steps(g, cs, w):
    """{(boundary, state)}: the walk stands on a stripe's top row / on its group's first step in that state."""
    tr = []
    W.batch_groups(g, cs, w.cells, tr)
    first = {k: b0 for k, _, b0, _ in tr}
    seen, b0 = set(), None
    for k, (i, j) in enumerate(w.cells):
        b0 = first.get(k, b0)
        _, r, t = W.locate(g, cs, i, j)
        for st in w.states[k]:
            if r == 0:
                seen.add(("top", st))
            if t == 16 * b0:
                seen.add(("first", st))
    return seen


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("m,n", W.SHAPES_B)
def test_constructed_paths_reach_their_boundaries(m, n, R):
    g, cs = W.model_geom(m, n, R)
    cases = W.path_cases(m, n, R, local=True)
    walks = {}
    for name, c in cases.items():
        walks[name], _ = _walk_case("sw", m, n, c)
        w = walks[name]
        assert W.steps_in_range(g, cs, w.cells) and W.inside(g, w.cells), name
        if not name.startswith("local"):   # the Gotoh kinds walk the same ops
            for kind in ("tag", "ref"):
                assert _walk_case(kind, m, n, c)[0].cells == w.cells, (name, kind)
    left = {name: W.left_exits(g, cs, w.cells) for name, w in walks.items()}
    # the horizontal gaps: 239 ends on the first step of the group staged at the stripe entry (the diagonal after it
    # leaves the group, in state H), 240 and more leave it inside the gap (in state E)
    assert left["local_after_hgap239"] == 0 == left["local_after_hgap238"] and left["local_after_hgap240"] == 1
    for L in W.HGAPS:
        w, tr = walks[f"hgap{L}"], []
        W.batch_groups(g, cs, w.cells, tr)
        entry = [k for k, _, _, lf in tr if not lf][1]      # the stripe above the end cell's
        exits = [k for k, _, _, lf in tr if lf and k <= entry + L]   # the group is left inside the gap's row
        assert W.locate(g, cs, *w.cells[entry])[2] % 16 == 15
        assert exits == {239: [], 700: [entry + 240, entry + 480]}.get(L, [entry + 240]), (L, entry, exits)
        assert all(w.cells[k][0] == w.cells[entry][0] for k in exits)
    # a gap that ends exactly on a group's first step: the local start there is read at tg == 0
    w = walks["local_after_hgap239"]
    tr = []
    W.batch_groups(g, cs, w.cells, tr)
    assert W.locate(g, cs, *w.stop)[2] == 16 * tr[-1][2]
    # the vertical gaps cross 0..4 (two rows per lane: 0..2) stripe links, each entered right of its prediction
    SR = 64 * R
    cross = [(m - 11) // SR - (m - 11 - L) // SR for L in W.VGAPS]
    assert min(cross) <= 1 and max(cross) >= (4 if R == 1 else 2), cross
    lb = {L: W.demand_lower_bound(g, cs, walks[f"vgap{L}"].cells) for L in W.VGAPS}
    assert lb[300] >= 3 and lb[300] > lb[20], lb
    # gaps that reopen on the next cell, E -> H -> F and F -> H -> E corners
    ops, reopen = W.expand(cases["reopen"]["segs"])
    assert len(reopen) >= 4 and b"DI" in ops and b"ID" in ops
    for k in W.STAIRS:
        assert walks[f"stair{k}"].ops[3:3 + 2 * k] == b"DI" * k
    # the four edges
    for name, row, colm in (("col_n_row_1", 1, n), ("row_m_col_1", m, 1)):
        cells = walks[name].cells
        assert sum(1 for i, _ in cells if i == row) >= n - 1 and sum(1 for _, j in cells if j == colm) >= m - 1
    # the border in each of the three states
    last = {name: max(walks[name].states[-1]) for name in ("border_E", "border_F", "vgap20")}
    assert last == {"border_E": 1, "border_F": 2, "vgap20": 0}
    assert walks["border_E"].stop[1] == 0 < walks["border_E"].stop[0]
    assert walks["border_F"].stop[0] == 0 < walks["border_F"].stop[1]
    # a stripe's top row and a group's first step, stood on in every state; the path ends on a stripe's top row (row
    # 1) in states H and F
    seen = set()
    for w in walks.values():
        seen |= _first_steps(g, cs, w)
    assert seen >= {(b, st) for b in ("top", "first") for st in (0, 1, 2)}, seen
    assert _first_steps(g, cs, walks["group_first_step_F"]) >= {("first", 2)}
    # local starts: after 0..7 single gaps, on a top row, right at a stripe entry, on row 1 and column 1
    assert [len(walks[f"local_pos{k}"].ops) for k in range(8)] == list(range(8))
    assert W.locate(g, cs, *walks["local_top_row"].stop)[1] == 0 or R == 2
    assert W.stripes_entered(g, walks["local_stripe_entry"].cells) == 2
    assert walks["local_stripe_entry"].stop == walks["local_stripe_entry"].cells[-1]
    assert walks["local_row_1"].stop[0] == 1 and walks["local_col_1"].stop[1] == 1
    # the diagonal runs: every length (the long ones on the large shape), starting at every residue mod 16
    for L in W.RUNS:
        if f"runs{L}" in walks:
            starts = W.run_starts(walks[f"runs{L}"].ops, L)
            assert {k % 16 for k in starts} == set(range(16)), (L, starts)
    assert {L for L in W.RUNS if f"runs{L}" in walks} >= ({1, 15, 16, 17} if m < 2000 else set(W.RUNS))


@pytest.mark.parametrize("band", W.BANDS)
def test_banded_paths_hug_the_band(band):
    m = W.BAND_M
    g, cs = W.model_geom(m, m, 1, band)
    diffs = {}
    for name, segs in W.band_cases(band).items():
        w, _ = _walk_case("nw", m, m, dict(segs=segs, local_stop=False))
        assert W.inside(g, w.cells, band) and W.steps_in_range(g, cs, w.cells), name
        diffs[name] = [i - j for i, j in w.cells]
    assert diffs["edge_plus"].count(band) >= m - 2 * band - 2 and max(diffs["edge_plus"]) == band
    assert diffs["edge_minus"].count(-band) >= m - 2 * band - 2 and min(diffs["edge_minus"]) == -band
    assert min(diffs["switch"]) == -band and max(diffs["switch"]) == band
    assert diffs["switch"].count(band) >= 100 and diffs["switch"].count(-band) >= 100


def test_tall_paths():
    m, n = W.RING_SHAPE
    ops = W.tall_ops(m, n)
    assert n <= 320 and len(ops) >= W.RING_MIN_OPS and b"MM" not in ops
    assert W.consumed(ops)[0] == m and W.consumed(ops)[1] < n
    assert ops.count(b"M") > 100 and ops.count(b"D") > 100
    # a ring word holds one window of at most 7 steps or one diagonal run -- here of length 1 --: at most 7 ops
    assert -(-len(ops) // 7) >= 2 * W.TB_RAW + W.TB_RAW // 2
    assert len(ops) > W.CAP
    m, n = W.STARTS_SHAPE
    g, cs = W.model_geom(m, n)
    assert m == 64 * 8192 + 65 and n == 96 and W.n_stripes(g) == W.TB_CSL + 2
    assert b"MM" not in W.tall_ops(m, n) and W.consumed(W.tall_ops(m, n))[0] == m


def test_tall_plane_walks_as_built():
    m, n = W.RING_SHAPE
    ops = W.tall_ops(m, n)
    for kind, R in (("nw", 1), ("tag", 2)):
        p = W.random_plane(kind, m, n, 0.5, "tall")
        W.apply_path(kind, p, ops, (m, n))
        w = W.walk_plane(kind, p, (m, n), 3)
        g, cs = W.model_geom(m, n, R)
        assert w.ops == ops and w.stop[0] == 0 and W.steps_in_range(g, cs, w.cells)
        assert W.stripes_entered(g, w.cells) == W.n_stripes(g)


def test_noisy_pair_has_many_gaps(oracle):
    A, B = W.noisy_pair()
    assert len(A) <= len(B) and abs(len(A) - W.NOISY["m"]) < 200 and abs(len(B) - W.NOISY["m"]) < 200
    o = oracle.sw(A, B, *W.NOISY["sw"], want_tb=True)
    cigar = o["cigar"]
    runs = sum(1 for ch in cigar if ch in "DI")
    assert runs >= W.NOISY["min_gap_runs"], runs
    g, h = W.NOISY["gh"]
    o = oracle.subproblem_align(A, B, -1, -1, float(g), float(h))
    ops = "".join("MDI"[t - 1] for (_, _, t) in reversed(o["nodes"])).encode()
    assert W.gap_runs(ops) >= W.NOISY["min_gap_runs"]
