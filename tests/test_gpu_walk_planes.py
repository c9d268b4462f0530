"""The two device traceback walkers (traceback_kernel in msa_traceback.hip, traceback_batch_kernel in msa_tbatch.hip)
on direction planes built on the CPU, isolated from the fills.

A plan runs once on a real pair, which gives it its stripe meta and, for the kinds that start there, its end cell.
Then its direction tensor is overwritten with a plane from tests/walk_reference.py (skew_dir, asserted against
Plan.deskew_dir itself) and walked: every op byte, the count, the stop cell, the status and the stripes entered equal
the plain-Python reference walker's; the batch walker's staged groups equal the geometry model's, the single walker's
on-demand groups are at least the model's lower bound; no byte of the 0xAA-prefilled ops buffer outside the ops
changes; the plan's error word stays 0.  test_walk_reference.py checks the references, the builders, the model and the
case lists on the CPU, and asserts that every case reaches the boundary it is named for.

Plan kinds (launch mode and rows per lane asserted for each): NW_ALIGN unbanded and banded (constructed paths only),
NW_FIT, NW_OVERLAP, SW_AFFINE with track_end in the stripe layout and in the flow layout (two rows per lane),
REF_GOTOH tagged (start type -1) in both layouts, and REF_GOTOH untagged (MSA_ALG_REF: start type -2 selects it).
The batch walker runs wherever it takes the plan (one row per lane, SW bytes).

Safety: before any walk of a plane the reference walk has terminated, and every cell it stands on is inside the matrix
(and the band), with a step 0 <= t < 16 pmax under the run's own stripe meta.  No plane holds arbitrary bytes.  The
file runs smallest cases first; run it with -x.  A failing case prints its kind, shape, seed and name.

a. random planes (20 seeds x 3 diagonal shares per shape); b. constructed paths; c. ring laps and a short ops buffer;
d. more than 8,192 stripes; e. a real noisy 6,000 x 6,000 pair against the oracle.
"""
import numpy as np
import pytest

import walk_reference as W

pytestmark = pytest.mark.gpu

UNTAGGED_START = -2   # any start type but -1 takes MSA_ALG_REF: table numbers in the bytes

# kind -> (walk kind of walk_reference, Plan arguments, rows per lane, the batch walker takes it)
KINDS = {
    "nw": ("nw", dict(alg="NW_ALIGN", gap_open=3, gap_extend=1, match=1, mismatch=0), 1, True),
    "fit": ("nw", dict(alg="NW_FIT", gap_open=3, gap_extend=1, match=1, mismatch=0), 1, True),
    "overlap": ("nw", dict(alg="NW_OVERLAP", gap_open=3, gap_extend=1, match=1, mismatch=0), 1, True),
    "sw": ("sw", dict(alg="SW_AFFINE", gap_open=5, gap_extend=2, match=2, mismatch=-3, track_end=True), 1, True),
    "sw_flow": ("sw", dict(alg="SW_AFFINE", gap_open=5, gap_extend=2, match=2, mismatch=-3, track_end=True), 2, False),
    "tag": ("tag", dict(alg="REF_GOTOH", gap_open=3, gap_extend=1, match=1, mismatch=0, start_type=-1), 1, False),
    "tag_flow": ("tag", dict(alg="REF_GOTOH", gap_open=3, gap_extend=1, match=1, mismatch=0, start_type=-1), 2, False),
    "ref": ("ref", dict(alg="REF_GOTOH", gap_open=3, gap_extend=1, match=1, mismatch=0, start_type=UNTAGGED_START), 1,
            False),
}
STRIPE_KINDS = [k for k, v in KINDS.items() if v[2] == 1]
FLOW_KINDS = [k for k, v in KINDS.items() if v[2] == 2]


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _suffix_pair(m, n, seed):
    """The shorter sequence is the longer one's suffix: every free-end kind ends at (m, n) with a positive score."""
    L = W._rng("pair", m, n, seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), max(m, n)).tobytes()
    return L[len(L) - m:], L[len(L) - n:]


def _codes(x):
    return np.frombuffer(x.translate(bytes.maketrans(b"ACGT", b"\x00\x01\x02\x03")), dtype=np.uint8).copy()


class Ctx:
    """One plan, run once on suffix pairs: its geometry, stripe starts and end cells, and a host copy of the layout."""

    def __init__(self, LB, dev, kind, shapes, band=-1, single=None):
        import torch
        from cse305_parallel_sequence_alignment_amd.plan import Plan

        self.kind, self.dev, self.band, self.LB = kind, dev, band, LB
        self.wkind, args, self.R, self.batch_ok = KINDS[kind]
        args = dict(args)
        alg = getattr(LB, args.pop("alg"))
        ms, ns = [m for m, _ in shapes], [n for _, n in shapes]
        pairs = [_suffix_pair(m, n, k) for k, (m, n) in enumerate(shapes)]
        ao = np.concatenate(([0], np.cumsum(ms)))[:-1]
        bo = np.concatenate(([0], np.cumsum(ns)))[:-1]
        if single is None:
            single = self.R == 2 or (len(shapes) == 1 and alg != LB.SW_AFFINE and alg != LB.REF_GOTOH)
        self.pl = pl = Plan(alg, LB.CELLS_DIR, ms, ns, ao, bo, band=band, single=single, **args)
        info = pl.launch_info()
        # a one-pair batch of 16 stripes or more (SW_AFFINE and REF_GOTOH here, whose single-pair plans are flow plans)
        # is split into items: the same kernel family and layout as "stripe"
        split = not single and len(shapes) == 1 and (ms[0] + 63) // 64 >= 16
        want_mode = "flow" if self.R == 2 else "band" if band >= 0 else "split" if split else "stripe"
        assert info["mode"] == want_mode and info["rows_per_lane"] == self.R, (kind, shapes, info)
        print("plan", kind, shapes[:2], "band", band, "mode", info["mode"], "rows per lane", info["rows_per_lane"])
        if kind.startswith("tag"):
            assert pl.format_info()["values"] == "tagged4"
        if kind == "ref":
            assert pl.format_info()["values"] == "int32"
        self.D = torch.empty(pl.cells_elems, dtype=torch.uint8, device=dev)
        dA = torch.from_numpy(np.concatenate([_codes(a) for a, _ in pairs])).to(dev)
        dB = torch.from_numpy(np.concatenate([_codes(b) for _, b in pairs])).to(dev)
        pl.run(dA, dB, self.D)
        self.meta = pl.stripe_meta()
        res = pl.results()
        assert pl.error() == 0
        self.geom, self.cs, self.ends = [], [], []
        for k, (m, n) in enumerate(shapes):
            pg = pl.geom[k]
            g = W.Geom(m, n, pg.pmax, pg.rows_per_lane, pg.out_off)
            cs = [int(x) for x in self.meta[pg.stripe0:pg.stripe0 + W.n_stripes(g), 0]]
            mg, mcs = W.model_geom(m, n, self.R, band)
            # the CPU suite's boundary assertions are made on the model's geometry: the plan's own must equal it
            assert (g.pmax if len(shapes) == 1 else None, cs) == (mg.pmax if len(shapes) == 1 else None, mcs), \
                (kind, m, n, g, mg)
            self.geom.append(g)
            self.cs.append(cs)
            if self.wkind in ("tag", "ref") or kind == "nw":
                self.ends.append((m, n))
            else:
                assert res[k]["score"] > 0 or kind != "sw"
                self.ends.append(tuple(res[k]["end"]))
        self.flat = np.zeros(pl.cells_elems, dtype=np.uint8)

    # -- planes into the layout ------------------------------------------------------------------------------------
    def load(self, planes, pad):
        """Skew every pair's plane into the host layout (every other byte = pad), assert the round trip through
        Plan.deskew_dir, and upload."""
        self.flat[:] = pad
        for k, p in enumerate(planes):
            W.skew_dir(self.geom[k], self.cs[k], p, pad, out=self.flat)
            back = self.pl.deskew_dir(self.flat, k, self.meta)
            ok = np.ones(p.shape, dtype=bool) if self.band < 0 else self._in_band(k)   # (a band: its cells)
            assert np.array_equal(back[ok], p[ok]), (self.kind, self.geom[k], "skew_dir is not deskew_dir's inverse")
        self.upload()

    def _in_band(self, k):
        g = self.geom[k]
        i, j = np.arange(g.m + 1)[:, None], np.arange(g.n + 1)[None, :]
        return (np.abs(i - j) <= self.band) & (i >= 1) & (j >= 1)

    def upload(self):
        import torch

        self.D.copy_(torch.from_numpy(self.flat).to(self.dev))

    def poke(self, k, plane, cells):
        """Copy the plane's bytes at `cells` into the host layout (the rest is as loaded)."""
        if cells:
            ij = np.asarray(cells)
            self.flat[W.layout_indices(self.geom[k], self.cs[k], cells)] = plane[ij[:, 0], ij[:, 1]]

    # -- the CPU side of a walk: the reference, and the conditions of a safe GPU walk --------------------------------
    def reference(self, k, plane, start_table, what):
        g, cs = self.geom[k], self.cs[k]
        w = W.walk_plane(self.wkind, plane, self.ends[k], start_table)   # (returned: it terminated)
        assert W.inside(g, w.cells, self.band), what
        assert W.steps_in_range(g, cs, w.cells), what
        assert min(w.stop) >= 0 and (w.status != 0 or min(w.stop) == 0 or self.wkind == "sw"), what
        return w

    # -- the walks -----------------------------------------------------------------------------------------------
    def single(self, k, w, start_table, what, cap=None):
        """The single walker over pair k against the reference walk w."""
        import torch

        g = self.geom[k]
        room = g.m + g.n + 2 + 64
        ops = torch.full((room,), 0xAA, dtype=torch.uint8, device=self.dev)
        info = torch.zeros(8, dtype=torch.int64, device=self.dev)
        view = ops[:room - 64 if cap is None else cap]
        if self.wkind == "sw":
            self.pl.traceback_async(self.D, view, info, pair=k)
        elif self.wkind == "nw":
            self.pl.traceback_nw_async(self.D, view, info, pair=k)
        else:
            self.pl.traceback_gotoh_async(self.D, view, info, end_type=start_table, pair=k)
        inf = [int(x) for x in info.cpu().tolist()]
        got = ops.cpu().numpy()
        self._check(what, "single", w, inf, got, view.numel(), g, self.cs[k])
        lb = W.demand_lower_bound(g, self.cs[k], w.cells)
        assert inf[5] >= lb, (what, "on-demand groups", inf[5], "model's lower bound", lb)

    def batch(self, ws, what):
        """The batch walker over every pair of the plan against the reference walks ws."""
        import torch

        off = self.pl.ops_layout(self.pl.ms, self.pl.ns)
        ops = torch.full((off[-1] + 64,), 0xAA, dtype=torch.uint8, device=self.dev)
        info = torch.zeros(8 * len(ws), dtype=torch.int64, device=self.dev)
        self.pl.traceback_batch_async(self.D, ops, torch.tensor(off, dtype=torch.int64, device=self.dev), info)
        inf = info.cpu().numpy().reshape(-1, 8)
        got = ops.cpu().numpy()
        assert (got[off[-1]:] == 0xAA).all(), what
        for k, w in enumerate(ws):
            x = [int(v) for v in inf[k]]
            self._check((what, "pair", k), "batch", w, x, got[off[k]:off[k + 1]], off[k + 1] - off[k], self.geom[k],
                        self.cs[k])
            staged = W.batch_groups(self.geom[k], self.cs[k], w.cells)
            assert x[5] == staged, (what, "pair", k, "groups staged", x[5], "model", staged)

    def _check(self, what, who, w, inf, got, cap, g, cs):
        status = w.status if (w.status != 0 or len(w.ops) <= cap) else W.ERR_CAPACITY
        want = dict(n_ops=len(w.ops), stop=(w.stop[0] + 1, w.stop[1] + 1), status=status,
                    stripes=W.stripes_entered(g, w.cells))
        have = dict(n_ops=inf[0], stop=(inf[1], inf[2]), status=inf[3], stripes=inf[4])
        print(who, what, have, "groups", inf[5])
        assert have == want, (who, what, have, want)
        k = min(len(w.ops), cap)
        ref = np.frombuffer(w.ops, dtype=np.uint8)[:k]
        bad = np.flatnonzero(got[:k] != ref)
        assert bad.size == 0, (who, what, "first differing op", int(bad[0]), bytes(got[bad[0]:bad[0] + 8]),
                               w.ops[bad[0]:bad[0] + 8])
        assert (got[k:] == 0xAA).all(), (who, what, "a byte past the ops changed", int(np.flatnonzero(got[k:] != 0xAA)[0]) + k)
        assert self.pl.error() == 0, (who, what)


def _start_table(wkind, seed):
    return 1 + seed % 3 if wkind in ("tag", "ref") else 1


# ---- a. random planes, one row per lane: one plan of ten pairs, both walkers -------------------------------------
@pytest.mark.parametrize("share", W.SHARES)
@pytest.mark.parametrize("kind", STRIPE_KINDS)
def test_random_planes_stripe_layout(dev, LB, kind, share):
    """Every pair of W.BATCH_SHAPES in one plan; per seed a random plane per pair, one batch launch (where the batch
    walker takes the plan) and one single walk per pair."""
    cx = Ctx(LB, dev, kind, W.BATCH_SHAPES)
    assert len(W.BATCH_SHAPES) >= 9 and len(W.BATCH_SHAPES) % W.TBB_WPB != 0
    for seed in range(W.SEEDS):
        pad = W.PADS[seed % 3]
        planes = [W.random_plane(cx.wkind, m, n, share, seed) for m, n in W.BATCH_SHAPES]
        st = _start_table(cx.wkind, seed)
        what = (kind, "share", share, "seed", seed, "pad", pad)
        ws = [cx.reference(k, p, st, what + (W.BATCH_SHAPES[k],)) for k, p in enumerate(planes)]
        cx.load(planes, pad)
        if cx.batch_ok:
            cx.batch(ws, what)
        for k, w in enumerate(ws):
            cx.single(k, w, st, what + (W.BATCH_SHAPES[k],))


# ---- a. random planes, two rows per lane: the single walker ------------------------------------------------------
@pytest.mark.parametrize("shape", W.flow_shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", FLOW_KINDS)
def test_random_planes_flow_layout(dev, LB, kind, shape):
    cx = Ctx(LB, dev, kind, [shape])
    assert cx.cs[0] == [W.fl_cs(k) for k in range(len(cx.cs[0]))]
    for share in W.SHARES:
        for seed in range(W.SEEDS):
            pad = W.PADS[seed % 3]
            p = W.random_plane(cx.wkind, shape[0], shape[1], share, seed)
            st = _start_table(cx.wkind, seed)
            what = (kind, shape, "share", share, "seed", seed, "pad", pad)
            w = cx.reference(0, p, st, what)
            cx.load([p], pad)
            cx.single(0, w, st, what)


# ---- b. constructed paths ----------------------------------------------------------------------------------------
def _paths(cx, cases, what0, both=True):
    """Walk every constructed path of `cases` ({name: dict(segs, local_stop[, nomatch])}) over one random background
    plane: the path's cells are poked into the loaded layout and restored after the walk."""
    g = cx.geom[0]
    end = cx.ends[0]
    assert end == (g.m, g.n), (what0, end)
    base = W.random_plane(cx.wkind, g.m, g.n, 0.5, ("base",) + tuple(what0))
    work = base.copy()
    loaded = None
    for n_case, (name, c) in enumerate(cases.items()):
        pad = W.PADS[n_case % 3]
        if loaded != pad:
            cx.load([base], pad)   # (asserts the round trip through Plan.deskew_dir)
            loaded = pad
        ops, reopen = W.expand(c["segs"])
        cells = W.apply_path(cx.wkind, work, ops, end, reopen, c.get("local_stop", False), c.get("nomatch", False))
        st = b"MDI".index(ops[:1]) + 1 if (ops and cx.wkind in ("tag", "ref")) else 1
        what = tuple(what0) + (name, "pad", pad)
        w = cx.reference(0, work, st, what)
        assert w.ops == ops and w.status == (W.ERR_NOMATCH if c.get("nomatch") else 0), what
        cx.poke(0, work, cells)
        cx.upload()
        if cx.batch_ok and both:
            cx.batch([w], what)
        cx.single(0, w, st, what)
        if cells:
            ij = np.asarray(cells)
            work[ij[:, 0], ij[:, 1]] = base[ij[:, 0], ij[:, 1]]
            cx.poke(0, base, cells)


@pytest.mark.parametrize("shape", W.SHAPES_B, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", list(KINDS))
def test_constructed_paths(dev, LB, kind, shape):
    """W.path_cases: long gaps inside a stripe row and straight up, reopened gaps and corners, staircases, the four
    edges, the border in each state, diagonal runs at every alignment of the ops; SW: local starts on the boundaries
    and at every step of a window; NW_ALIGN: a "no predecessor" byte on the path (MSA_ERR_NOMATCH)."""
    cx = Ctx(LB, dev, kind, [shape])
    cases = W.path_cases(shape[0], shape[1], cx.R, local=cx.wkind == "sw")
    if kind == "nw":
        cases["nomatch"] = dict(segs=[("M", 50), ("D", 3), ("M", 20)], local_stop=False, nomatch=True)
    _paths(cx, cases, (kind, shape))


@pytest.mark.parametrize("band", W.BANDS)
def test_constructed_paths_banded(dev, LB, band):
    """Banded NW_ALIGN, 700 x 700: paths on either band edge and one that switches between them."""
    cx = Ctx(LB, dev, "nw", [(W.BAND_M, W.BAND_M)], band=band)
    cases = {name: dict(segs=segs, local_stop=False) for name, segs in W.band_cases(band).items()}
    _paths(cx, cases, ("nw", "band", band))


# ---- c. / d. the long vertical-dominant path ---------------------------------------------------------------------
def _tall(dev, LB, kind, shape, caps):
    import time

    t0 = time.perf_counter()
    m, n = shape
    cx = Ctx(LB, dev, kind, [shape])
    ops = W.tall_ops(m, n)
    p = W.random_plane(cx.wkind, m, n, 0.5, "tall")
    W.apply_path(cx.wkind, p, ops, (m, n))
    st = 3 if cx.wkind in ("tag", "ref") else 1   # (the path starts with 'I')
    w = cx.reference(0, p, st, (kind, shape))
    assert w.ops == ops
    cx.load([p], 0x0F)
    for cap in caps:
        cx.single(0, w, st, (kind, shape, "cap", cap), cap=cap)
    dt = time.perf_counter() - t0
    print(kind, shape, "whole case: %.2f s" % dt)
    return cx, w


@pytest.mark.parametrize("kind", ["nw", "tag_flow"])
def test_ring_laps(dev, LB, kind):
    """>= 71,680 ops at no more than 7 per ring word: the walker waits on `consumed`, the decoder wraps, both ring
    halves are entered again twice.  Then the same walk into 1,000 bytes: MSA_ERR_CAPACITY, the true count, the first
    1,000 ops, nothing past them."""
    _, w = _tall(dev, LB, kind, W.RING_SHAPE, (None, W.CAP))
    assert len(w.ops) >= W.RING_MIN_OPS


def test_more_stripes_than_staged_starts(dev, LB):
    """8,194 stripes: the last two stripe starts come from memory, not from the 8,192 staged in LDS."""
    cx, w = _tall(dev, LB, "nw", W.STARTS_SHAPE, (None,))
    assert W.n_stripes(cx.geom[0]) > W.TB_CSL and W.stripes_entered(cx.geom[0], w.cells) == W.n_stripes(cx.geom[0])


# ---- e. a real noisy pair ----------------------------------------------------------------------------------------
def test_noisy_pair_sw_affine(oracle, dev, LB):
    """6,000 rows at 8 % substitutions and 6 % indels, filled and walked by the SW-affine single-pair plan."""
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    A, B = W.noisy_pair()
    ma, mi, go, ge = W.NOISY["sw"]
    pl = Plan(LB.SW_AFFINE, LB.CELLS_DIR, [len(A)], [len(B)], [0], [0], match=ma, mismatch=mi, gap_open=go,
              gap_extend=ge, track_end=True, single=True)
    assert pl.launch_info()["mode"] == "flow" and pl.launch_info()["rows_per_lane"] == 2
    D = torch.empty(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(torch.from_numpy(_codes(A)).to(dev), torch.from_numpy(_codes(B)).to(dev), D)
    tb, r = pl.traceback(D), pl.results()[0]
    o = oracle.sw(A, B, ma, mi, go, ge, want_tb=True)
    assert (r["score"], tuple(r["end"]), tuple(tb["beg"]), tb["cigar"]) == \
        (o["score"], tuple(o["end"]), tuple(o["beg"]), o["cigar"])
    assert W.gap_runs(tb["ops"]) >= W.NOISY["min_gap_runs"]
    assert pl.error() == 0


def test_noisy_pair_gotoh(oracle, dev, LB):
    """The same pair, filled and walked by the reference-Gotoh single-pair plan against the oracle's node list."""
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    A, B = W.noisy_pair()
    g, h = W.NOISY["gh"]
    pl = Plan(LB.REF_GOTOH, LB.CELLS_DIR, [len(A)], [len(B)], [0], [0], match=1, mismatch=0, gap_open=g + h,
              gap_extend=g, start_type=-1, single=True)
    assert pl.launch_info()["mode"] == "flow" and pl.launch_info()["rows_per_lane"] == 2
    D = torch.empty(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(torch.from_numpy(_codes(A)).to(dev), torch.from_numpy(_codes(B)).to(dev), D)
    tb = pl.traceback_gotoh(D, end_type=-1)
    o = oracle.subproblem_align(A, B, -1, -1, float(g), float(h))
    want = "".join("MDI"[t - 1] for (_, _, t) in reversed(o["nodes"]))
    assert tb["ops"].decode() == want
    assert W.gap_runs(tb["ops"]) >= W.NOISY["min_gap_runs"]
    assert pl.error() == 0
