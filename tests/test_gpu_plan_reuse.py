"""One plan, run again on different inputs: every plan kind and launch family of tests/reuse_cases.py.

msa_plan_run's contract is "build once, run many times", and a plan owns device state that one run writes and the
next must not see: the ticket line with the fused best-cell key (only ever raised, by atomicMax), the per-stripe meta
(best, best_i, best_j, col_best, col_i, fin, has_fin, cs, phases), the {epoch, value} granules, the pass-2 block bests,
the staged code copies, the chunked band's ck / dk / okk / skip words and int16 cell plane, and the result records both
walkers start from.  Each case is checked in two ways:

  reuse     one plan, one set of output buffers and one ops / info buffer, every buffer filled with a non-zero
            pattern once and never cleared: the previous run's valid output is the strongest dirt there is.  The runs
            are reuse_cases' hi, lo, mid, zero, hi2 (a batch rotates them over its pairs; a chunked band runs similar,
            random, similar and must report converged 1, 0, 1), chosen -- and shown by test_reuse_cases.py on the
            references alone -- so that a tracker keeping an earlier maximum, a slot keeping its earlier occupant's
            end cell, a surviving skip / okk word, a walker starting from the previous end cell or a cell a shorter
            alignment leaves unwritten changes a checked value.
  recreate  hi on a plan, the plan destroyed and the same description created again (the pool hands back the same
            blocks): before any run the walkers of a fit, overlap or extension plan answer MSA_ERR_ARG, as
            test_gpu_extend.test_walk_before_any_run expects of fresh memory (msa.h promises it of those three kinds);
            then lo runs and is checked.

After each run everything the family's own test checks for a fresh plan is checked again, exactly (integer DP): score,
end cell, fin and status of results(), error() == 0, scores_into, every cell (the H checksum, the three table planes,
the direction bytes under the existing validity masks), and where the plan has a walker the single walk, the batch
walk and both once more into the test's own dirty ops / info buffers: ops byte for byte, stop / begin cell, the CIGAR
and the ops rescored.  The table-scored kinds call the _check helpers of test_gpu_extend / fit / overlap / nw_scored / sw_scored /
wide_alphabet / profile / nw_align as they are; the oracle-checked families (SW linear and affine, the reference's
Gotoh, the partial tables, banded H) repeat the comparisons of test_gpu_parity.py, whose checks create their own plans.
status == 0 after every run also shows has_fin set by that run: reduce_pairs_kernel clears it once reported.

One case (flow_affine_dir_floor) makes its second and later runs on a side stream, after synchronising the first, and
passes that stream to results, error, scores_into and the walks.
"""
import gc

import numpy as np
import pytest

import profile_reference as PR
import reuse_cases as RC
import sw_scored_reference as SR
import test_gpu_extend as EX
import test_gpu_fit as FT
import test_gpu_nw_align as NA
import test_gpu_nw_scored as NS
import test_gpu_overlap as OV
import test_gpu_parity as P
import test_gpu_profile as PRF
import test_gpu_sw_scored as SS
import test_gpu_wide_alphabet as WA
import wide_reference as W

pytestmark = pytest.mark.gpu

ARG = -1
MSA_NEG = -(1 << 30)  # -inf of the int32 table planes (msa_refwalk.h)
NW_WALK = (RC.NW_ALIGN, RC.NW_SCORED, RC.NW_FIT, RC.NW_OVERLAP, RC.NW_EXTEND)
SW_WALK = (RC.SW_AFFINE, RC.SW_SCORED)
U8_DIRT, I32_DIRT, I64_DIRT = 0xA5, 0x5A5A5A5A, 0x7777777777


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


class Reused:
    """A case's plan with its buffers: made once, dirtied once, never cleared."""

    def __init__(self, c, dev, LB, oracle):
        import torch
        from cse305_parallel_sequence_alignment_amd.plan import Plan

        self.c, self.dev, self.LB, self.O, self.torch = c, dev, LB, oracle, torch
        self.al = PR.alphabet_of(c.profile) if c.profile else c.sc.al
        self.dA = None if c.profile else torch.full((sum(c.ms),), U8_DIRT, dtype=torch.uint8, device=dev)
        self.dB = torch.full((max(o + n for o, n in zip(c.b_offs, c.ns)),), U8_DIRT, dtype=torch.uint8, device=dev)
        self.pl = self.make()
        planes = {RC.NONE: 0, RC.H: 1, RC.DIR: 1, RC.TAB: 3}[c.cells]
        dt, dirt = (torch.uint8, U8_DIRT) if c.cells == RC.DIR else (torch.int32, I32_DIRT)
        self.out = [torch.full((self.pl.cells_elems,), dirt, dtype=dt, device=dev) for _ in range(planes)]
        self.D = self.out[0] if planes else None
        self.off = Plan.ops_layout(c.ms, c.ns)
        self.d_off = torch.tensor(self.off, dtype=torch.int64, device=dev)
        self.ops = torch.full((self.off[-1],), U8_DIRT, dtype=torch.uint8, device=dev)
        self.info = torch.full((8 * len(c.ms),), I64_DIRT, dtype=torch.int64, device=dev)
        self.scores = torch.full((len(c.ms),), I32_DIRT, dtype=torch.int32, device=dev)
        self.walks = c.cells == RC.DIR and (c.alg in NW_WALK or c.alg in SW_WALK)

    def make(self):
        """The case's plan, on the launch path and in the formats the case names."""
        from cse305_parallel_sequence_alignment_amd.plan import Plan

        c, sc = self.c, self.c.sc
        if c.profile:
            kw = dict(gap_open=PR.GO, gap_extend=PR.GE, profile=PR.pad32(RC.profile_of(c.profile)))
        elif c.family in ("nw_scored", "fit", "overlap", "extend", "sw_scored"):
            kw = dict(gap_open=sc.g + sc.h, gap_extend=sc.g, sub=W.sub32(sc.S) if c.codes == 32 else SR.sub8(sc.S))
        else:
            kw = dict(zip(("match", "mismatch", "gap_open", "gap_extend"), sc.mm))
        pl = Plan(c.alg, c.cells, c.ms, c.ns, c.a_offs, c.b_offs, **kw, **c.kw)
        info, fmt = pl.launch_info(), pl.format_info()
        assert info["mode"] == c.mode and (info["fill_grid"] > 0) == c.fill, (c.name, info)
        assert (fmt["values"], fmt["tracking"], fmt["codes"], fmt["profile"]) == \
            (c.values, c.tracking, c.codes, bool(c.profile)), (c.name, fmt)
        assert fmt["int16_cells"] == c.int16_cells or c.mode != "band_chunked", (c.name, fmt)
        assert pl.single == (not c.batch) and (info["items"] > 1 or not c.items_gt1), (c.name, info)
        return pl

    def remake(self):
        """Destroy the plan and create its description again: the pool returns the same blocks."""
        del self.pl
        gc.collect()
        self.pl = self.make()

    def _codes(self, x):
        return self.torch.from_numpy(W.codes32(x, self.al).astype(np.uint8))

    def run(self, r, stream=None):
        c, pairs = self.c, RC.inputs(self.c)[r]
        if self.dA is not None:
            self.dA.copy_(self._codes(b"".join(A for A, _ in pairs)))
        hB = bytearray(len(self.dB))
        for (_, B), o in zip(pairs, c.b_offs):
            hB[o:o + len(B)] = B
        self.dB.copy_(self._codes(bytes(hB)))
        if stream is not None:
            self.torch.cuda.current_stream().synchronize()  # (the copies above: torch's current stream)
        self.pl.run(self.dA, self.dB, *self.out, stream=stream)

    # ---- what every family checks ------------------------------------------------------------------------------
    def check(self, r, stream=None):
        c, pl = self.c, self.pl
        exp = RC.expected(c, r)
        res = pl.results(stream)
        assert pl.error(stream) == 0
        for k, e in enumerate(exp):
            assert res[k]["score"] == e["score"], (r, k, res[k], e["score"], e["end"])
            assert e["end"] is None or tuple(res[k]["end"]) == e["end"], (r, k, res[k], e["end"])
            assert res[k]["status"] == 0, (r, k, res[k])
        pl.scores_into(self.scores, stream)
        if stream is not None:
            stream.synchronize()
        assert self.scores.cpu().tolist() == [e["score"] for e in exp], r
        getattr(self, "_" + c.family)(r, exp, res, stream)
        assert pl.error(stream) == 0

    def _host(self, t, stream=None):
        if stream is not None:
            stream.synchronize()
        return t.cpu().numpy()

    def _dirty_walk(self, k, tb, stream=None):
        """The single walk once more, into the ops / info buffers that hold the earlier walks' output."""
        pl, nw = self.pl, self.c.alg in NW_WALK
        (pl.traceback_nw_async if nw else pl.traceback_async)(self.out[0], self.ops, self.info, pair=k, stream=stream)
        inf = self._host(self.info, stream)[:8].tolist()
        assert inf[3] == 0, inf
        got = self._host(self.ops)[:inf[0]].tobytes()
        if nw:
            got += pl._border_gap(inf[1] - 1, inf[2] - 1)
            assert (inf[1] - 1, inf[2] - 1) == tuple(tb["stop"])
        else:
            assert not tb["ops"] or (inf[1], inf[2]) == tuple(tb["beg"])
        assert got == tb["ops"], (k, len(got), len(tb["ops"]))

    def _batch_walk(self, singles, stream=None):
        """The one-launch batch walk, through the plan's own fetch and into the dirty buffers, against the singles."""
        pl, nw = self.pl, self.c.alg in NW_WALK
        where = "stop" if nw else "beg"
        for one, tb in zip(singles, pl.traceback_batch(self.out[0], stream=stream)):
            assert (tb["ops"], tb["cigar"]) == (one["ops"], one["cigar"])
            assert not one["ops"] or tuple(tb[where]) == tuple(one[where])
        pl.traceback_batch_async(self.out[0], self.ops, self.d_off, self.info, stream=stream)
        inf, oh = self._host(self.info, stream).reshape(-1, 8), self._host(self.ops)
        for k, one in enumerate(singles):
            assert inf[k, 3] == 0, (k, inf[k])
            got = oh[self.off[k]:self.off[k] + int(inf[k, 0])].tobytes()
            if nw:
                got += pl._border_gap(int(inf[k, 1]) - 1, int(inf[k, 2]) - 1)
            assert got == one["ops"], k

    def _after_walks(self, singles, stream=None):
        if not self.walks:
            return
        for k, tb in enumerate(singles):
            self._dirty_walk(k, tb, stream)
        if self.c.batch:
            self._batch_walk(singles, stream)

    # ---- the oracle-checked families (test_gpu_parity.py's comparisons) -----------------------------------------
    def _swl(self, r, exp, res, stream):
        if self.c.cells == RC.H:
            for k, e in enumerate(exp):
                assert self.pl.checksum(self.out[0], pair=k, stream=stream) == self.O.checksum_h(e["ref"]["H"]), (r, k)

    def _swa(self, r, exp, res, stream):
        from cse305_parallel_sequence_alignment_amd.plan import Plan

        c, pl, D = self.c, self.pl, self.out[0]
        ma, mi, go, ge = c.sc.mm
        singles = []
        for k, ((A, B), e) in enumerate(zip(RC.inputs(c)[r], exp)):
            o = e["ref"]
            tb = pl.traceback(D, pair=k, stream=stream)
            assert tb["cigar"] == o["cigar"], (r, k)
            if o["score"] > 0:
                assert tuple(tb["beg"]) == tuple(o["beg"]), (r, k)
                assert P._rescore(A, B, tb["beg"], tb["cigar"], ma, mi, go, ge) == (o["score"], tuple(o["end"]))
            else:
                assert tb["ops"] == b""  # the empty alignment: no walk
            singles.append(tb)
        if c.mode != "flow":
            # the stripe kernel's bytes: bits 0-3 of every interior cell (SW_SCORED's format, which
            # test_gpu_sw_scored.test_null_sub_equals_affine_plan shows this plan to write)
            Dh, meta = self._host(D, stream), pl.stripe_meta(stream)
            for k, (A, B) in enumerate(RC.inputs(c)[r]):
                want = SR.sw_scored_reference(A, B, c.sc.al, c.sc.S, go, ge, walk=False)["byte"]
                bad = (pl.deskew_dir(Dh, k, meta)[1:, 1:] & 15) != (want[1:, 1:] & 15)
                assert not bad.any(), (r, k, int(bad.sum()), (np.argwhere(bad)[:4] + 1).tolist())
        elif not c.fill:
            # test_sw_affine_flow_dir_bytes: the flow kernel writes the byte of the stripe kernel's one-pair batch
            twin = Plan(c.alg, c.cells, c.ms, c.ns, [0], [0], match=ma, mismatch=mi, gap_open=go, gap_extend=ge,
                        track_end=True, single=False)
            assert twin.launch_info()["mode"] in ("stripe", "split")
            Dt = self.torch.empty(twin.cells_elems, dtype=self.torch.uint8, device=self.dev)
            twin.run(self.dA, self.dB, Dt)
            rt = twin.results()[0]
            assert (rt["score"], tuple(rt["end"])) == (exp[0]["score"], exp[0]["end"])
            d1 = pl.deskew_dir(self._host(D, stream), 0, pl.stripe_meta(stream))
            d0 = twin.deskew_dir(Dt.cpu().numpy(), 0, twin.stripe_meta())
            assert np.array_equal(d1[1:, 1:], d0[1:, 1:]), r
        self._after_walks(singles, stream)

    def _gotoh(self, r, exp, res, stream):
        c, pl = self.c, self.pl
        g, h = float(c.sc.g), float(c.sc.h)
        meta = pl.stripe_meta()
        for k, ((A, B), e) in enumerate(zip(RC.inputs(c)[r], exp)):
            T, m, n = e["ref"]["T"], c.ms[k], c.ns[k]
            assert tuple(float(x) for x in res[k]["fin"]) == e["ref"]["fin"], (r, k)
            if c.cells == RC.TAB:
                for v in range(3):
                    got = pl.deskew(self.out[v].cpu().numpy(), k, meta)[1:, 1:]
                    got = np.where(got == MSA_NEG, -np.inf, got.astype(np.float64))
                    bad = np.argwhere(got != T[v][1:, 1:])
                    assert len(bad) == 0, (r, k, f"T{v + 1}", len(bad), (bad[:4] + 1).tolist())
            if c.cells == RC.DIR:
                d = pl.deskew_dir(self.out[0].cpu().numpy(), k, meta)
                bad = np.argwhere((d[1:, 1:] & 63) != P._gotoh_tags(*T, g, h))
                assert len(bad) == 0, (r, k, len(bad), (bad[:4] + 1).tolist())
                if m <= n:  # (the oracle walks its own, swapped, tables of a taller pair)
                    tb = pl.traceback_gotoh(self.out[0], end_type=-1, pair=k)
                    o = self.O.subproblem_align(A, B, c.kw["start_type"], -1, g, h, tables=T)
                    ts = [t for (_, _, t) in o["nodes"]]
                    want = "".join("MDI"[t - 1] for t in reversed(ts)) if ts else "MDI"[o["end"][2] - 1]
                    assert tb["ops"].decode() == want, (r, k)
                    assert min(tb["stop"]) == 0 and max(tb["stop"]) >= 0, tb["stop"]

    def _partial(self, r, exp, res, stream):
        pl, meta = self.pl, self.pl.stripe_meta()
        for k, e in enumerate(exp):
            assert tuple(res[k]["fin"]) == e["ref"]["fin"], (r, k)
            for v in range(3):
                got = pl.deskew(self.out[v].cpu().numpy(), k, meta)[1:, 1:]
                bad = np.argwhere(got != e["ref"]["T"][v][1:, 1:])
                assert len(bad) == 0, (r, k, f"T{v + 1}", len(bad), (bad[:4] + 1).tolist())

    def _banded(self, r, exp, res, stream):
        c, pl = self.c, self.pl
        if c.cells == RC.H:
            assert pl.checksum(self.out[0]) == exp[0]["ref"]["digest"], r
        info = pl.run_info()
        if c.mode == "band_chunked":
            assert info["mode"] == "chunked" and info["chunks"] >= 2 and info["int16_cells"] == c.int16_cells, info
            assert info["converged"] == (0 if c.kinds[r] == "rnd" else 1), (r, c.kinds[r], info)
        else:
            assert info["mode"] == "stripe", info

    # ---- the families with a yardstick module: the existing _check helpers as they are -------------------------
    def _each(self, r, exp, check):
        """check(k, A, B, ref) for every pair of a plan with direction bytes; then the walks again."""
        if self.c.cells != RC.DIR:
            return
        singles = [check(k, A, B, e["ref"]) for k, ((A, B), e) in enumerate(zip(RC.inputs(self.c)[r], exp))]
        self._after_walks(singles)

    def _nw_align(self, r, exp, res, stream):
        c, sc, pl, D = self.c, self.c.sc, self.pl, self.D
        self._each(r, exp, lambda k, A, B, ref: NA._check(self.O, pl, D, A, B, c.band, sc.g, sc.h, ref, pair=k))

    def _nw_scored(self, r, exp, res, stream):
        c, sc, pl, D = self.c, self.c.sc, self.pl, self.D
        f = WA._check if c.codes == 32 else NS._check
        self._each(r, exp, lambda k, A, B, ref: f(pl, D, A, B, c.band, sc.al, sc.S, sc.g, sc.h, ref, pair=k))

    def _fit(self, r, exp, res, stream):
        c, sc, pl, D = self.c, self.c.sc, self.pl, self.D
        f = WA._check_fit if c.codes == 32 else FT._check
        self._each(r, exp, lambda k, A, B, ref: f(pl, D, A, B, sc.al, sc.S, sc.g, sc.h, ref, pair=k))

    def _overlap(self, r, exp, res, stream):
        sc, pl, D = self.c.sc, self.pl, self.D
        self._each(r, exp, lambda k, A, B, ref: OV._check(pl, D, A, B, sc.al, sc.S, sc.g, sc.h, ref, pair=k))

    def _extend(self, r, exp, res, stream):
        sc, pl, D = self.c.sc, self.pl, self.D
        for k, e in enumerate(exp):
            assert res[k]["fin"][0] == e["ref"]["global_score"], (r, k)
        self._each(r, exp, lambda k, A, B, ref: EX._check(pl, D, A, B, sc.al, sc.S, sc.g, sc.h, ref, pair=k))

    def _sw_scored(self, r, exp, res, stream):
        c, sc, pl, D = self.c, self.c.sc, self.pl, self.D
        self._each(r, exp, lambda k, A, B, ref: SS._check(pl, D, A, B, sc.al, sc.S, ref, c.codes, pair=k,
                                                          go=sc.g + sc.h, ge=sc.g))

    def _profile(self, r, exp, res, stream):
        c, pl, D = self.c, self.pl, self.D
        self._each(r, exp, lambda k, A, B, ref: PRF._check(c.profile, pl, D, RC.profile_rows(c, k), B, ref, pair=k))


@pytest.mark.parametrize("how", ["reuse", "recreate"])
@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_plan_reuse(oracle, dev, LB, monkeypatch, name, how):
    import torch

    c = RC.BY_NAME[name]
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)  # (read per plan, at creation)
    run = Reused(c, dev, LB, oracle)
    if how == "reuse":
        side = torch.cuda.Stream(device=dev) if c.side_stream else None
        for r in range(c.n_runs):
            stream = side if r >= 1 else None
            if stream is not None:
                torch.cuda.synchronize(dev)  # the earlier run and its checks, whichever stream they used
            run.run(r, stream)
            run.check(r, stream)
        return
    run.run(0)
    exp = RC.expected(c, 0)
    assert [x["score"] for x in run.pl.results()] == [e["score"] for e in exp] and run.pl.error() == 0
    run.remake()
    if c.cells == RC.DIR and c.alg in (RC.NW_FIT, RC.NW_OVERLAP, RC.NW_EXTEND):
        # no end cell yet, whatever the blocks held: msa_plan_create fills these kinds' result records
        assert _status(lambda: run.pl.traceback_nw(run.out[0])) == ARG
        if c.batch:
            assert _status(lambda: run.pl.traceback_batch(run.out[0])) == ARG
    run.run(1)
    run.check(1)
