"""Seed chaining on the device: msa_chain_run, msa_chain_seeds_batch and api.chain_seeds / api.chain_align against the
yardstick tests/chain_reference.py.  Integer arithmetic: every comparison is for equality -- f, pred, chain_of, n_chains
and chain_score.

Window and ring edges: lookback 1, 63, 64 (one chunk of 64 lanes exactly), 65 (the second chunk holds one lane) and 130
(three chunks) over problems of 1, 2, 64, 65 and 300 anchors -- fewer anchors than the lookback, more than the ring's
128, 192 or 256 entries (it wraps), a last block of 64 with one anchor in it.  The anchors lie on D interleaved
diagonals further apart than the band, so an anchor's best predecessor is about D places back: with D = 90 only the
third chunk of lookback 130 reaches it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import chain_reference as CR
import extend_band_reference as XB
import seed_reference as SR

pytestmark = pytest.mark.gpu

ARG = -1
POISON = -77
LOOKBACKS = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _sorted(a, b, ln):
    order = CR.sort_order(a, b, ln)
    return tuple([int(x[t]) for t in order] for x in (a, b, ln))


def _diagonals(seed, n, D, spacing=50):
    """n anchors of 8-15 symbols on D diagonals `spacing` apart (in A: B's coordinate orders them), advancing 1-3
    symbols per anchor, in (be, ae) order."""
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.integers(1, 4, size=n))
    diag = rng.integers(0, D, size=n) * spacing
    ln = rng.integers(8, 16, size=n)
    return _sorted(pos + diag, pos, ln)


def _round_robin(n, D, spacing=50):
    """Anchor t = 10 symbols ending at B's t + 10 on diagonal t mod D: its only admissible predecessors under a band
    below `spacing` are t - D, t - 2 D, ..."""
    t = np.arange(n)
    return _sorted(t + (t % D) * spacing, t, np.full(n, 10))


@functools.lru_cache(maxsize=None)
def _edge_problems():
    return (_diagonals(11, 1, 1), _diagonals(12, 2, 1), _diagonals(13, 64, 3), _round_robin(65, 64),
            _round_robin(300, 65), _round_robin(300, 129), _diagonals(15, 300, 90))


def _c_batch(LB, problems, **kw):
    """msa_chain_seeds_batch over problems in order -> per problem dict(f, pred, chain_of, n_chains, chain_score)."""
    off = np.concatenate(([0], np.cumsum([len(p[0]) for p in problems]))).astype(np.int64)
    a, b, ln = (np.array([x for p in problems for x in p[k]], dtype=np.int64) for k in range(3))
    n = max(int(off[-1]), 1)
    f, pred, co, sc = (np.full(n, POISON, dtype=np.int32) for _ in range(4))
    nc = np.full(len(problems), POISON, dtype=np.int32)
    par = dict(match=1, gap_open=3, gap_extend=1, band=0, max_dist=5000, lookback=64, min_score=0)
    par.update(kw)
    LB.check(LB.lib().msa_chain_seeds_batch(_p(a), _p(b), _p(ln), len(problems), _p(off), par["match"],
                                            par["gap_open"], par["gap_extend"], par["band"], par["max_dist"],
                                            par["lookback"], par["min_score"], _p(f), _p(pred), _p(co), _p(nc), _p(sc)),
             "msa_chain_seeds_batch")
    out = []
    for p in range(len(problems)):
        lo, hi = int(off[p]), int(off[p + 1])
        out.append(dict(f=f[lo:hi].tolist(), pred=pred[lo:hi].tolist(), chain_of=co[lo:hi].tolist(),
                        n_chains=int(nc[p]), chain_score=sc[lo:lo + int(nc[p])].tolist()))
    return out


def _refs(problems, **kw):
    return [CR.chain_reference(*p, **kw) for p in problems]


# ---- 1. window and ring edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookback", LOOKBACKS)
def test_window_and_ring_edges(dev, LB, lookback):
    problems = _edge_problems()
    assert [len(p[0]) for p in problems] == [1, 2, 64, 65, 300, 300, 300]
    kw = dict(band=4, max_dist=400, lookback=lookback, min_score=12)
    want = _refs(problems, **kw)
    assert _c_batch(LB, problems, **kw) == want
    # what the round-robin problems are there for: a predecessor exactly 64, 65 and 129 places back, which lookback
    # 64 (the last lane of one chunk), 65 (the one lane of a second chunk) and 130 (the third chunk) are the first to see
    assert want[3]["pred"][64] == (0 if lookback >= 64 else -1)
    assert want[4]["pred"][100] == (35 if lookback >= 65 else -1) and want[4]["f"][299] == (50 if lookback >= 65 else 10)
    assert want[5]["pred"][200] == (71 if lookback >= 129 else -1)
    assert lookback == 1 or any(j >= 0 for j in want[6]["pred"])


# ---- 2. the batch's shape, on device arrays --------------------------------------------------------------------------
def _run_device(LB, dev, problems, match=1, gap_open=3, gap_extend=1, band=0, max_dist=5000, lookback=64):
    """msa_chain_run over poisoned outputs -> (f, pred per problem, status)."""
    import torch

    off = np.concatenate(([0], np.cumsum([len(p[0]) for p in problems]))).astype(np.int64)
    cols = [torch.from_numpy(np.array([x for p in problems for x in p[k]], dtype=np.int64)).to(dev) for k in range(3)]
    d_off = torch.from_numpy(off).to(dev)
    f, pred = (torch.full((int(off[-1]),), POISON, dtype=torch.int32, device=dev) for _ in range(2))
    status = torch.full((len(problems) + 2,), POISON, dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    LB.check(LB.lib().msa_chain_run(ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), len(problems), ptr(d_off), match, gap_open,
                                    gap_extend, band, max_dist, lookback, ptr(f), ptr(pred), ptr(status), st),
             "msa_chain_run")
    torch.cuda.synchronize(dev)
    f, pred = f.cpu().numpy(), pred.cpu().numpy()
    return ([f[off[p]:off[p + 1]].tolist() for p in range(len(problems))],
            [pred[off[p]:off[p + 1]].tolist() for p in range(len(problems))], status.cpu().numpy().tolist())


def test_six_problems_one_empty_one_unsorted(dev, LB):
    """Six problems (no multiple of the four of a workgroup) of different N; one has no anchors, one is out of order:
    its status is ARG, nothing else is written for it, and its neighbours' results are the yardstick's."""
    good = [_diagonals(21, 70, 3), _diagonals(22, 5, 1), _diagonals(23, 130, 8), _diagonals(24, 1, 1)]
    bad = _diagonals(25, 40, 2)
    bad = tuple(x[:5] + [x[30]] + x[6:30] + [x[5]] + x[31:] for x in bad)   # anchors 5 and 30 swapped
    assert not CR.is_sorted(*bad)
    problems = [good[0], ([], [], []), good[1], bad, good[2], good[3]]
    kw = dict(band=4, max_dist=300, lookback=65)
    f, pred, status = _run_device(LB, dev, problems, **kw)
    assert status == [0, 0, 0, ARG, 0, 0, POISON, POISON]
    assert f[3] == [POISON] * 40 and pred[3] == [POISON] * 40
    for p in (0, 2, 4, 5):
        r = CR.chain_reference(*problems[p], **kw)
        assert (f[p], pred[p]) == (r["f"], r["pred"]), p
    # the other rules: a negative coordinate, len 0, an end above 2^26 -- each its own problem's status
    rules = [([0, -1], [0, 5], [4, 4]), ([0, 9], [0, 9], [4, 0]), ([0, (1 << 26) - 3], [0, 9], [4, 4]), good[1]]
    f, pred, status = _run_device(LB, dev, rules, **kw)
    assert status[:4] == [ARG, ARG, ARG, 0] and f[0] == f[1] == f[2] == [POISON] * 2
    assert f[3] == CR.chain_reference(*good[1], **kw)["f"]


# ---- 3. content ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _read(seed=31, m=420, cut=200):
    """(A, B, anchors in the caller's order): B is A with 3 % substitutions and a 6-base deletion at `cut`; the anchors
    are the 12-mers at stride 5 (neighbours overlap by 7) on both sides of the deletion, none for 30 symbols around it
    (the region between is 30 x 24), one pair of anchors that leaves 3 symbols of A alone, every fourth anchor twice
    (equal scores on purpose), and decoys on diagonals 150 and -120 away."""
    rng = np.random.default_rng(seed)
    A = XB.rs(rng, m)
    b = bytearray(A)
    for t in np.flatnonzero(rng.random(m) < 0.03):
        b[t] = b"ACGT"[(b"ACGT".index(b[t]) + 1 + int(rng.integers(0, 3))) % 4]
    del b[cut:cut + 6]
    B = bytes(b)
    anchors = []
    for a0 in range(0, m - 12, 5):
        if a0 + 12 <= cut - 12:
            anchors.append((a0, a0, 12))
        elif a0 >= cut + 18 and a0 <= m - 25:
            anchors.append((a0, a0 - 6, 12))
    anchors += anchors[::4]
    anchors.append((m - 10, m - 19, 10))   # after (m - 25, m - 31, 12): da = 13, db = 10, 3 symbols of A stay alone
    anchors += [(a0, a0 + 150, 12) for a0 in range(3, 200, 11) if a0 + 162 <= len(B)]
    anchors += [(a0, a0 - 120, 12) for a0 in range(130, 330, 13) if a0 + 12 <= m]
    order = rng.permutation(len(anchors))
    return A, B, [anchors[t] for t in order]


@pytest.mark.parametrize("band,max_dist,lookback", [(8, 60, 64), (8, 20, 130), (200, 5000, 64), (200, 300, 130),
                                                    (0, 5000, 64)])
def test_edited_copy_with_decoys(dev, LB, band, max_dist, lookback):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, anchors = _read()
    a, b, ln = ([t[k] for t in anchors] for k in range(3))
    problem = _sorted(a, b, ln)
    assert len(a) > 64    # more than one block of anchors
    for kw in (dict(), dict(match=2, gap_open=4, gap_extend=2, min_score=30), dict(gap_open=0, gap_extend=0)):
        kw = dict(kw, band=band, max_dist=max_dist, lookback=lookback)
        want = CR.chain_reference(*problem, **kw)
        assert _c_batch(LB, [problem], **kw) == [want]
        # the same through the api, from the caller's shuffled order
        assert api.chain_seeds(a, b, ln, **kw) == CR.chains(a, b, ln, **kw)
    want = CR.chain_reference(*problem, band=band, max_dist=max_dist, lookback=lookback)
    ties = sum(1 for i, j in enumerate(want["pred"]) if j > 0 and problem[0][j] == problem[0][j - 1]
               and problem[1][j] == problem[1][j - 1])
    assert ties > 5      # predecessors that are the later of two equal anchors
    best = CR.chains(a, b, ln, band=band, max_dist=max_dist, lookback=lookback)[0]
    if band == 8 and max_dist == 60:   # the best chain crosses the deletion and holds no decoy
        assert (best["a_beg"], best["b_beg"], best["a_end"], best["b_end"]) == (0, 0, len(A), len(B) - 3)
        assert all(0 <= a[t] - b[t] <= 9 for t in best["anchors"])
    if max_dist == 20:                 # the window is deeper than max_dist reaches (the walk of it stops early), and
        assert best["a_end"] - best["a_beg"] < 230   # the deletion is too far to cross
    if band == 0:                      # ... band 0 cannot
        assert best["a_end"] - best["a_beg"] < 230


# ---- 4. the alignment through the best chain -------------------------------------------------------------------------
def _merge(runs):
    out = []
    for run, op in runs:
        if run and out and out[-1][1] == op:
            out[-1] = (out[-1][0] + run, op)
        elif run:
            out.append((run, op))
    return "".join(f"{run}{op}" for run, op in out)


def _by_hand(api, A, B, anchors, w, xdrop, chain_kw, kw, traceback=True):
    """chain_align's result from calls the library had before it: the yardstick's chain and plan, api.nw_align_batch on
    the regions between anchors, api.extend_align_batch on the two flanks cut by hand (the left one reversed)."""
    al, S = kw["alphabet"], np.asarray(kw["matrix"])
    g, h = kw["gap_extend"], kw["gap_open"] - kw["gap_extend"]
    a, b, ln = ([t[k] for t in anchors] for k in range(3))
    # (chain_align's chain_gap_open / chain_gap_extend default to the alignment's)
    found = CR.chains(a, b, ln, band=w, gap_open=kw["gap_open"], gap_extend=kw["gap_extend"], **chain_kw)
    if not found:
        return None
    ch = found[0]
    plan = CR.plan(a, b, ln, ch["anchors"])
    score, runs = 0, []
    both = [p for p in plan["parts"] if p[0] == "gap" and p[2] > p[1] and p[4] > p[3]]
    fills = iter(api.nw_align_batch([A[p[1]:p[2]] for p in both], [B[p[3]:p[4]] for p in both], band=w,
                                    traceback=traceback, **kw) if both else [])
    for kind, a0, a1, b0, b1 in plan["parts"]:
        if kind == "seed":
            score += SR.seed_score(A, B, a0, b0, a1 - a0, al, S)
            runs.append((a1 - a0, "M"))
        elif a1 > a0 and b1 > b0:
            r = next(fills)
            score += r["score"]
            runs += SR.parse_cigar(r["cigar"]) if traceback else []
        else:
            L = (a1 - a0) + (b1 - b0)
            score -= h + g * L
            runs.append((L, "I" if a1 > a0 else "D"))
    (la, lb), (ra, rb) = plan["left"], plan["right"]
    cut = [(A[:la][::-1], B[:lb][::-1]), (A[ra:], B[rb:])]
    live = [k for k, (x, y) in enumerate(cut) if x and y]
    ext = api.extend_align_batch([cut[k][0] for k in live], [cut[k][1] for k in live], band=w, xdrop=xdrop,
                                 traceback=traceback, **kw) if live else []
    empty = dict(score=0, a_end=0, b_end=0, diagonals=0, dropped=False, cigar="")
    L, R = (dict(zip(live, ext)).get(k, empty) for k in (0, 1))
    flank = lambda f: {k: f[k] for k in ("score", "a_end", "b_end", "diagonals", "dropped")}  # noqa: E731
    r = dict(score=L["score"] + score + R["score"], a_beg=la - L["a_end"], b_beg=lb - L["b_end"], a_end=ra + R["a_end"],
             b_end=rb + R["b_end"], chain_score=ch["score"], anchors=ch["anchors"], left=flank(L), right=flank(R))
    if traceback:
        r["cigar"] = _merge(SR.parse_cigar(L["cigar"])[::-1] + runs + SR.parse_cigar(R["cigar"]))
    return r


def _consumed(cigar):
    runs = SR.parse_cigar(cigar)
    return sum(n for n, op in runs if op != "D"), sum(n for n, op in runs if op != "I")


@pytest.mark.parametrize("xdrop", [-1, 15])
def test_chain_align(dev, xdrop):
    from cse305_parallel_sequence_alignment_amd import api

    al, S, g, h = XB.score_set("dna")
    kw = dict(alphabet=al, matrix=S, gap_open=g + h, gap_extend=g)
    w = 16
    chain_kw = dict(max_dist=60, lookback=64, min_score=20)
    A0, B0, anc0 = _read()
    A1, B1, anc1 = _read(seed=32, m=300, cut=140)
    # flanks on both sides: the pairs inside longer sequences, the anchors moved with them
    rng = np.random.default_rng(41)
    pa, pb = XB.rs(rng, 37), XB.rs(rng, 55)
    A1, B1 = pa + A1 + XB.rs(rng, 20), pb + B1 + XB.rs(rng, 31)
    anc1 = [(x + 37, y + 55, l) for x, y, l in anc1 if 60 <= x <= 230]   # (60 similar symbols beyond the chain)
    pairs = [(A0, B0, [t for t in anc0 if abs(t[0] - t[1]) < 50]), (A1, B1, anc1),
             (A0, B0, [(100, 100, 25)]),   # a single anchor: seed_align's answer
             (A1, B1, [])]                 # none
    cols = lambda k: [[t[k] for t in p[2]] for p in pairs]  # noqa: E731
    for tb in (True, False):
        got = api.chain_align_batch([p[0] for p in pairs], [p[1] for p in pairs], cols(0), cols(1), cols(2), w,
                                    xdrop=xdrop, traceback=tb, **chain_kw, **kw)
        want = [_by_hand(api, A, B, anchors, w, xdrop, chain_kw, kw, tb) for A, B, anchors in pairs]
        assert got == want
        assert got[3] is None and all(("cigar" in r) == tb for r in got[:3])
        A, B, anchors = pairs[1]
        assert api.chain_align(A, B, *([t[k] for t in anchors] for k in range(3)), w, xdrop=xdrop, traceback=tb,
                               **chain_kw, **kw) == got[1]
    full =api.chain_align_batch([p[0] for p in pairs], [p[1] for p in pairs], cols(0), cols(1), cols(2), w,
                                 xdrop=xdrop, **chain_kw, **kw)
    for r, (A, B, _) in zip(full[:3], pairs):
        beg, end = (r["a_beg"], r["b_beg"]), (r["a_end"], r["b_end"])
        assert SR.rescore(r["cigar"], A, B, beg, end, al, S, g, h) == r["score"]
        assert _consumed(r["cigar"]) == (end[0] - beg[0], end[1] - beg[1])
    # what the cases are there for: a two-sided region and a one-sided one in the first chain, flanks in the second
    seed = api.seed_align(A0, B0, 100, 100, 25, w, xdrop=xdrop, **kw)
    assert {k: full[2][k] for k in ("score", "a_beg", "b_beg", "a_end", "b_end", "left", "right", "cigar")} == \
        {k: seed[k] for k in ("score", "a_beg", "b_beg", "a_end", "b_end", "left", "right", "cigar")}
    parts = CR.plan(*([t[k] for t in pairs[0][2]] for k in range(3)), full[0]["anchors"])["parts"]
    gaps = [p for p in parts if p[0] == "gap"]
    assert any(p[2] > p[1] and p[4] > p[3] for p in gaps) and any((p[2] - p[1]) * (p[4] - p[3]) == 0 for p in gaps)
    assert any(p[0] == "seed" and p[2] - p[1] == 5 for p in parts)     # a trimmed anchor
    assert full[1]["left"]["score"] > 0 and full[1]["right"]["score"] > 0
    assert full[1]["left"]["dropped"] == (xdrop >= 0)
