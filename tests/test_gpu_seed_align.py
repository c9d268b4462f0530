"""Seed extension on the device: msa_xdrop_flank_run's per-pair reading direction, and api.seed_align /
api.seed_align_batch against the yardstick tests/seed_reference.py and against api.extend_align_batch on flanks cut and
reversed by hand -- the acceptance criterion proper: every field equal, `diagonals`, `dropped` and the CIGAR included.

Device level.  A pair read backwards in place (step -1 over buffers that hold the pairs forwards, offsets at each
flank's last byte) must give, byte for byte, what a forward run gives on reversed copies: the eight result words, the
whole band-form plane (the 0xFF poison outside the cells included), the walk's ops, its stop cell and its info words.
Six pairs (no multiple of the four of a workgroup) of 150-300 symbols whose neighbours in the buffer hold different
content, the first at an offset > 0, so a read one byte off lands on foreign symbols; bands 0, 16 (one chunk of 64
lanes), 64 (65 cells: the second chunk holds one lane, the first band at which the chunk loop's own loads run) and 130
(three chunks)."""
import ctypes as C
import functools

import numpy as np
import pytest

import extend_band_reference as XB
import extend_reference as ER
import seed_reference as SR
import xdrop_reference as XD

pytestmark = pytest.mark.gpu

ARG = -1
POISON_DIR, POISON_OPS = 0xFF, 0xEE


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _t(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _table32(S):
    S = np.asarray(S)
    out = np.zeros((32, 32), dtype=np.int8)
    out[:S.shape[0], :S.shape[1]] = S
    return out.reshape(-1)


def _run(LB, dev, bufA, bufB, tasks, S, g, h, w, xdrop, steps="extend"):
    """msa_xdrop_flank_run (steps: None, or one int per task) or msa_xdrop_extend_run (steps="extend"), then
    msa_xdrop_extend_walk, over the code buffers bufA / bufB and the tasks (m, n, a_off, b_off), sizes clipped already
    -> per task dict(res = the 8 result words, byte = the band-form plane, ops, stop, info, tail = the task's ops bytes
    past n_ops)."""
    import torch

    K = len(tasks)
    ms, ns, ao, bo = (np.array([t[k] for t in tasks], dtype=np.int64) for k in range(4))
    dA, dB = _t(np.asarray(bufA, dtype=np.uint8), dev), _t(np.asarray(bufB, dtype=np.uint8), dev)
    doff = np.concatenate(([0], np.cumsum((2 * w + 1) * (ms + 1)))).astype(np.int64)
    ooff = np.concatenate(([0], np.cumsum((ms + ns + 2 + 15) // 16 * 16))).astype(np.int64)
    dm, dn, dao, dbo, ddoff, dooff = (_t(x, dev) for x in (ms, ns, ao, bo, doff, ooff))
    tab = _t(_table32(S), dev)
    dDir = torch.full((int(doff[-1]),), POISON_DIR, dtype=torch.uint8, device=dev)
    dOps = torch.full((int(ooff[-1]),), POISON_OPS, dtype=torch.uint8, device=dev)
    dRes = torch.zeros(8 * K, dtype=torch.int64, device=dev)
    dInfo = torch.zeros(8 * K, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = LB.lib()
    tail = (_ptr(tab), 0, 0, g + h, g, w, xdrop, _ptr(dDir), _ptr(ddoff), _ptr(dRes), st)
    if isinstance(steps, str):
        LB.check(L.msa_xdrop_extend_run(_ptr(dA), _ptr(dB), K, _ptr(dm), _ptr(dn), _ptr(dao), _ptr(dbo), *tail),
                 "msa_xdrop_extend_run")
    else:
        dStep = None if steps is None else _t(np.array(steps, dtype=np.int8), dev)
        LB.check(L.msa_xdrop_flank_run(_ptr(dA), _ptr(dB), K, _ptr(dm), _ptr(dn), _ptr(dao), _ptr(dbo),
                                       None if dStep is None else _ptr(dStep), *tail), "msa_xdrop_flank_run")
    LB.check(L.msa_xdrop_extend_walk(K, w, _ptr(dDir), _ptr(ddoff), _ptr(dRes), _ptr(dOps), _ptr(dooff), _ptr(dInfo),
                                     st), "msa_xdrop_extend_walk")
    torch.cuda.synchronize(dev)
    res, info = dRes.cpu().numpy().reshape(K, 8), dInfo.cpu().numpy().reshape(K, 8)
    byte, ops = dDir.cpu().numpy(), dOps.cpu().numpy()
    out = []
    for p in range(K):
        seg = ops[ooff[p]:ooff[p + 1]]
        n_ops = int(info[p, 0])
        out.append(dict(res=[int(x) for x in res[p]], byte=byte[doff[p]:doff[p + 1]].reshape(int(ms[p]) + 1, 2 * w + 1),
                        ops=seg[:n_ops].tobytes(), stop=(int(info[p, 1]) - 1, int(info[p, 2]) - 1),
                        info=[int(x) for x in info[p]], tail=seg[n_ops:]))
    return out


def _same(got, want):
    """Two tasks of _run, field by field."""
    assert got["res"] == want["res"]
    assert got["byte"].shape == want["byte"].shape and (got["byte"] == want["byte"]).all(), \
        ("band-form plane", np.argwhere(got["byte"] != want["byte"])[:4])
    assert (got["ops"], got["stop"], got["info"]) == (want["ops"], want["stop"], want["info"])
    assert (got["tail"] == POISON_OPS).all() and (want["tail"] == POISON_OPS).all()


@functools.lru_cache(maxsize=None)
def _six():
    """The six flank pairs, as the byte strings a LEFT flank's extension runs on (nearest the seed first): similar
    pairs with substitutions and indels, one clipped by every band here (150 x 300), one that X-drop stops early, one
    where the other side is the longer.  Pairwise different content."""
    pairs = []
    for k, m in enumerate((150, 211, 300)):   # (the first without indels: never stopped, even by band 0)
        pairs.append(XB.similar(np.random.default_rng(700 + k), m, sub=0.04 + 0.01 * k, indel=0.005 * k))
    rng = np.random.default_rng(710)
    P = XB.rs(rng, 150)
    pairs.append((P, P[:70] + XB.rs(rng, 230)))          # 150 x 300: clipped; the tail is unrelated
    pairs.append(ER._prefix(711, 40, 200, 180))          # stops soon after 40 common symbols
    q = XB.rs(rng, 170)
    pairs.append((q[:90] + q[96:] + XB.rs(rng, 60), q))  # 224 x 170, a 6-symbol deletion at 90
    return tuple(pairs)


def _layouts(w):
    """(forward buffers and tasks with the offsets at each pair's LAST byte, reversed copies and tasks with the offsets
    at each pair's first byte): the same six clipped pairs both ways.  The buffers start with 7 foreign codes, and a
    pair's neighbours are other pairs."""
    al = b"ACGT"
    fa, fb, ra, rb, back, fwd = [np.array([3, 2, 1, 0, 3, 2, 1])], [np.array([0, 1, 2, 3, 0, 1, 2])], [], [], [], []
    pa = pb = 7
    qa = qb = 0
    for a, b in _six():
        m, n = XB.clip(len(a), len(b), w)
        fa.append(ER.codes(a[::-1], al))   # the buffer holds the sequence forwards: the flank is its reverse
        fb.append(ER.codes(b[::-1], al))
        ra.append(ER.codes(a, al))
        rb.append(ER.codes(b, al))
        back.append((m, n, pa + len(a) - 1, pb + len(b) - 1))
        fwd.append((m, n, qa, qb))
        pa, pb, qa, qb = pa + len(a), pb + len(b), qa + len(a), qb + len(b)
    return (np.concatenate(fa), np.concatenate(fb), back), (np.concatenate(ra), np.concatenate(rb), fwd)


BANDS = [0, 16, 64, 130]
XDROP = 30


# ---- 1. a pair read backwards in place is the forward run on its reversed copy ---------------------------------------
@pytest.mark.parametrize("w", BANDS)
def test_reversed_in_place(dev, LB, w):
    al, S, g, h = XB.score_set("dna")
    (bufA, bufB, back), (revA, revB, fwd) = _layouts(w)
    want = _run(LB, dev, revA, revB, fwd, S, g, h, w, XDROP)
    got = _run(LB, dev, bufA, bufB, back, S, g, h, w, XDROP, steps=[-1] * 6)
    for x, y in zip(got, want):
        assert x["res"][5] == 0 and x["info"][3] == 0
        _same(x, y)
    # ... and the forward run is the yardstick's: score, end cell, D (so the six pairs do what their names say)
    refs = [XD.xdrop_reference(a, b, al, S, g, h, w, XDROP) for a, b in _six()]
    for x, r in zip(got, refs):
        assert (x["res"][0], tuple(x["res"][1:3]), x["res"][3], x["res"][6]) == \
            (r["score"], r["end"], r["diagonals"], r["cells"])
        assert x["ops"] == r["walk_ops"] and x["stop"] == r["stop"]
    assert refs[4]["dropped"] and not refs[0]["dropped"]
    assert (refs[3]["m_eff"], refs[3]["n_eff"]) == (150, min(300, 150 + w))
    # (from band 64 on an anti-diagonal holds w + 1 > 64 cells once the rows allow it, so the chunk loop's own loads ran)
    assert min(r["m_eff"] for r in refs) > 130


# ---- 2. both directions in one launch --------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [16, 64])
def test_mixed_steps(dev, LB, w):
    al, S, g, h = XB.score_set("dna")
    (bufA, bufB, back), (revA, revB, fwd) = _layouts(w)
    steps = [1, -1, -1, 1, -1, 1]
    # one buffer holding both layouts: the forward-read tasks point into its second half
    offA, offB = len(bufA), len(bufB)
    tasks = [back[p] if s < 0 else (fwd[p][0], fwd[p][1], fwd[p][2] + offA, fwd[p][3] + offB)
             for p, s in enumerate(steps)]
    got = _run(LB, dev, np.concatenate((bufA, revA)), np.concatenate((bufB, revB)), tasks, S, g, h, w, XDROP,
               steps=steps)
    want = _run(LB, dev, revA, revB, fwd, S, g, h, w, XDROP)
    for x, y in zip(got, want):
        _same(x, y)


# ---- 3. no steps: msa_xdrop_extend_run, word for word ----------------------------------------------------------------
@pytest.mark.parametrize("w", [16, 130])
def test_null_step_is_the_forward_entry(dev, LB, w):
    al, S, g, h = XB.score_set("dna")
    _, (revA, revB, fwd) = _layouts(w)
    want = _run(LB, dev, revA, revB, fwd, S, g, h, w, XDROP)
    for steps in (None, [1] * 6):
        for x, y in zip(_run(LB, dev, revA, revB, fwd, S, g, h, w, XDROP, steps=steps), want):
            _same(x, y)


# ---- 4. a step that is neither +1 nor -1 -----------------------------------------------------------------------------
def test_bad_step_is_that_pairs_error(dev, LB):
    al, S, g, h = XB.score_set("dna")
    w = 16
    (bufA, bufB, back), (revA, revB, fwd) = _layouts(w)
    want = _run(LB, dev, revA, revB, fwd, S, g, h, w, XDROP)
    got = _run(LB, dev, bufA, bufB, back, S, g, h, w, XDROP, steps=[-1, 0, -1, 2, -1, -128])
    for p, (x, y) in enumerate(zip(got, want)):
        if p in (1, 3, 5):
            assert x["res"] == [0, 0, 0, 0, LB.SCORE_NONE, ARG, 0, 0]
            assert (x["byte"] == POISON_DIR).all() and x["ops"] == b"" and x["info"][3] == ARG
        else:
            _same(x, y)


# ---- the API ---------------------------------------------------------------------------------------------------------
def _kw(alphabet, S, g, h, w, xdrop):
    return dict(alphabet=alphabet, matrix=S, gap_open=g + h, gap_extend=g, band=w, xdrop=xdrop,
                max_symbols=32 if len(alphabet) > 8 else 8)


def _stitch(left, seed_len, right):
    """The CIGAR through a seed from its flanks' own CIGARs: the left one's runs turned round, seed_len M, the right
    one's, neighbouring runs of one op merged."""
    runs = SR.parse_cigar(left)[::-1] + ([(seed_len, "M")] if seed_len else []) + SR.parse_cigar(right)
    out = []
    for run, op in runs:
        if out and out[-1][1] == op:
            out[-1] = (out[-1][0] + run, op)
        else:
            out.append((run, op))
    return "".join(f"{run}{op}" for run, op in out)


def _by_hand(api, seeds, kw, traceback=True):
    """What the parent commit offers for the same answers: two extend_align_batch calls on flanks cut and reversed on the
    host (flanks without symbols on a side left out), the seed's score, the coordinates and the CIGARs glued."""
    S, al = np.asarray(kw["matrix"]), kw["alphabet"]
    cut = [SR.flanks(A, B, sa, sb, sl) for A, B, sa, sb, sl in seeds]
    empty = dict(score=0, a_end=0, b_end=0, diagonals=0, dropped=False, cigar="")
    sides = []
    for side in (0, 1):
        live = [p for p, c in enumerate(cut) if c[side][0] and c[side][1]]
        res = api.extend_align_batch([cut[p][side][0] for p in live], [cut[p][side][1] for p in live],
                                     traceback=traceback, **kw) if live else []
        by = dict(zip(live, res))
        sides.append([by.get(p, empty) for p in range(len(seeds))])
    out = []
    for (A, B, sa, sb, sl), L, R in zip(seeds, *sides):
        mid = SR.seed_score(A, B, sa, sb, sl, al, S)
        flank = lambda f: {k: f[k] for k in ("score", "a_end", "b_end", "diagonals", "dropped")}  # noqa: E731
        r = dict(score=L["score"] + mid + R["score"], a_beg=sa - L["a_end"], b_beg=sb - L["b_end"],
                 a_end=sa + sl + R["a_end"], b_end=sb + sl + R["b_end"], seed_score=mid, left=flank(L), right=flank(R))
        if traceback:
            r["cigar"] = _stitch(L["cigar"], sl, R["cigar"])
        out.append(r)
    return out


def _refs(seeds, al, S, g, h, w, xdrop):
    return [SR.seed_reference(A, B, sa, sb, sl, al, S, g, h, w, xdrop) for A, B, sa, sb, sl in seeds]


def _check_api(api, seeds, al, S, g, h, w, xdrop, Bs=None):
    """seed_align_batch (and seed_align on the first seed) against the yardstick and against the flanks by hand, with
    and without CIGARs.  -> the yardstick's dictionaries."""
    kw = _kw(al, S, g, h, w, xdrop)
    skw = {k: v for k, v in kw.items() if k not in ("band", "xdrop")}
    refs = _refs(seeds, al, S, g, h, w, xdrop)
    cols = [[s[k] for s in seeds] for k in range(5)]
    for tb in (True, False):
        got = api.seed_align_batch(cols[0], cols[1] if Bs is None else Bs, cols[2], cols[3], cols[4], w, xdrop=xdrop,
                                   traceback=tb, **skw)
        assert got == [SR.want(r, tb) for r in refs]
        assert got == _by_hand(api, seeds, kw, tb)
        A, B, sa, sb, sl = seeds[0]
        assert api.seed_align(A, B, sa, sb, sl, w, xdrop=xdrop, traceback=tb, **skw) == got[0]
    for r, (A, B, sa, sb, sl) in zip(refs, seeds):
        assert SR.rescore(r["cigar"], A, B, r["beg"], r["end"], al, S, g, h) == r["score"]
    return refs


@functools.lru_cache(maxsize=None)
def _similar_300():
    return XB.similar(np.random.default_rng(720), 300, sub=0.05, indel=0.01)


@pytest.mark.parametrize("xdrop", [20, -1])
@pytest.mark.parametrize("w", [16, 80])
@pytest.mark.parametrize("sset", ["dna", "asym"])
def test_similar_pairs(dev, sset, w, xdrop):
    """Seeds at a quarter, a half and three quarters of a ~300-symbol pair; "asym" scores differ between S[a][b] and
    S[b][a], so a table transposed for the reversed flank shows."""
    from cse305_parallel_sequence_alignment_amd import api

    A, B = _similar_300()
    al, S, g, h = XB.score_set(sset)
    assert sset != "asym" or (np.asarray(S) != np.asarray(S).T).any()
    seeds = [(A, B, q * len(A) // 4, q * len(A) // 4 - 1, 12) for q in (1, 2, 3)]
    refs = _check_api(api, seeds, al, S, g, h, w, xdrop)
    assert all(r["left"]["score"] > 0 and r["right"]["score"] > 0 for r in refs)


def test_wide_alphabet(dev):
    from cse305_parallel_sequence_alignment_amd import api

    A, B, al, S, g, h = ER.protein32()
    assert len(al) == 24
    seeds = [(A, B, 40, 40, 5), (A, B, 3, 4, 0)]   # (the pair's first 80 symbols are alike)
    for xdrop in (-1, 8):
        refs = _check_api(api, seeds, al, S, g, h, 16, xdrop)
        assert refs[0]["left"]["score"] > 0 and refs[0]["right"]["score"] > 0


def test_left_clip(dev):
    """seed_a = 30, seed_b = 300, band 16: B's left flank is clipped to the 46 symbols NEAREST the seed, so the window
    read backwards starts at the seed, not at B's first byte."""
    from cse305_parallel_sequence_alignment_amd import api

    al, S, g, h = XB.score_set("dna")
    rng = np.random.default_rng(721)
    P = XB.rs(rng, 30)
    A = P + XB.rs(rng, 40)
    B = XB.rs(rng, 270) + P + A[30:]
    ref, = _check_api(api, [(A, B, 30, 300, 10)], al, S, g, h, 16, -1)
    assert ref["left"]["end"] == (30, 30) and ref["left"]["diagonals"] == 30 + 46 and ref["beg"] == (0, 270)
    # ... and the mirror on the right: A's right flank is clipped to the 20 + 16 symbols nearest the seed
    ref, = _check_api(api, [(B, A, 300, 30, 20)], al, S, g, h, 16, -1)
    assert ref["right"]["diagonals"] == 20 + 20 and ref["left"]["diagonals"] == 46 + 30


def test_short_and_empty_flanks(dev):
    """A 1-symbol flank, every combination of empty flanks, and seed_len = 0."""
    from cse305_parallel_sequence_alignment_amd import api

    al, S, g, h = XB.score_set("dna")
    A, B = _similar_300()
    A, B = A[:120], B[:118]
    m, n = len(A), len(B)
    seeds = [(A, B, 1, 1, 8),              # a 1 x 1 left flank
             (A, B, 1, 40, 8),             # 1 x 40
             (A, B, m - 9, n - 9, 8),      # a 1 x 1 right flank
             (A, B, 0, 0, 8),              # the seed at (0, 0): no left flank
             (A, B, 0, 30, 8),             # ... on A's side alone
             (A, B, 50, 0, 8),             # ... on B's side alone
             (A, B, m - 8, n - 8, 8),      # the seed ending at (m, n): no right flank
             (A, B, m - 8, 60, 8),         # ... at m alone
             (A, A, 0, 0, m),              # the seed = both whole sequences: nothing to launch
             (A, B, 60, 60, 0),            # a bare anchor
             (A, B, 0, 0, 0), (A, B, m, n, 0), (A, B, 0, n, 0)]   # ... in three corners
    refs = _check_api(api, seeds, al, S, g, h, 16, 20)
    assert refs[3]["left"] == refs[6]["right"] == refs[8]["left"] == refs[8]["right"] == SR.EMPTY
    assert refs[8]["cigar"] == f"{m}M" and refs[9]["seed_score"] == 0 and refs[12]["cigar"] == ""
    for s in seeds:   # one by one through the single entry as well
        _check_api(api, [s], al, S, g, h, 16, 20)


def test_islands_drop_one_flank(dev):
    """Left of the seed a matching island, unrelated symbols, another island: xdrop 10 stops the left flank in the
    gap between them; the right flank matches to its end and is not dropped."""
    from cse305_parallel_sequence_alignment_amd import api

    al, S, g, h = XB.score_set("dna")
    rng = np.random.default_rng(722)
    far, near, right = XB.rs(rng, 70), XB.rs(rng, 50), XB.rs(rng, 90)
    seed = XB.rs(rng, 15)
    A = far + XB.rs(rng, 25) + near + seed + right
    B = far + XB.rs(rng, 25) + near + seed + right
    sa = 70 + 25 + 50
    ref, = _check_api(api, [(A, B, sa, sa, 15)], al, S, g, h, 32, 10)
    assert ref["left"]["dropped"] and not ref["right"]["dropped"]
    assert ref["left"]["end"] == (50, 50) and ref["right"]["end"] == (90, 90) and ref["beg"] == (95, 95)
    ref, = _check_api(api, [(A, B, sa, sa, 15)], al, S, g, h, 32, 60)   # a larger xdrop crosses the gap
    assert ref["beg"] == (0, 0) and ref["score"] > 2 * (50 + 15 + 90)


def test_batch_compaction(dev):
    """Five seeds, three of their ten flanks empty: seven launched tasks, neither a multiple of the four of a workgroup
    nor two per seed."""
    from cse305_parallel_sequence_alignment_amd import api

    al, S, g, h = XB.score_set("dna")
    pairs = [XB.similar(np.random.default_rng(730 + k), 90 + 17 * k, sub=0.05, indel=0.01) for k in range(5)]
    seeds = [(pairs[0][0], pairs[0][1], 0, 0, 10),                                   # no left flank
             (pairs[1][0], pairs[1][1], 50, 50, 10),
             (pairs[2][0], pairs[2][1], len(pairs[2][0]) - 6, len(pairs[2][1]) - 6, 6),   # no right flank
             (pairs[3][0], pairs[3][1], 70, 69, 0),
             (pairs[4][0], pairs[4][1], 20, 0, 9)]                                   # no left flank (seed_b == 0)
    refs = _check_api(api, seeds, al, S, g, h, 16, 25)
    assert sum(f == SR.EMPTY for r in refs for f in (r["left"], r["right"])) == 3


def test_many_seeds_one_reference(dev):
    """Eight reads seeded against one shared reference, given once as a bytes object."""
    from cse305_parallel_sequence_alignment_amd import api

    al, S, g, h = XB.score_set("dna")
    rng = np.random.default_rng(740)
    ref_b = XB.rs(rng, 400)
    seeds = []
    for k in range(8):
        at = 20 + 40 * k
        read = ER.edited(rng, ref_b[at:at + 90])
        seeds.append((read, ref_b, 40, at + 40, 6))
    _check_api(api, seeds, al, S, g, h, 16, 30, Bs=ref_b)


def test_two_seeds_on_one_pair(dev):
    from cse305_parallel_sequence_alignment_amd import api

    al, S, g, h = XB.score_set("dna")
    A, B = _similar_300()
    refs = _check_api(api, [(A, B, 60, 60, 10), (A, B, 220, 219, 14)], al, S, g, h, 16, -1)
    assert all(r[f]["score"] > 0 for r in refs for f in ("left", "right"))
