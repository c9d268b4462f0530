"""The plans, inputs and expected results of the plan-reuse tests (not a test file; no GPU needed to import it).

A plan is built once and run many times, and it owns device state that one run writes and the next must not see: the
ticket line with the fused best-cell key, the per-stripe meta, the {epoch, value} granules, the pass-2 block bests, the
staged code copies, the chunked band state and the result records both walkers start from.  Every case here is one plan
description -- of the shape tests/golden/plan_shapes.json records as the smallest that reaches its launch family, or a
SHAPES / BATCH entry of the reference modules for the table-scored kinds -- with an ordered list of inputs of the plan's
fixed lengths, chosen so that stale state wins if it survives:

  hi    a similar pair (one sequence is the other with a few substitutions and a short deletion and insertion): a
        large result whose end cell lies in the last stripe (an extension's: as far down as the shorter sequence goes);
  lo    local and free-end kinds: a 12-symbol planted match in the first stripe, in a low lane, over a background in
        which nothing scores above 0 (the rows repeat one symbol z, the columns use only symbols b with S[z][b] <= 0):
        a small score and an early end cell.  Global kinds: an unrelated random pair; fit: a copy with four symbols
        in ten replaced, at the reference's start;
  mid   a different similar pair whose end cell lies in a middle stripe and another lane (fit: in another column
        block; global: only the score differs);
  zero  local and free-end kinds: that background alone -- nothing positive, the empty result (score 0 at (0, 0), an
        overlap's at (m, 0)) and an empty walk.  Global and fit kinds: lo's again, the fit's copy two thirds along;
  hi2   another similar pair: the step low -> high.

The order is hi, lo, mid, zero, hi2 (the 1,000 x 3,000 pairs stop after zero; the 70,000-row, the 25,000- and
33,000-column and the 4,000 x 4,000 cases after mid); a batch runs five times and rotates the kinds over its pairs, pair
k of run r getting kind (k + r) mod 4, so that every per-pair slot goes high -> low and low -> high.
The chunked band cases run similar -> random -> similar.  tests/test_reuse_cases.py asserts on the references alone that
the inputs do dominate each other as claimed; tests/test_gpu_plan_reuse.py runs them.
"""
from __future__ import annotations

import functools
import importlib.util
import zlib
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import extend_reference as ER
import fit_reference as FR
import nw_reference as R
import nw_scored_reference as RS
import overlap_reference as OR
import profile_reference as PR
import sw_scored_reference as SR
import wide_reference as W

_spec = importlib.util.spec_from_file_location("make_plan_shapes", Path(__file__).resolve().parent / "golden" /
                                               "make_plan_shapes.py")
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)
SHAPE = {c["name"]: c for c in MK.CASES}

# the public algorithm and cell constants of _lib.py (restated: this module imports without the library)
SW_LINEAR, SW_AFFINE, NW_BANDED, REF_GOTOH, PARTIAL, NW_ALIGN, NW_SCORED, NW_FIT, SW_SCORED, NW_OVERLAP, NW_EXTEND = \
    range(11)
NONE, H, DIR, TAB = 0, 1, 2, 3
ALG_NAMES = ["SW_LINEAR", "SW_AFFINE", "NW_BANDED", "REF_GOTOH", "PARTIAL", "NW_ALIGN", "NW_SCORED", "NW_FIT",
             "SW_SCORED", "NW_OVERLAP", "NW_EXTEND"]

# msa_alg.h's result rules, by public algorithm
RULE = {SW_LINEAR: "RES_BEST", SW_AFFINE: "RES_BEST", SW_SCORED: "RES_BEST", NW_BANDED: "RES_FINAL",
        REF_GOTOH: "RES_FINAL", PARTIAL: "RES_FINAL", NW_ALIGN: "RES_FINAL", NW_SCORED: "RES_FINAL",
        NW_FIT: "RES_ROW_M", NW_OVERLAP: "RES_ROW_M_COL", NW_EXTEND: "RES_BEST_ANY"}
FREE_END = ("RES_BEST", "RES_ROW_M_COL", "RES_BEST_ANY")  # the rules with a planted lo and an empty result

KINDS = ("hi", "lo", "mid", "zero", "hi2")
RANK = {"hi": 3, "hi2": 3, "mid": 2, "lo": 1, "zero": 0, "sim": 3, "sim2": 3, "rnd": 0}
CHUNKED_KINDS = ("sim", "rnd", "sim2")


# ---- scorings -----------------------------------------------------------------------------------------------------
def _quiet(al: bytes, S):
    """(z, cols): the row symbol z with the most column symbols b of S[z][b] <= 0, and those symbols."""
    S = np.asarray(S)
    z = int(np.argmax((S <= 0).sum(axis=1)))
    cols = bytes(al[b] for b in np.flatnonzero(S[z] <= 0))
    assert len(cols) >= 2
    return al[z:z + 1], cols


def scoring(al: bytes, S, g: int, h: int) -> SimpleNamespace:
    """A table scoring: alphabet, S[row symbol][column symbol], gap_extend g, gap_open - gap_extend h."""
    z, cols = _quiet(al, S)
    return SimpleNamespace(al=al, S=np.asarray(S, dtype=np.int64), g=g, h=h, z=z, cols=cols)


def dna(match: int, mismatch: int, gap_open: int, gap_extend: int) -> SimpleNamespace:
    """Match / mismatch over ACGT through the plan description."""
    assert mismatch <= 0
    sc = scoring(b"ACGT", RS.match_mismatch(b"ACGT", match, mismatch), gap_extend, gap_open - gap_extend)
    sc.mm = (match, mismatch, gap_open, gap_extend)
    return sc


DNA_SET = scoring(*RS.SCORE_SETS["dna"])                      # +2 / -3, g = 2, h = 3, as an 8 x 8 table
SW7 = scoring(SR.AL7, SR.T7, SR.GE, SR.GO - SR.GE)            # the dense 7-symbol table of the SW_SCORED tests
SW31 = scoring(SR.AL31, SR.T31, SR.GE, SR.GO - SR.GE)
NW32 = scoring(W.AL32, W.table32(), 1, 2)
FIT20 = scoring(W.AL20, W.protein20(), 1, 10)
PROT24 = scoring(ER.AL24, W.table32()[:24, :24], 2, 9)


# ---- inputs -------------------------------------------------------------------------------------------------------
def _rnd(rng, n: int, al: bytes) -> bytes:
    return rng.choice(np.frombuffer(al, dtype=np.uint8), n).tobytes()


def _mutate(rng, s: bytes, al: bytes, frac: float, indel=True) -> bytes:
    """s with about `frac` of its symbols replaced by another one; 60 symbols and more: also a two-symbol deletion
    and a two-symbol insertion (the same length again).  frac 0: s itself."""
    t = bytearray(s)
    if frac <= 0 or not t:
        return bytes(t)
    for k in rng.choice(len(t), size=max(1, int(len(t) * frac)), replace=False):
        t[k] = al[(al.index(t[k]) + 1 + int(rng.integers(len(al) - 1))) % len(al)]
    if indel and len(t) >= 60:
        a = len(t) // 3
        del t[a:a + 2]
        b = 2 * len(t) // 3
        t[b:b] = _rnd(rng, 2, al)
    return bytes(t)


def segments(kind: str, rule: str, m: int, n: int):
    """[(row offset, column offset, length, mutated fraction)]: where the rows copy the columns."""
    L = min(m, n)
    s12 = min(12, L)
    if rule == "RES_ROW_M" and kind in ("lo", "zero"):
        # (all but unrelated: four symbols in ten differ; what is left puts the row maximum in a column block of
        # its own)
        return [(m - L, 0 if kind == "lo" else 2 * (n - L) // 3, L, 0.4)]
    if kind in ("rnd", "zero") or (kind == "lo" and rule not in FREE_END):
        return []
    if kind in ("hi", "hi2", "sim", "sim2"):
        frac = 0.02 if kind.startswith("sim") else 0.03
        return [(0, 0, L, frac)] if rule == "RES_BEST_ANY" else [(m - L, n - L, L, frac)]
    if kind == "lo":
        if rule == "RES_BEST_ANY":
            return [(0, 0, s12, 0.0)]
        if rule == "RES_ROW_M_COL":
            return [(0, n - s12, s12, 0.0)]
        return [(min(5, m - s12), min(20, n - s12), s12, 0.0)]
    assert kind == "mid"
    if rule == "RES_BEST_ANY":
        return [(0, 0, min(L, L // 2 + 3), 0.08)]
    if rule == "RES_ROW_M_COL":
        return [(0, n - max(1, L // 2), max(1, L // 2), 0.08)]
    if rule == "RES_BEST":
        L2 = max(1, L // 2)
        return [(min(m // 4, m - L2), min(n // 4 + 7, n - L2), L2, 0.08)]
    if rule == "RES_ROW_M":
        return [(m - L, (n - L) // 3, L, 0.12)]
    return [(m - L, n - L, L, 0.2)]


def make_rows(kind: str, rule: str, m: int, B: bytes, sc, rng) -> bytes:
    """The row sequence of a pair of the kind, for the column sequence B."""
    quiet = rule in FREE_END and kind not in ("sim", "sim2", "rnd")
    A = bytearray(sc.z * m if quiet else _rnd(rng, m, sc.al))
    for ai, bj, L, frac in segments(kind, rule, m, len(B)):
        # (under gap costs of 60 a band chunk's warm-up rows do not find a diagonal two columns off: no indels there)
        A[ai:ai + L] = _mutate(rng, B[bj:bj + L], sc.al, frac, indel=sc.g < 10)
    assert len(A) == m
    return bytes(A)


def make_cols(kind: str, rule: str, n: int, sc, rng, shared: bool) -> bytes:
    """A column sequence: over every symbol where the rows copy most of it, over the quiet symbols where the rows'
    background must score nothing against it (lo, zero, and a column sequence that several pairs share)."""
    quiet = rule in FREE_END and kind not in ("sim", "sim2", "rnd")
    return _rnd(rng, n, sc.cols if quiet and (shared or kind in ("lo", "mid", "zero")) else sc.al)


def profile_cols(kind: str, rule: str, P, n: int, al: bytes, rng) -> bytes:
    """A column sequence for the profile rows P (m x len(al)): the segments copy the rows' consensus; the quiet
    background is the alphabet's last symbol, which scores -3 in every row of profile_reference.specific_profile."""
    m = len(P)
    cons = PR.consensus(P, al)
    quiet = rule in FREE_END
    B = bytearray(al[-1:] * n if quiet else _rnd(rng, n, al[:-1]))
    for ai, bj, L, frac in segments(kind, rule, m, n):
        B[bj:bj + L] = _mutate(rng, cons[ai:ai + L], al[:-1], frac)
    assert len(B) == n
    return bytes(B)


# ---- the case table -----------------------------------------------------------------------------------------------
PROFILE_ROWS = 330


PROFILE_SLICES = [(0, 200), (37, 150), (253, 77)]  # (a_off, m): the second starts inside the profile, the third ends it


@functools.lru_cache(maxsize=None)
def profile_of(mode: str):
    """profile_reference.specific_profile's 330 rows (preferred symbols of codes 0..22, repeating every 21 rows); rows
    5..16 of every slice prefer one of codes 23..28 instead, which no other row does, so that the 12 symbols lo plants
    there fit nowhere else."""
    P = PR.specific_profile(950 + PR.MODES.index(mode), PROFILE_ROWS, len(PR.alphabet_of(mode)))
    for a, _ in PROFILE_SLICES:
        for r in range(a + 5, a + 17):
            P[r, int(P[r].argmax())] = -2
            P[r, 23 + r % 6] = 9
    return P


def _offs(lens):
    return [int(x) for x in np.concatenate(([0], np.cumsum(lens)[:-1]))]


def _tracking(c) -> str:
    """choose_algorithm's end-cell tracking mode (msa_plan.inc), restated."""
    if c.rule == "RES_BEST_ANY":
        return "select"
    if c.rule != "RES_BEST" or c.values == "packed16" or not (c.kw.get("track_end") or c.alg == SW_SCORED):
        return "none"
    S = profile_of(c.profile) if c.profile else c.sc.S if c.alg == SW_SCORED else np.asarray(c.sc.mm[:2])
    smax = max(0, int(S.max()))
    pack = all(smax * min(m, n) < 65536 and n + 512 < 32768 for m, n in zip(c.ms, c.ns))
    return "key" if pack else "select"


def case(name, family, alg, cells, ms, ns, sc, mode, *, b_offs=None, fill=False, values="int32", codes=8,
         profile=None, rows=None, kinds=KINDS, env=None, side_stream=False, int16_cells=0, items_gt1=False,
         score_sign=1, **kw):
    """One plan and what it must report.  ms / ns: the pairs' lengths (a_off: end to end; b_off: end to end unless
    b_offs shares column sequences); sc: its scoring; mode / fill: launch_info()'s mode and whether a separate pass-2
    launch is meant; values / codes / profile / int16_cells: format_info(); kw: the rest of the plan description.
    profile: the mode of a profile plan, whose pair k is profile rows rows[k] = (a_off, m).  kinds: the runs of a
    single pair.  score_sign: 0 where the final values of two runs only differ (the partial tables hold the
    reference's wrapped int32 costs, which have no order)."""
    c = SimpleNamespace(name=name, family=family, alg=alg, cells=cells, ms=list(ms), ns=list(ns), sc=sc, mode=mode,
                        fill=fill, values=values, codes=codes, profile=profile, rows=rows, kinds=tuple(kinds),
                        env=dict(env or {}), side_stream=side_stream, int16_cells=int16_cells, items_gt1=items_gt1,
                        score_sign=score_sign, kw=kw, rule=RULE[alg])
    c.a_offs = [a for a, _ in rows] if rows else _offs(ms)
    c.b_offs = list(b_offs) if b_offs is not None else _offs(ns)
    c.batch = len(c.ms) > 1
    c.n_runs = 5 if c.batch else len(c.kinds)
    c.tracking = _tracking(c)
    c.band = kw.get("band", -1)
    return c


def _from_shape(name, family, sc, mode, **over):
    """A case of make_plan_shapes.CASES, description and all (over: what this table changes or adds)."""
    s = SHAPE[name]
    kw = {k: s[k] for k in ("start_type", "band", "track_end", "single")}
    kw.update({k: over.pop(k) for k in list(over) if k in kw})
    if sc is None:
        sc = dna(s["match"], s["mismatch"], s["gap_open"], s["gap_extend"])
    return case(over.pop("as_name", name), family, s["alg"], s["cells"], s["ms"], s["ns"], sc, mode,
                b_offs=s["b_offs"], env=s["env"], **kw, **over)


B3 = ([200, 150, 77], [180, 200, 90])           # stripe_batch_h's recorded shape (nw_reference.BATCH_MS / BATCH_NS)
G3 = ([150, 100, 77], [180, 200, 90])           # ... with m <= n (the oracle's Subproblem swaps a taller pair)
T4 = (FR.BATCH_MS[:4], FR.BATCH_NS[:4])         # the table-scored modules': 200 x 700, 150 x 200, 77 x 90, 64 x 300
assert T4 == (ER.BATCH_MS[:2] + [77, 64], ER.BATCH_NS[:2] + [90, 300]) and B3 == (R.BATCH_MS, R.BATCH_NS)
W4 = ([m for m, _ in SR.BATCH[:2]] + [64, 70], [n for _, n in SR.BATCH[:2]] + [64, 40])  # 600 x 150: ten stripes
S13 = (1000, 3000)                              # single_1000x3000 of extend / overlap_reference, q1000_r3000 of fit
assert tuple(len(x) for x in ER.SHAPES["single_1000x3000"][1]()) == S13
assert tuple(len(x) for x in OR.SHAPES["single_1000x3000"]()) == S13
assert tuple(len(x) for x in FR.SHAPES["q1000_r3000"]()) == S13
CUT3 = KINDS[:3]                                # the long cases: three runs


def _table():
    T = []
    # ---- stripe kernel, batches of three or four ragged pairs
    T.append(case("batch_swl_h", "swl", SW_LINEAR, H, *B3, dna(2, -1, 1, 1), "stripe", track_end=1, single=0))
    T.append(case("batch_swa_dir", "swa", SW_AFFINE, DIR, *B3, dna(2, -3, 5, 2), "stripe", track_end=1, single=0))
    T.append(case("batch_gotoh_tab", "gotoh", REF_GOTOH, TAB, *G3, dna(1, 0, 3, 1), "stripe", start_type=1, single=0))
    T.append(case("batch_nw_align_dir", "nw_align", NW_ALIGN, DIR, *B3, dna(1, 0, 3, 1), "stripe", single=0))
    for fam, alg in (("nw_scored", NW_SCORED), ("fit", NW_FIT), ("overlap", NW_OVERLAP), ("extend", NW_EXTEND)):
        for cells in (DIR, NONE):
            T.append(case(f"batch_{fam}_{'dir' if cells == DIR else 'none'}", fam, alg, cells, *T4, DNA_SET, "stripe",
                          single=0))
    for cells in (DIR, NONE):
        T.append(case(f"batch_sw_scored_{'dir' if cells == DIR else 'none'}", "sw_scored", SW_SCORED, cells, *T4, SW7,
                      "stripe", single=0))
    T.append(case("batch_nw_scored_32", "nw_scored", NW_SCORED, DIR, *W4, NW32, "stripe", codes=32, single=0))
    T.append(case("batch_fit_32", "fit", NW_FIT, DIR, *T4, FIT20, "stripe", codes=32, single=0))
    T.append(case("batch_overlap_32", "overlap", NW_OVERLAP, DIR, *T4, PROT24, "stripe", codes=32, single=0))
    T.append(case("batch_extend_32", "extend", NW_EXTEND, DIR, *T4, PROT24, "stripe", codes=32, single=0))
    T.append(case("batch_sw_scored_32", "sw_scored", SW_SCORED, DIR, *W4, SW31, "stripe", codes=32, single=0))
    # the three profile modes: slices of one 330-row profile (the second and third start inside it)
    for mode, alg in (("local", SW_SCORED), ("global", NW_SCORED), ("fit", NW_FIT)):
        T.append(case(f"batch_profile_{mode}", "profile", alg, DIR, [m for _, m in PROFILE_SLICES], [300, 200, 150],
                      None, "stripe", codes=32, profile=mode, rows=PROFILE_SLICES, single=0))
    # ---- stripe kernel, one pair over several items
    T.append(case("single_extend_1000x3000", "extend", NW_EXTEND, DIR, [1000], [3000], DNA_SET, "stripe",
                  kinds=KINDS[:4], items_gt1=True, single=1))
    T.append(case("single_fit_1000x3000", "fit", NW_FIT, DIR, [1000], [3000], DNA_SET, "stripe", kinds=KINDS[:4],
                  items_gt1=True, single=1))
    T.append(case("single_overlap_1000x3000", "overlap", NW_OVERLAP, DIR, [1000], [3000], DNA_SET, "stripe",
                  kinds=KINDS[:4], items_gt1=True, single=1))
    T.append(case("single_nw_scored_330x300", "nw_scored", NW_SCORED, DIR, [330], [300], DNA_SET, "stripe",
                  items_gt1=True, single=1))
    T.append(case("single_sw_scored_330x300", "sw_scored", SW_SCORED, DIR, [330], [300], SW7, "stripe",
                  items_gt1=True, single=1))
    # (the scoring of the plan msa_partial_tables creates)
    part = dna(1, 0, 3, 1)
    part.mm = (0, 1, 3, 1)
    T.append(_from_shape("stripe_single_partial_tab", "partial", part, "stripe", as_name="single_partial_tab",
                         start_type=1, score_sign=0))
    # ---- split batch, packed score-only batches
    T.append(_from_shape("split_h", "swl", dna(2, -1, 1, 1), "split", track_end=1))
    T.append(_from_shape("cflow_4", "swl", None, "cflow", values="packed16"))
    T.append(_from_shape("cflow_4_lockstep", "swl", None, "stripe", values="packed16"))
    # (a 64-pair cut of packed_1024 keeps the packed format; it is few enough couples for cflow_kernel, whose items
    # of several pairs' stripes it queues 32 deep -- the lock-step kernel's batch mode is cflow_4_lockstep's)
    s = SHAPE["packed_1024"]
    T.append(case("packed_64", "swl", SW_LINEAR, NONE, s["ms"][:64], s["ns"][:64], dna(1, 0, 1, 1), "cflow",
                  b_offs=s["b_offs"][:64], values="packed16", single=0))
    # ---- flow kernel, pass 2 inside the launch
    T.append(_from_shape("flow_score", "swl", None, "flow"))
    T.append(_from_shape("flow_h_whole_rows", "swl", None, "flow"))
    T.append(_from_shape("flow_h_code_rings", "swl", None, "flow", kinds=CUT3))
    T.append(_from_shape("flow_h_end_packed", "swl", None, "flow"))
    T.append(_from_shape("flow_h_end_unpacked", "swl", None, "flow", kinds=CUT3))
    T.append(_from_shape("flow_h_floor", "swl", None, "flow"))
    T.append(_from_shape("flow_affine_dir_nneg", "swa", None, "flow"))
    T.append(_from_shape("flow_affine_dir_floor", "swa", None, "flow", side_stream=True))
    T.append(_from_shape("flow_gotoh_dir", "gotoh", None, "flow", values="tagged4"))
    # (recorded as the stripe kernel's: the Gotoh flow kernel is a fill, and a score-only plan has nothing to fill)
    T.append(_from_shape("flow_gotoh_score", "gotoh", None, "stripe", values="tagged4"))
    # ---- flow kernel with the fill launch
    T.append(_from_shape("fill_swl_h_end", "swl", None, "flow", fill=True, kinds=CUT3))
    T.append(_from_shape("fill_affine_floor", "swa", None, "flow", fill=True, kinds=CUT3))
    T.append(_from_shape("fill_gotoh", "gotoh", None, "flow", fill=True, values="tagged4", kinds=CUT3))
    # ---- band kernel
    T.append(_from_shape("band_exact_h", "banded", None, "band"))
    T.append(_from_shape("band_exact_score", "banded", None, "band", kinds=CUT3))
    T.append(_from_shape("band_chunked_h16", "banded", None, "band_chunked", kinds=CHUNKED_KINDS, int16_cells=1))
    T.append(_from_shape("band_chunked_i32", "banded", None, "band_chunked", kinds=CHUNKED_KINDS))
    return T


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
def kind_of(c, r: int, k: int) -> str:
    """The kind of pair k in run r."""
    return KINDS[(k + r) % 4] if c.batch else c.kinds[r]


@functools.lru_cache(maxsize=None)
def _inputs(name: str):
    c = BY_NAME[name]
    runs = []
    for r in range(c.n_runs):
        rng = np.random.default_rng([zlib.crc32(name.encode()), r])
        pairs, shared = [], {}
        for k, (m, n) in enumerate(zip(c.ms, c.ns)):
            kind = kind_of(c, r, k)
            if c.profile:
                al = PR.alphabet_of(c.profile)
                a = c.a_offs[k]
                pairs.append((None, profile_cols(kind, c.rule, profile_of(c.profile)[a:a + m], n, al, rng)))
                continue
            bo = c.b_offs[k]
            if bo not in shared:
                shared[bo] = make_cols(kind, c.rule, n, c.sc, rng, shared=c.b_offs.count(bo) > 1)
            pairs.append((make_rows(kind, c.rule, m, shared[bo], c.sc, rng), shared[bo]))
        runs.append(pairs)
    return runs


def inputs(c):
    """[[(A, B) per pair] per run]; a profile plan's A is None.  Computed once and shared (never modified)."""
    return _inputs(c.name)


def profile_rows(c, k: int):
    a, m = c.rows[k]
    return profile_of(c.profile)[a:a + m]


# ---- expected results (the references alone) ----------------------------------------------------------------------
def _oracle():
    """The oracle module (the tests' `oracle` fixture has built it; its lib() builds a missing library itself)."""
    from oracle import oracle as O

    return O


def gotoh_tables(O, A: bytes, B: bytes, st: int, g: int, h: int):
    """The oracle's three tables of the unswapped pair: its Subproblem swaps a tall pair (m > n), and the symmetric
    recurrence makes the unswapped tables its transposes with T2 <-> T3 (start type -1 only)."""
    T1, T2, T3, inv = O.subproblem_tables(A, B, st, float(g), float(h))
    if inv:
        assert st == -1
        T1, T2, T3 = T1.T.copy(), T3.T.copy(), T2.T.copy()
    return T1, T2, T3


def _expect_pair(c, k: int, A, B):
    """dict(score, end, ref): what results() must report for the pair (end None: not reported), and the family's
    reference object."""
    sc, m, n = c.sc, c.ms[k], c.ns[k]
    if c.family == "swl":
        ma, mi, go, ge = sc.mm
        o = _oracle().sw(A, B, ma, mi, go, ge, want_h=c.cells == H)
        return dict(score=o["score"], end=tuple(o["end"]) if c.kw.get("track_end") else None, ref=o)
    if c.family == "swa":
        o = _oracle().sw(A, B, *sc.mm, want_tb=True)
        return dict(score=o["score"], end=tuple(o["end"]), ref=o)
    if c.family == "gotoh":
        T = gotoh_tables(_oracle(), A, B, c.kw["start_type"], sc.g, sc.h)
        fin = tuple(float(t[m, n]) for t in T)
        return dict(score=int(max(fin)), end=(m, n), ref=dict(T=T, fin=fin))
    if c.family == "partial":
        T, _ = _oracle().partial_tables(A, B, float(sc.g), float(sc.h), c.kw["start_type"], 1)
        fin = tuple(int(t[m, n]) for t in T)
        return dict(score=max(fin), end=(m, n), ref=dict(T=T, fin=fin))
    if c.family == "banded":
        score, digest = _oracle().banded_ref(A, B, c.band, float(sc.g), float(sc.h), want_digest=True)
        return dict(score=int(score), end=(m, n), ref=dict(digest=digest))
    if c.family == "nw_align":
        ref = R.nw_reference(A, B, sc.g, sc.h, c.band)
        return dict(score=ref["score"], end=(m, n), ref=ref)
    if c.family == "profile":
        ref = PR.profile_reference(c.profile, profile_rows(c, k), B, PR.alphabet_of(c.profile))
        end = ref["end"] if c.profile == "local" else (m, n) if c.profile == "global" else (m, ref["end_j"])
        return dict(score=ref["score"], end=tuple(end), ref=ref)
    wide = c.codes == 32
    if c.family == "nw_scored":
        ref = (W.nw_reference32 if wide else RS.nw_scored_reference)(A, B, sc.al, sc.S, sc.g, sc.h, c.band)
        return dict(score=ref["score"], end=(m, n), ref=ref)
    if c.family == "fit":
        ref = (W.fit_reference32 if wide else FR.fit_reference)(A, B, sc.al, sc.S, sc.g, sc.h)
        return dict(score=ref["score"], end=(m, ref["end_j"]), ref=ref)
    if c.family == "overlap":
        ref = OR.overlap_reference(A, B, sc.al, sc.S, sc.g, sc.h)
        return dict(score=ref["score"], end=tuple(ref["end"]), ref=ref)
    if c.family == "extend":
        ref = ER.extend_reference(A, B, sc.al, sc.S, sc.g, sc.h)
        return dict(score=ref["score"], end=tuple(ref["end"]), ref=ref)
    assert c.family == "sw_scored"
    ref = SR.sw_scored_reference(A, B, sc.al, sc.S, sc.g + sc.h, sc.g)
    return dict(score=ref["score"], end=tuple(ref["end"]), ref=ref)


@functools.lru_cache(maxsize=2)
def _expected(name: str, r: int):
    c = BY_NAME[name]
    return [_expect_pair(c, k, A, B) for k, (A, B) in enumerate(inputs(c)[r])]


def expected(c, r: int):
    """Run r's expected result per pair.  Only the last two stay cached (a 70,000 x 300 Gotoh reference is three
    tables of doubles)."""
    return _expected(c.name, r)


def empty_end(c, k: int):
    """The end cell of the rule's empty result, or None where the rule has none."""
    return {"RES_BEST": (0, 0), "RES_BEST_ANY": (0, 0), "RES_ROW_M_COL": (c.ms[k], 0)}.get(c.rule)
