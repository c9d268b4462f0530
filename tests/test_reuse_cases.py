"""The plan-reuse case table (tests/reuse_cases.py) does what it claims, shown on the references alone (no GPU).

tests/test_gpu_plan_reuse.py runs every case's inputs through one plan, and it can only catch state that survives a run
if the next input's result differs from the last one's in the way stale state would betray.  Conditions, not
measurements: each holds for the references (oracle.*, extend_ / fit_ / overlap_ / profile_ / sw_scored_ / nw_ /
nw_scored_ / wide_reference), whatever the library does.

Dominations, for every case and every pair of consecutive runs of each pair slot (test_consecutive_runs_dominate):
  D1  the score is strictly lower where the kind's rank falls and strictly higher where it rises (hi > mid > lo >
      zero; similar > random); the partial plan's final values, wrapped int32 costs without an order, differ;
  D2  a zero run of a local, overlap or extension plan gives the empty result: score 0 at (0, 0), an overlap's at
      (m, 0);
  D3  where the plan reports an end cell: next to an empty result the two end cells differ; a fit's end columns lie
      in different 16-step blocks where the reference is 64 symbols longer than the query and more, and differ where
      it is not; any other two end cells of a pair of 192 rows and more lie in different 64-row
      stripes and in different lanes or 16-step blocks, and those of a shorter pair (too few stripes) differ;
  D4  a planted lo ends in the first stripe, a hi of a pair of m <= n rows in the last one;
  D5  every slot of a batch sees both directions, a fall and a rise, and so does every single pair with more than
      three runs; the three-run cases fall and then rise as well;
  D6  the chunked band cases run similar, random, similar.
Coverage (the test_covers_* functions):
  C1  every public algorithm constant of _lib.py, with this module's restated numbers equal to the library's;
  C2  both code widths, the three profile modes, all four cell kinds;
  C3  every launch mode of test_gpu_plan_shapes.MODES but "chunked" -- the stripe fallback of a chunked band, which
      only bands of 8,192 and up reach (plan_shapes.json's band_8192 ... band_32768 rows all still report
      band_chunked), so no test-sized plan runs it;
  C4  every result rule of msa_alg.h's enum, which RULE maps as the table there does;
  C5  every launch family the recorded shapes reach, under the recorded mode and pass-2 launch, and the separate
      pass-2 launch at all;
  C6  a case on a side stream, cases over several items, end-cell tracking by select and by key.
"""
import re
from pathlib import Path

import pytest

import reuse_cases as RC
import test_gpu_plan_shapes as PS

ROOT = Path(__file__).resolve().parent.parent
NAMES = [c.name for c in RC.CASES]


def _summary(c):
    """[[(score, end, fin) per pair] per run], the reference objects dropped as they come."""
    out = []
    for r in range(c.n_runs):
        out.append([(e["score"], e["end"], e["ref"].get("fin") if isinstance(e["ref"], dict) else None)
                    for e in RC.expected(c, r)])
    return out


def _stripe(i):
    return (i - 1) // 64


@pytest.mark.parametrize("name", NAMES)
def test_consecutive_runs_dominate(oracle, name):
    c = RC.BY_NAME[name]
    runs = _summary(c)
    assert c.n_runs >= 3 and len(RC.inputs(c)) == c.n_runs
    for k, (m, n) in enumerate(zip(c.ms, c.ns)):
        for A, B in (run[k] for run in RC.inputs(c)):
            assert (c.profile or len(A) == m) and len(B) == n
        kinds = [RC.kind_of(c, r, k) for r in range(c.n_runs)]
        falls = rises = 0
        for r in range(c.n_runs):
            score, end, _ = runs[r][k]
            empty = kinds[r] == "zero" and c.rule in RC.FREE_END
            if empty:  # D2
                assert score == 0 and (end is None or end == RC.empty_end(c, k)), (r, k, score, end)
            if end is not None and c.rule in ("RES_BEST", "RES_BEST_ANY", "RES_ROW_M_COL"):  # D4
                if kinds[r] == "lo":
                    assert _stripe(end[0]) == 0, (r, k, end)
                if kinds[r] in ("hi", "hi2") and m <= n:
                    assert _stripe(end[0]) == _stripe(m), (r, k, end)
        for r in range(1, c.n_runs):
            (s0, e0, f0), (s1, e1, f1) = runs[r - 1][k], runs[r][k]
            up = RC.RANK[kinds[r]] > RC.RANK[kinds[r - 1]]
            assert RC.RANK[kinds[r]] != RC.RANK[kinds[r - 1]]
            falls, rises = falls + (not up), rises + up
            if c.score_sign == 0:  # D1, the partial plan
                assert f0 != f1, (r, k, f0, f1)
            else:
                assert (s1 > s0) if up else (s1 < s0), (r, k, kinds[r - 1], s0, kinds[r], s1)
            if e0 is None or c.rule == "RES_FINAL":
                continue
            empties = [RC.empty_end(c, k) if kd == "zero" and c.rule in RC.FREE_END else None
                       for kd in (kinds[r - 1], kinds[r])]
            if any(e is not None for e in empties):  # D3
                assert e0 != e1, (r, k, e0, e1)
            elif c.rule == "RES_ROW_M" and n - m >= 64:
                assert e0[1] // 16 != e1[1] // 16, (r, k, e0, e1)
            elif c.rule == "RES_ROW_M":
                assert e0 != e1, (r, k, e0, e1)
            elif m >= 192:
                assert _stripe(e0[0]) != _stripe(e1[0]), (r, k, e0, e1)
                assert (e0[0] - 1) % 64 != (e1[0] - 1) % 64 or e0[1] // 16 != e1[1] // 16, (r, k, e0, e1)
            else:
                assert e0 != e1, (r, k, e0, e1)
        assert falls >= 1 and rises >= 1, (k, kinds)  # D5
    if c.mode == "band_chunked":  # D6
        assert c.kinds == ("sim", "rnd", "sim2") and not c.batch


def test_covers_every_algorithm():
    """C1."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    public = {n: getattr(LB, n) for n in dir(LB) if re.fullmatch(r"(SW|NW|REF)_[A-Z]+|PARTIAL", n)}
    assert public == {n: getattr(RC, n) for n in RC.ALG_NAMES}
    assert {c.alg for c in RC.CASES} == set(public.values())
    assert (LB.CELLS_NONE, LB.CELLS_H, LB.CELLS_DIR, LB.CELLS_TAB) == (RC.NONE, RC.H, RC.DIR, RC.TAB)


def test_covers_code_widths_profiles_and_cells():
    """C2: each table-scored kind over 8 and over 32 codes, with direction bytes and score-only."""
    assert {c.codes for c in RC.CASES} == {8, 32}
    assert {c.profile for c in RC.CASES if c.profile} == {"local", "global", "fit"}
    assert {c.cells for c in RC.CASES} == {RC.NONE, RC.H, RC.DIR, RC.TAB}
    for alg in (RC.NW_SCORED, RC.NW_FIT, RC.NW_OVERLAP, RC.NW_EXTEND, RC.SW_SCORED):
        mine = [c for c in RC.CASES if c.alg == alg and not c.profile]
        assert {(c.codes, c.cells) for c in mine} >= {(8, RC.DIR), (8, RC.NONE), (32, RC.DIR)}, alg


def test_covers_every_launch_mode():
    """C3: "chunked" is the stripe fallback of a chunked band whose band kernel does not fit; only bands of 8,192 and
    up reach it, and the recorded rows of that size still launch band_chunked."""
    assert {c.mode for c in RC.CASES} == set(PS.MODES) - {"chunked"}
    assert PS.MODES["chunked"] not in {rec["launch_info"][0] for rec in PS.RECORDED["cases"].values()
                                       if rec["status"] == 0}


def test_covers_every_result_rule():
    """C4."""
    text = (ROOT / "cse305_parallel_sequence_alignment_amd" / "csrc" / "msa_alg.h").read_text()
    rules = re.findall(r"\b(RES_[A-Z_]+) = \d", text[text.index("enum msa_result"):])
    assert len(rules) == 5 and {c.rule for c in RC.CASES} == set(rules)
    # the table of msa_alg.h: kernel algorithm -> rule, by the public algorithm that selects it
    kernel = {"SWL": RC.SW_LINEAR, "SWL0": RC.SW_LINEAR, "SWLP": RC.SW_LINEAR, "SWA": RC.SW_AFFINE,
              "SWS": RC.SW_SCORED, "SWS32": RC.SW_SCORED, "SWP": RC.SW_SCORED, "NWA32": RC.NW_SCORED,
              "NWP": RC.NW_SCORED, "FIT": RC.NW_FIT, "FIT32": RC.NW_FIT, "FITP": RC.NW_FIT, "OVL": RC.NW_OVERLAP,
              "OVL32": RC.NW_OVERLAP, "EXT": RC.NW_EXTEND, "EXT32": RC.NW_EXTEND, "REF": RC.REF_GOTOH,
              "REF1": RC.REF_GOTOH, "PART": RC.PARTIAL}
    rows = dict(re.findall(r"case MSA_ALG_(\w+):\s+return \{\d, \w+,\s+\w+, \w+, (RES_\w+),", text))
    assert set(rows) == set(kernel) | {"NWA"}  # (NWA: MSA_NW_BANDED, MSA_NW_ALIGN and MSA_NW_SCORED, all RES_FINAL)
    assert rows["NWA"] == "RES_FINAL" == RC.RULE[RC.NW_BANDED] == RC.RULE[RC.NW_ALIGN] == RC.RULE[RC.NW_SCORED]
    for name, alg in kernel.items():
        assert rows[name] == RC.RULE[alg], name


FAMILIES = ["split_h", "cflow_4", "cflow_4_lockstep", "flow_score", "flow_h_whole_rows", "flow_h_code_rings",
            "flow_h_end_packed", "flow_h_end_unpacked", "flow_h_floor", "flow_affine_dir_nneg",
            "flow_affine_dir_floor", "flow_gotoh_dir", "flow_gotoh_score", "fill_swl_h_end", "fill_affine_floor",
            "fill_gotoh", "band_exact_h", "band_exact_score", "band_chunked_h16", "band_chunked_i32"]


def test_covers_every_recorded_family():
    """C5: the cases named after a recorded shape keep its lengths and offsets, and the recording shows the launch
    mode and the pass-2 launch the case asserts."""
    for name in FAMILIES + ["stripe_single_partial_tab"]:
        c = RC.BY_NAME["single_partial_tab" if name == "stripe_single_partial_tab" else name]
        s, rec = RC.SHAPE[name], PS.RECORDED["cases"][name]
        assert (c.ms, c.ns, c.a_offs, c.b_offs) == (s["ms"], s["ns"], s["a_offs"], s["b_offs"]), name
        assert rec["status"] == 0 and rec["launch_info"][0] == PS.MODES[c.mode], name
        assert (rec["launch_info"][5] > 0) == c.fill, name
        if name in PS.REACHES:
            assert PS.REACHES[name] == (c.mode, c.fill), name
    assert sum(c.fill for c in RC.CASES) == 3
    cut = RC.BY_NAME["packed_64"]
    whole = RC.SHAPE["packed_1024"]
    assert (cut.ms, cut.ns, cut.b_offs) == (whole["ms"][:64], whole["ns"][:64], whole["b_offs"][:64])
    for name, int16 in (("band_chunked_h16", 1), ("band_chunked_i32", 0)):
        assert PS.RECORDED["cases"][name]["run_info_0_1_3"][2] >> 16 == RC.BY_NAME[name].int16_cells == int16


def test_covers_streams_items_and_tracking():
    """C6."""
    assert [c.name for c in RC.CASES if c.side_stream] == ["flow_affine_dir_floor"]
    assert {c.rule for c in RC.CASES if c.items_gt1} >= {"RES_FINAL", "RES_BEST", "RES_ROW_M", "RES_ROW_M_COL",
                                                         "RES_BEST_ANY"}
    assert {c.tracking for c in RC.CASES} == {"none", "select", "key"}
    assert RC.BY_NAME["flow_h_end_packed"].tracking == "key" and RC.BY_NAME["flow_h_end_unpacked"].tracking == "select"
    assert all(len(c.ms) in (3, 4) for c in RC.CASES if c.name.startswith("batch_"))
