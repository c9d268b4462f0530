"""Launch shapes of msa_plan_create, recorded per plan description (needs the MI355X).

    python tests/golden/make_plan_shapes.py

Every case of CASES only creates a plan and reads it back (no kernel runs): the status of
msa_plan_create and, on success, the 8 values of msa_plan_launch_info, the cells size, the stripe
count, every pair's 4 layout values and fields 0, 1 and 3 of msa_plan_run_info (field 2 reads a
device word that only a run writes).  Writes tests/golden/plan_shapes.json together with the
device's CU count and architecture name: grids and occupancies depend on both.
tests/test_gpu_plan_shapes.py replays the same table (CASES and probe() are shared) against the
recorded file, so a change of the host-side plan code that moves any launch shape, layout or
status shows there.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

OUT = HERE / "plan_shapes.json"

# diagnostic variables libmsa reads once per process: a recorded shape only holds with none of them set
ONCE_PER_PROCESS = ("MSA_FLOW_LDS_MIN", "MSA_BAND_WARM", "MSA_BAND_CHUNK", "MSA_BAND_H16")

SW_LINEAR, SW_AFFINE, NW_BANDED, REF_GOTOH, PARTIAL = 0, 1, 2, 3, 4
NONE, H, DIR, TAB = 0, 1, 2, 3


def case(name, alg, cells, ms, ns, b_offs=None, env=None, **kw):
    """One plan description: scores default to match 1 / mismatch 0 / gap 1; a_off and b_off are the
    pairs' sequences laid end to end unless b_offs says which column sequences are shared."""
    d = dict(match=1, mismatch=0, gap_open=1, gap_extend=1, start_type=-1, band=-1, track_end=0,
             single=int(len(ms) == 1))
    d.update(kw)
    a_offs = [sum(ms[:k]) for k in range(len(ms))]
    if b_offs is None:
        b_offs = [sum(ns[:k]) for k in range(len(ns))]
    return dict(name=name, alg=alg, cells=cells, ms=list(ms), ns=list(ns), a_offs=a_offs, b_offs=list(b_offs),
                env=dict(env or {}), **d)


CASES = [
    # ---- stripe_kernel, batch and single pair
    case("stripe_batch_h", SW_LINEAR, H, [200, 150, 77], [180, 200, 90]),
    case("stripe_batch_gotoh_tab_st1", REF_GOTOH, TAB, [100, 90], [100, 90], start_type=1, gap_open=3),
    case("stripe_single_gotoh_tab_st1", REF_GOTOH, TAB, [300], [280], start_type=1, gap_open=3),
    case("stripe_single_gotoh_dir_st1", REF_GOTOH, DIR, [300], [280], start_type=1, gap_open=3),
    case("stripe_single_partial_tab", PARTIAL, TAB, [300], [280], gap_open=3),
    case("stripe_single_sw_score_end", SW_LINEAR, NONE, [1000], [1000], track_end=1),
    case("stripe_single_nw_unbanded", NW_BANDED, H, [500], [480], band=-1),
    # ---- split batch: 18 stripes >= 2 * 8, fewer pairs than two workgroups per CU
    case("split_h", SW_LINEAR, H, [1100] * 4, [500] * 4),
    # ---- packed score-only batches: cflow_kernel or the lock-step stripe kernel
    case("cflow_4", SW_LINEAR, NONE, [500] * 4, [500] * 4, b_offs=[0, 0, 500, 500]),
    case("cflow_4_lockstep", SW_LINEAR, NONE, [500] * 4, [500] * 4, b_offs=[0, 0, 500, 500],
         env={"MSA_C4_KERNEL": "lockstep"}),
    case("packed_1024", SW_LINEAR, NONE, [100] * 1024, [100] * 1024, b_offs=[100 * (k // 2) for k in range(1024)]),
    case("packed_1024_cflow", SW_LINEAR, NONE, [100] * 1024, [100] * 1024,
         b_offs=[100 * (k // 2) for k in range(1024)], env={"MSA_C4_KERNEL": "cflow"}),
    case("unpacked_score_batch", SW_LINEAR, NONE, [500] * 4, [500, 400, 500, 400]),
    # ---- flow_kernel
    case("flow_score", SW_LINEAR, NONE, [1000], [1000]),
    case("flow_h_whole_rows", SW_LINEAR, H, [1000], [1000]),
    case("flow_h_code_rings", SW_LINEAR, H, [300], [25000]),
    case("flow_h_end_packed", SW_LINEAR, H, [1000], [1000], track_end=1),
    case("flow_h_end_unpacked", SW_LINEAR, H, [300], [33000], track_end=1),
    case("flow_h_floor", SW_LINEAR, H, [1000], [1000], match=2, mismatch=-1),
    case("flow_affine_dir_nneg", SW_AFFINE, DIR, [1000], [1000], track_end=1, gap_open=3, gap_extend=1),
    case("flow_affine_dir_floor", SW_AFFINE, DIR, [1000], [1000], track_end=1, match=2, mismatch=-3, gap_open=5,
         gap_extend=2),
    case("flow_gotoh_dir", REF_GOTOH, DIR, [1000], [1000], start_type=-1, gap_open=3),
    case("flow_gotoh_score", REF_GOTOH, NONE, [1000], [1000], start_type=-1, gap_open=3),
    # ---- flow with the separate pass-2 launch: 137 items > half the CUs
    case("fill_swl_h", SW_LINEAR, H, [70000], [300]),
    case("fill_swl_h_end", SW_LINEAR, H, [70000], [300], track_end=1),
    case("fill_affine", SW_AFFINE, DIR, [70000], [300], track_end=1, gap_open=3, gap_extend=1),
    case("fill_affine_floor", SW_AFFINE, DIR, [70000], [300], track_end=1, match=2, mismatch=-3, gap_open=5,
         gap_extend=2),
    case("fill_gotoh", REF_GOTOH, DIR, [70000], [300], start_type=-1, gap_open=3),
    # ---- band_kernel, exact and chunked
    case("band_exact_h", NW_BANDED, H, [1000], [1000], band=64),
    case("band_exact_score", NW_BANDED, NONE, [4000], [4000], band=64),
    case("band_chunked_h16", NW_BANDED, H, [2400], [2400], band=64),
    case("band_chunked_i32", NW_BANDED, H, [2400], [2400], band=512, gap_open=60, gap_extend=60),
    case("band_dir_unsupported", NW_BANDED, DIR, [1000], [1000], band=64),
    # ---- the search for the chunked stripe fallback (mode 2: band_kernel's LDS does not fit): bands doubling
    # from 8,192 at m = n = 2 band (gap 4: rows + gap * band > 30,000, so no int16 chunk cells are allocated)
    case("band_8192", NW_BANDED, H, [16384], [16384], band=8192, gap_open=4, gap_extend=4),
    case("band_16384", NW_BANDED, H, [32768], [32768], band=16384, gap_open=4, gap_extend=4),
    case("band_32768", NW_BANDED, H, [65536], [65536], band=32768, gap_open=4, gap_extend=4),
    # ---- one failing condition each
    case("bad_no_pairs", SW_LINEAR, H, [], []),
    case("bad_alg", 99, H, [100], [100]),
    case("bad_single_two_pairs", SW_LINEAR, H, [100, 100], [100, 100], single=1),
    case("bad_m_zero", SW_LINEAR, H, [0], [100]),
    case("bad_m_zero_batch", SW_LINEAR, H, [100, 0], [100, 100]),
    case("bad_band_violation", NW_BANDED, H, [500], [400], band=10),
    case("bad_swl_dir", SW_LINEAR, DIR, [100], [100]),
    case("bad_swl_tab", SW_LINEAR, TAB, [100], [100]),
    case("bad_swl_dir_batch", SW_LINEAR, DIR, [100, 90], [100, 90]),
    case("bad_swa_tab", SW_AFFINE, TAB, [100], [100], gap_open=3),
    case("bad_nw_dir", NW_BANDED, DIR, [100], [100]),
    case("bad_nw_tab", NW_BANDED, TAB, [100], [100]),
    case("bad_partial_h", PARTIAL, H, [100], [100]),
    case("bad_partial_none", PARTIAL, NONE, [100], [100]),
    case("bad_partial_dir", PARTIAL, DIR, [100], [100]),
    case("bad_nw_open_below_extend", NW_BANDED, H, [100], [100], gap_open=1, gap_extend=2),
    case("bad_linear_gap_negative", SW_LINEAR, H, [100], [100], gap_open=-1, gap_extend=-1),
    case("bad_linear_profile_byte", SW_LINEAR, H, [100], [100], match=100, gap_open=20, gap_extend=20),
    case("bad_affine_open_negative", SW_AFFINE, H, [100], [100], gap_open=-1, gap_extend=0),
    case("bad_batch_row_buffer_lds", SW_LINEAR, H, [100, 120], [60000, 60000]),
    # ---- two failing conditions at once: which status wins
    case("bad_single_two_pairs_and_cells", SW_LINEAR, DIR, [100, 100], [100, 100], single=1),
    case("bad_band_violation_and_open_below_extend", NW_BANDED, H, [500], [400], band=10, gap_open=1, gap_extend=2),
    case("bad_m_zero_and_cells", SW_LINEAR, DIR, [0], [100]),
]


def device_facts() -> dict:
    import torch

    p = torch.cuda.get_device_properties(0)
    return dict(cus=int(p.multi_processor_count), arch=str(p.gcnArchName).split(":")[0])


def probe(c: dict) -> dict:
    """Create the plan of case c, read it back, destroy it."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    saved = {k: os.environ.get(k) for k in c["env"]}
    os.environ.update(c["env"])
    try:
        n = len(c["ms"])
        arrs = [(C.c_int64 * n)(*c[k]) for k in ("ms", "ns", "a_offs", "b_offs")]
        d = LB.PlanDesc(alg=c["alg"], cells=c["cells"], match=c["match"], mismatch=c["mismatch"],
                        gap_open=c["gap_open"], gap_extend=c["gap_extend"], start_type=c["start_type"],
                        band=c["band"], track_end=c["track_end"], single=c["single"], n_pairs=n, m=arrs[0],
                        n=arrs[1], a_off=arrs[2], b_off=arrs[3])
        h = C.c_void_p()
        rec = dict(status=int(L.msa_plan_create(C.byref(d), C.byref(h))))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if rec["status"] != 0:
        return rec
    try:
        li = (C.c_int32 * 8)()
        LB.check(L.msa_plan_launch_info(h, li), "msa_plan_launch_info")
        rec["launch_info"] = [int(x) for x in li]
        e = C.c_int64()
        LB.check(L.msa_plan_cells_size(h, C.byref(e)), "msa_plan_cells_size")
        rec["cells_elems"] = int(e.value)
        rec["n_stripes"] = int(L.msa_plan_stripes(h))
        lay = (C.c_int64 * 4)()
        rec["layout"] = []
        for k in range(n):
            LB.check(L.msa_plan_pair_layout(h, k, lay), "msa_plan_pair_layout")
            rec["layout"].append([int(x) for x in lay])
        ri = (C.c_int32 * 4)()
        LB.check(L.msa_plan_run_info(h, ri, None), "msa_plan_run_info")
        rec["run_info_0_1_3"] = [int(ri[0]), int(ri[1]), int(ri[3])]
    finally:
        L.msa_plan_destroy(h)
    return rec


def main():
    set_ = [k for k in ONCE_PER_PROCESS if k in os.environ]
    if set_:
        sys.exit(f"unset {set_}: the recorded shapes are the defaults'")
    out = dict(device=device_facts(), cases={c["name"]: probe(c) for c in CASES})
    OUT.write_text(json.dumps(out, separators=(",", ":")) + "\n")
    for name, rec in out["cases"].items():
        print(name, rec["status"], rec.get("launch_info"), rec.get("run_info_0_1_3"))
    print("wrote", OUT, out["device"])


if __name__ == "__main__":
    main()
