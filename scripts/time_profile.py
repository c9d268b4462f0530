"""Time the fill kernel under a profile plan against its 32-code table twin (MI355X; there is no fallback: without a
GPU it fails).

What the profile's stripe prologue costs or saves: the same 4-symbol sequences (seeded, data.synth) run under a
32-code table plan (msa_plan_create_scored32: the row code is loaded, then the row's 32 bytes are read from the LDS copy
of the table) and under a profile plan (msa_plan_create_profile: each lane loads its row's 32 bytes from the plan's
profile) whose profile is api.profile_from_matrix of the same sequences and table (+2 / -3, gap_open 5, gap_extend 2),
so both plans compute the same cells.  For MSA_SW_SCORED, MSA_NW_SCORED and MSA_NW_FIT:
  single_dir   one 4,096 x 4,096 pair with direction bytes (single = 1),
  batch_dir    256 pairs of 1,024 x 1,024 with direction bytes (single = 0),
  batch_none   the same batch, scores only.
Per shape both plans are created once and warmed up, then run alternately in one process; every run's fill time is
msa_plan_last_kernel_ms (HIP events around the DP launch), over as many runs as make each plan's summed kernel time
exceed 0.5 s (at least 20, at most 2,000).  Reported: median, min and max per plan -- the table plan's own spread is
the yardstick of the ratio -- and the ratio of the medians.  Both plans must give the same scores and end cells, and
with direction bytes the same bytes.  Prints one JSON line.

    python scripts/time_profile.py [--len1 4096] [--pairs 256] [--len 1024]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cse305_parallel_sequence_alignment_amd import _lib as LB  # noqa: E402
from cse305_parallel_sequence_alignment_amd import api, data  # noqa: E402
from cse305_parallel_sequence_alignment_amd.plan import Plan  # noqa: E402

MATCH, MISMATCH, GAP_OPEN, GAP_EXTEND = 2, -3, 5, 2
MIN_MS, MIN_RUNS, MAX_RUNS = 500.0, 20, 2000
T4 = np.where(np.eye(4, dtype=bool), MATCH, MISMATCH).astype(np.int8)


def table32() -> np.ndarray:
    """32 x 32: the 4 x 4 match / mismatch scores in the corner, 0 elsewhere."""
    t = np.zeros((32, 32), dtype=np.int8)
    t[:4, :4] = T4
    return t


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=len(v))


def measure(torch, dev, alg, cells, k, m, n, single):
    As = [data.synth(m, 0x5EEDF000 + p) for p in range(k)]
    Bs = [data.synth(n, 0x5EEDF800 + p) for p in range(k)]
    dA = torch.from_numpy(data.encode(b"".join(As))).to(dev)
    dB = torch.from_numpy(data.encode(b"".join(Bs))).to(dev)
    prof = np.zeros((k * m, 32), dtype=np.int8)
    prof[:, :4] = api.profile_from_matrix(b"".join(As), b"ACGT", T4)
    a_offs, b_offs = [p * m for p in range(k)], [p * n for p in range(k)]
    kw = dict(gap_open=GAP_OPEN, gap_extend=GAP_EXTEND, single=single)
    plans = {"table": Plan(alg, cells, [m] * k, [n] * k, a_offs, b_offs, sub=table32(), **kw),
             "profile": Plan(alg, cells, [m] * k, [n] * k, a_offs, b_offs, profile=prof, **kw)}
    outs = {}
    for name, pl in plans.items():
        assert pl.format_info()["codes"] == 32 and pl.launch_info()["mode"] == "stripe"
        assert pl.format_info()["profile"] == (name == "profile")
        outs[name] = torch.zeros(max(pl.cells_elems, 1), dtype=torch.uint8, device=dev) \
            if cells == LB.CELLS_DIR else None

    def run(name):
        plans[name].run(None if name == "profile" else dA, dB, outs[name])
        return plans[name].kernel_ms()  # (synchronizes on the run's events)

    for name in plans:  # warm-up of both launch shapes
        run(name)
        run(name)
    res = {name: pl.results() for name, pl in plans.items()}  # (raises on a sticky plan error)
    assert [r["score"] for r in res["table"]] == [r["score"] for r in res["profile"]], "the two plans' scores differ"
    assert [r["end"] for r in res["table"]] == [r["end"] for r in res["profile"]]
    if cells == LB.CELLS_DIR:
        assert plans["table"].cells_elems == plans["profile"].cells_elems
        assert torch.equal(outs["table"], outs["profile"]), "the bytes differ"
    ms = {"table": [], "profile": []}
    while len(ms["table"]) < MAX_RUNS and (len(ms["table"]) < MIN_RUNS or
                                           min(sum(ms["table"]), sum(ms["profile"])) < MIN_MS):
        for name in plans:
            ms[name].append(run(name))
    assert plans["table"].error() == 0 and plans["profile"].error() == 0
    tmed = statistics.median(ms["table"])
    return dict(table_ms=summary(ms["table"]), profile_ms=summary(ms["profile"]),
                ratio_profile_over_table=round(statistics.median(ms["profile"]) / tmed, 4),
                table_spread=[round(min(ms["table"]) / tmed, 4), round(max(ms["table"]) / tmed, 4)],
                lds_bytes={name: pl.launch_info()["lds_bytes"] for name, pl in plans.items()},
                grid={name: pl.launch_info()["grid"] for name, pl in plans.items()},
                tracking=plans["profile"].format_info()["tracking"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--len1", type=int, default=4096, help="rows and columns of the single pair")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--len", type=int, default=1024, help="rows and columns of a batch pair")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_profile.py needs a GPU (there is no fallback)")
    dev = torch.device("cuda", 0)
    line = dict(script="time_profile", scoring=dict(match=MATCH, mismatch=MISMATCH, gap_open=GAP_OPEN,
                                                    gap_extend=GAP_EXTEND),
                single=[args.len1, args.len1], batch=[args.pairs, args.len, args.len],
                device=torch.cuda.get_device_name(0))
    for name, alg in (("SW_SCORED", LB.SW_SCORED), ("NW_SCORED", LB.NW_SCORED), ("NW_FIT", LB.NW_FIT)):
        line[name] = dict(
            single_dir=measure(torch, dev, alg, LB.CELLS_DIR, 1, args.len1, args.len1, True),
            batch_dir=measure(torch, dev, alg, LB.CELLS_DIR, args.pairs, args.len, args.len, False),
            batch_none=measure(torch, dev, alg, LB.CELLS_NONE, args.pairs, args.len, args.len, False))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
