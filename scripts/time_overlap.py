"""Time the overlap plan's fill against the fit plan's (MI355X; there is no fallback: without a GPU it fails).

What the overlap alignment's last-column search costs.  An MSA_NW_OVERLAP fill is an MSA_NW_FIT fill -- the same
cell, the same zero top border, the same row-m maximum in the stripe of row m -- with a zero left border and, in the
masked head and tail phases of EVERY stripe, the capture of H at column n, plus a wave reduction per stripe.  The fit
plans are the baseline.  The same 4-symbol sequences (seeded, data.synth; +2 / -3, gap_open 5, gap_extend 2) run
under both algorithms, at 8 codes (msa_plan_create_scored) and at 32 (msa_plan_create_scored32, the 4 x 4 scores
embedded in the 32 x 32 table):
  single_dir / single_none   one 4,096 x 4,096 pair, with direction bytes / the score alone (single = 1),
  batch_dir / batch_none     256 pairs of 1,024 x 1,024 likewise (single = 0).
Per shape both plans are created once and warmed up, then run alternately in one process; every run's fill time is
msa_plan_last_kernel_ms (HIP events around the DP launch), over as many runs as make each plan's summed kernel time
exceed 0.5 s (at least 20, at most 2,000).  Reported: median, min and max per plan, and the ratio of the medians,
overlap over fit.  Prints one JSON line.

    python scripts/time_overlap.py [--len1 4096] [--pairs 256] [--len 1024]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cse305_parallel_sequence_alignment_amd import _lib as LB  # noqa: E402
from cse305_parallel_sequence_alignment_amd import data  # noqa: E402
from cse305_parallel_sequence_alignment_amd.plan import Plan  # noqa: E402

MATCH, MISMATCH, GAP_OPEN, GAP_EXTEND = 2, -3, 5, 2
MIN_MS, MIN_RUNS, MAX_RUNS = 500.0, 20, 2000


def table(k: int) -> np.ndarray:
    """k x k: the 4 x 4 match / mismatch scores in the corner, 0 elsewhere."""
    t = np.zeros((k, k), dtype=np.int8)
    t[:4, :4] = np.where(np.eye(4, dtype=bool), MATCH, MISMATCH)
    return t


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=len(v))


def measure(torch, dev, codes, cells, k, m, n, single):
    As = [data.synth(m, 0x5EEDF000 + p) for p in range(k)]
    Bs = [data.synth(n, 0x5EEDF800 + p) for p in range(k)]
    dA = torch.from_numpy(data.encode(b"".join(As))).to(dev)
    dB = torch.from_numpy(data.encode(b"".join(Bs))).to(dev)
    a_offs, b_offs = [p * m for p in range(k)], [p * n for p in range(k)]
    algs = {"fit": LB.NW_FIT, "overlap": LB.NW_OVERLAP}
    plans, outs = {}, {}
    for name, alg in algs.items():
        plans[name] = Plan(alg, cells, [m] * k, [n] * k, a_offs, b_offs, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND,
                           single=single, sub=table(codes))
        assert plans[name].format_info()["codes"] == codes and plans[name].launch_info()["mode"] == "stripe"
        outs[name] = torch.zeros(max(plans[name].cells_elems, 1), dtype=torch.uint8, device=dev) \
            if cells == LB.CELLS_DIR else None

    def run(name):
        plans[name].run(dA, dB, outs[name])
        return plans[name].kernel_ms()  # (synchronizes on the run's events)

    for name in algs:  # warm-up of both kernels
        run(name)
        run(name)
    res = {name: plans[name].results() for name in algs}  # (raises on a sticky plan error)
    # H under two zero borders is >= H under one, cell by cell, and the overlap's candidates include the fit's
    assert all(o["score"] >= max(f["score"], 0) for o, f in zip(res["overlap"], res["fit"]))
    ms = {name: [] for name in algs}
    while len(ms["fit"]) < MAX_RUNS and (len(ms["fit"]) < MIN_RUNS or min(sum(ms["fit"]), sum(ms["overlap"])) < MIN_MS):
        for name in algs:
            ms[name].append(run(name))
    assert plans["fit"].error() == 0 and plans["overlap"].error() == 0
    return dict(fit_ms=summary(ms["fit"]), overlap_ms=summary(ms["overlap"]),
                ratio_overlap_over_fit=round(statistics.median(ms["overlap"]) / statistics.median(ms["fit"]), 4),
                grid={name: plans[name].launch_info()["grid"] for name in algs},
                lds_bytes={name: plans[name].launch_info()["lds_bytes"] for name in algs})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--len1", type=int, default=4096, help="rows and columns of the single pair")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--len", type=int, default=1024, help="rows and columns of a batch pair")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_overlap.py needs a GPU (there is no fallback)")
    dev = torch.device("cuda", 0)
    line = dict(script="time_overlap", scoring=dict(match=MATCH, mismatch=MISMATCH, gap_open=GAP_OPEN,
                                                    gap_extend=GAP_EXTEND),
                single=[args.len1, args.len1], batch=[args.pairs, args.len, args.len],
                device=torch.cuda.get_device_name(0))
    for codes in (8, 32):
        line[f"codes{codes}"] = dict(
            single_dir=measure(torch, dev, codes, LB.CELLS_DIR, 1, args.len1, args.len1, True),
            single_none=measure(torch, dev, codes, LB.CELLS_NONE, 1, args.len1, args.len1, True),
            batch_dir=measure(torch, dev, codes, LB.CELLS_DIR, args.pairs, args.len, args.len, False),
            batch_none=measure(torch, dev, codes, LB.CELLS_NONE, args.pairs, args.len, args.len, False))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
