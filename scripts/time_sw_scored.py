"""Time the fill kernel of local alignment under a substitution table (MI355X; there is no fallback: without a GPU it
fails).

The same 4-symbol sequences (seeded, data.synth) under +2 / -3, gap_open 5, gap_extend 2 run as three plans:
  affine    MSA_SW_AFFINE with track_end (match / mismatch in the kernel parameters),
  scored8   MSA_SW_SCORED over 8 codes, the 4 x 4 scores in the corner of its 8 x 8 table,
  scored32  MSA_SW_SCORED over 32 codes, the same corner of a 32 x 32 table,
on one single-pair shape and one batch shape, with direction bytes and without:
  single_dir / single_none   one 4,096 x 4,096 pair (single = 1),
  batch_dir / batch_none     512 pairs of 1,024 x 1,024 (single = 0).
The scored plans always launch the stripe kernel.  The affine plan launches it where the planner lets it: a
single pair with direction bytes takes the flow kernels, and a batch of fewer pairs than two per compute unit with
equal row counts takes the split launch; the mode each plan reports is in the output, and only "stripe" against
"stripe" compares the same kernel.  Per shape the plans are created once and warmed up, then run in turn (affine,
scored8, scored32, affine, ...) in one process; every run's fill time is msa_plan_last_kernel_ms (HIP events around the
DP launch), over as many rounds as make each plan's summed kernel time exceed 0.5 s (at least 20, at most 2,000).
Reported: median, min and max per plan and the ratios of the medians.  The three plans must give the same scores and
end cells, and the stripe-kernel plans the same direction bytes.  Prints one JSON line.

    python scripts/time_sw_scored.py [--len1 4096] [--pairs 512] [--len 1024]
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
NAMES = ("affine", "scored8", "scored32")


def table(k: int) -> np.ndarray:
    """k x k: the 4 x 4 match / mismatch scores in the corner, 0 elsewhere."""
    t = np.zeros((k, k), dtype=np.int8)
    t[:4, :4] = np.where(np.eye(4, dtype=bool), MATCH, MISMATCH)
    return t


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=len(v))


def measure(torch, dev, cells, k, m, n, single):
    As = [data.synth(m, 0x5EED5000 + p) for p in range(k)]
    Bs = [data.synth(n, 0x5EED5800 + p) for p in range(k)]
    dA = torch.from_numpy(data.encode(b"".join(As))).to(dev)
    dB = torch.from_numpy(data.encode(b"".join(Bs))).to(dev)
    shape = ([m] * k, [n] * k, [p * m for p in range(k)], [p * n for p in range(k)])
    gaps = dict(gap_open=GAP_OPEN, gap_extend=GAP_EXTEND, single=single)
    plans = dict(affine=Plan(LB.SW_AFFINE, cells, *shape, match=MATCH, mismatch=MISMATCH, track_end=True, **gaps),
                 scored8=Plan(LB.SW_SCORED, cells, *shape, sub=table(8), **gaps),
                 scored32=Plan(LB.SW_SCORED, cells, *shape, sub=table(32), **gaps))
    mode = {x: plans[x].launch_info()["mode"] for x in NAMES}
    assert mode["scored8"] == mode["scored32"] == "stripe"
    assert plans["scored8"].format_info()["codes"] == 8 and plans["scored32"].format_info()["codes"] == 32
    outs = {x: torch.zeros(max(plans[x].cells_elems, 1), dtype=torch.uint8, device=dev) if cells == LB.CELLS_DIR
            else None for x in NAMES}

    def run(x):
        plans[x].run(dA, dB, outs[x])
        return plans[x].kernel_ms()  # (synchronizes on the run's events)

    for x in NAMES:  # warm-up of every launch shape
        run(x)
        run(x)
    res = {x: plans[x].results() for x in NAMES}  # (raises on a sticky plan error)
    for x in NAMES[1:]:
        assert [(r["score"], r["end"]) for r in res[x]] == [(r["score"], r["end"]) for r in res["affine"]], x
    if cells == LB.CELLS_DIR:
        same = [x for x in NAMES if mode[x] == "stripe"]
        for x in same[1:]:
            assert plans[x].cells_elems == plans[same[0]].cells_elems and torch.equal(outs[x], outs[same[0]]), x
    ms = {x: [] for x in NAMES}
    while len(ms["affine"]) < MAX_RUNS and (len(ms["affine"]) < MIN_RUNS or min(sum(v) for v in ms.values()) < MIN_MS):
        for x in NAMES:
            ms[x].append(run(x))
    assert all(plans[x].error() == 0 for x in NAMES)
    med = {x: statistics.median(ms[x]) for x in NAMES}
    return dict(ms={x: summary(ms[x]) for x in NAMES}, mode=mode, order=list(NAMES),
                tracking={x: plans[x].format_info()["tracking"] for x in NAMES},
                scored8_over_affine=round(med["scored8"] / med["affine"], 4),
                scored32_over_scored8=round(med["scored32"] / med["scored8"], 4),
                lds_bytes={x: plans[x].launch_info()["lds_bytes"] for x in NAMES},
                grid={x: plans[x].launch_info()["grid"] for x in NAMES})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--len1", type=int, default=4096, help="rows and columns of the single pair")
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--len", type=int, default=1024, help="rows and columns of a batch pair")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_sw_scored.py needs a GPU (there is no fallback)")
    dev = torch.device("cuda", 0)
    line = dict(script="time_sw_scored", scoring=dict(match=MATCH, mismatch=MISMATCH, gap_open=GAP_OPEN,
                                                      gap_extend=GAP_EXTEND),
                single=[args.len1, args.len1], batch=[args.pairs, args.len, args.len],
                device=torch.cuda.get_device_name(0),
                single_dir=measure(torch, dev, LB.CELLS_DIR, 1, args.len1, args.len1, True),
                single_none=measure(torch, dev, LB.CELLS_NONE, 1, args.len1, args.len1, True),
                batch_dir=measure(torch, dev, LB.CELLS_DIR, args.pairs, args.len, args.len, False),
                batch_none=measure(torch, dev, LB.CELLS_NONE, args.pairs, args.len, args.len, False))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
