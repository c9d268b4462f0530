"""Time the fill kernel under 8-code and 32-code plans (MI355X; there is no fallback: without a GPU it fails).

What the wider score lookup costs: the same 4-symbol sequences (seeded, data.synth) run under an 8-code plan
(msa_plan_create_scored, one v_perm_b32 per four cells) and under a 32-code plan (msa_plan_create_scored32, seven)
whose 32 x 32 table embeds the same 4 x 4 scores (+2 / -3, gap_open 5, gap_extend 2), for MSA_NW_SCORED and MSA_NW_FIT:
  single_dir   one 4,096 x 4,096 pair with direction bytes (single = 1),
  batch_dir    256 pairs of 1,024 x 1,024 with direction bytes (single = 0),
  batch_none   the same batch, scores only.
Per shape both plans are created once and warmed up, then run alternately in one process; every run's fill time is
msa_plan_last_kernel_ms (HIP events around the DP launch), over as many runs as make each plan's summed kernel time
exceed 0.5 s (at least 20, at most 2,000).  Reported: median, min and max per plan, and the ratio of the medians.
Both plans must give the same scores, and with direction bytes the same bytes.  Prints one JSON line.

    python scripts/time_wide_alphabet.py [--len1 4096] [--pairs 256] [--len 1024]
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


def measure(torch, dev, alg, cells, k, m, n, single):
    As = [data.synth(m, 0x5EEDF000 + p) for p in range(k)]
    Bs = [data.synth(n, 0x5EEDF800 + p) for p in range(k)]
    dA = torch.from_numpy(data.encode(b"".join(As))).to(dev)
    dB = torch.from_numpy(data.encode(b"".join(Bs))).to(dev)
    a_offs, b_offs = [p * m for p in range(k)], [p * n for p in range(k)]
    plans, outs = {}, {}
    for codes in (8, 32):
        plans[codes] = Plan(alg, cells, [m] * k, [n] * k, a_offs, b_offs, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND,
                            single=single, sub=table(codes))
        assert plans[codes].format_info()["codes"] == codes and plans[codes].launch_info()["mode"] == "stripe"
        outs[codes] = torch.zeros(max(plans[codes].cells_elems, 1), dtype=torch.uint8, device=dev) \
            if cells == LB.CELLS_DIR else None

    def run(codes):
        plans[codes].run(dA, dB, outs[codes])
        return plans[codes].kernel_ms()  # (synchronizes on the run's events)

    for codes in (8, 32):  # warm-up of both launch shapes
        run(codes)
        run(codes)
    res = {c: plans[c].results() for c in (8, 32)}  # (raises on a sticky plan error)
    assert [r["score"] for r in res[8]] == [r["score"] for r in res[32]], "the two plans' scores differ"
    assert [r["end"] for r in res[8]] == [r["end"] for r in res[32]]
    if cells == LB.CELLS_DIR:
        assert plans[8].cells_elems == plans[32].cells_elems and torch.equal(outs[8], outs[32]), "the bytes differ"
    ms = {8: [], 32: []}
    while len(ms[8]) < MAX_RUNS and (len(ms[8]) < MIN_RUNS or min(sum(ms[8]), sum(ms[32])) < MIN_MS):
        for codes in (8, 32):
            ms[codes].append(run(codes))
    assert plans[8].error() == 0 and plans[32].error() == 0
    return dict(codes8_ms=summary(ms[8]), codes32_ms=summary(ms[32]),
                ratio_32_over_8=round(statistics.median(ms[32]) / statistics.median(ms[8]), 4),
                lds_bytes={c: plans[c].launch_info()["lds_bytes"] for c in (8, 32)},
                grid={c: plans[c].launch_info()["grid"] for c in (8, 32)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--len1", type=int, default=4096, help="rows and columns of the single pair")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--len", type=int, default=1024, help="rows and columns of a batch pair")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_wide_alphabet.py needs a GPU (there is no fallback)")
    dev = torch.device("cuda", 0)
    line = dict(script="time_wide_alphabet", scoring=dict(match=MATCH, mismatch=MISMATCH, gap_open=GAP_OPEN,
                                                          gap_extend=GAP_EXTEND),
                single=[args.len1, args.len1], batch=[args.pairs, args.len, args.len],
                device=torch.cuda.get_device_name(0))
    for name, alg in (("NW_SCORED", LB.NW_SCORED), ("NW_FIT", LB.NW_FIT)):
        line[name] = dict(
            single_dir=measure(torch, dev, alg, LB.CELLS_DIR, 1, args.len1, args.len1, True),
            batch_dir=measure(torch, dev, alg, LB.CELLS_DIR, args.pairs, args.len, args.len, False),
            batch_none=measure(torch, dev, alg, LB.CELLS_NONE, args.pairs, args.len, args.len, False))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
