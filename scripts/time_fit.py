#!/usr/bin/env python
"""A batch of 256 pairs of 4,096 x 4,096 with direction bytes under +2 / -3 scoring, g = 2, h = 3, as a fit
alignment (MSA_NW_FIT) next to the global one (MSA_NW_SCORED) in one process: the fill's kernel time (HIP events,
Plan.kernel_ms()) and the device time of the one-launch batch walk (torch events around
Plan.traceback_batch_async), median and min-max of --runs runs after --warmup.  One JSON line per plan.

    python scripts/time_fit.py [--runs 20] [--warmup 3] [--pairs 256] [--size 4096] [--only scored|fit] [--cells dir|none]

--cells none times the score-only plans (no direction bytes, no walk).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cse305_parallel_sequence_alignment_amd import _lib as LB  # noqa: E402
from cse305_parallel_sequence_alignment_amd.plan import Plan  # noqa: E402


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--only", choices=["scored", "fit"], default=None)
    ap.add_argument("--cells", choices=["dir", "none"], default="dir")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    k, m = args.pairs, args.size
    rng = np.random.default_rng(7)
    # every reference a random sequence, every query a copy of it with 2% of the symbols redrawn
    Bc = rng.integers(0, 4, (k, m), dtype=np.uint8)
    Ac = Bc.copy()
    edit = rng.random((k, m)) < 0.02
    Ac[edit] = rng.integers(0, 4, int(edit.sum()), dtype=np.uint8)
    dA, dB = torch.from_numpy(Ac.reshape(-1)).to(dev), torch.from_numpy(Bc.reshape(-1)).to(dev)
    offs = [m * p for p in range(k)]
    sub = np.zeros((8, 8), dtype=np.int8)
    sub[:4, :4] = np.where(np.eye(4, dtype=bool), 2, -3)
    algs = {"scored": ("NW_SCORED", LB.NW_SCORED), "fit": ("NW_FIT", getattr(LB, "NW_FIT", None))}
    for key, (name, alg) in algs.items():
        if (args.only and args.only != key) or alg is None:
            continue
        if args.cells == "none":
            pl = Plan(alg, LB.CELLS_NONE, [m] * k, [m] * k, offs, offs, sub=sub, gap_open=5, gap_extend=2, band=-1)
            fill = []
            for r in range(args.warmup + args.runs):
                pl.run(dA, dB)
                torch.cuda.synchronize()
                if r >= args.warmup:
                    fill.append(pl.kernel_ms())
            res = pl.results()
            print(json.dumps(dict(plan=name, cells="none", lib=str(LB.LIB_PATH), mode=pl.launch_info()["mode"],
                                  pairs=k, size=m, score0=res[0]["score"], end0=list(res[0]["end"]),
                                  error=pl.error(), fill_kernel_ms=stats(fill))), flush=True)
            continue
        pl = Plan(alg, LB.CELLS_DIR, [m] * k, [m] * k, offs, offs, sub=sub, gap_open=5, gap_extend=2, band=-1)
        d = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
        off = Plan.ops_layout(pl.ms, pl.ns)
        ops = torch.empty(off[-1], dtype=torch.uint8, device=dev)
        info = torch.empty(8 * k, dtype=torch.int64, device=dev)
        d_off = torch.tensor(off, dtype=torch.int64, device=dev)
        fill, walk = [], []
        for r in range(args.warmup + args.runs):
            pl.run(dA, dB, d)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pl.traceback_batch_async(d, ops, d_off, info)
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                fill.append(pl.kernel_ms())
                walk.append(e0.elapsed_time(e1))
        res = pl.results()
        inf = info.cpu().numpy().reshape(-1, 8)
        print(json.dumps(dict(plan=name, lib=str(LB.LIB_PATH), mode=pl.launch_info()["mode"], pairs=k, size=m,
                              score0=res[0]["score"], end0=list(res[0]["end"]), error=pl.error(),
                              walk_status=int(np.abs(inf[:, 3]).max()), ops0=int(inf[0, 0]),
                              fill_kernel_ms=stats(fill), walk_batch_ms=stats(walk))), flush=True)
        del d, ops, pl


if __name__ == "__main__":
    main()
