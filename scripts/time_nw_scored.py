#!/usr/bin/env python
"""C3's pair (97,403 x 97,403, band 512) as a global alignment with direction bytes and the device walk, under
+2 / -3 scoring with g = 2, h = 3 (MSA_NW_SCORED) next to the +1 / 0 plan (MSA_NW_ALIGN, g = 1, h = 2): the fill's
kernel time (HIP events, Plan.kernel_ms()), the wall time of run() + synchronize and of the walk with its fetch,
medians of --runs runs after --warmup, and whether the chunks converged.  One JSON line per plan.

    python scripts/time_nw_scored.py [--runs 20] [--warmup 3]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cse305_parallel_sequence_alignment_amd import _lib as LB, data  # noqa: E402
from cse305_parallel_sequence_alignment_amd.plan import Plan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    A, B = data.c3_pair()
    tr = bytes.maketrans(b"ACGT", b"\x00\x01\x02\x03")
    dA = torch.from_numpy(np.frombuffer(A.translate(tr), dtype=np.uint8).copy()).to(dev)
    dB = torch.from_numpy(np.frombuffer(B.translate(tr), dtype=np.uint8).copy()).to(dev)
    sub = np.zeros((8, 8), dtype=np.int8)
    sub[:4, :4] = np.where(np.eye(4, dtype=bool), 2, -3)
    plans = {
        "NW_ALIGN +1/0 g=1 h=2": Plan(LB.NW_ALIGN, LB.CELLS_DIR, [len(A)], [len(B)], [0], [0], match=1, mismatch=0,
                                      gap_open=3, gap_extend=1, band=512),
        "NW_SCORED +2/-3 g=2 h=3": Plan(LB.NW_SCORED, LB.CELLS_DIR, [len(A)], [len(B)], [0], [0], sub=sub,
                                        gap_open=5, gap_extend=2, band=512),
    }
    for name, pl in plans.items():
        d = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
        fill, wall, walk = [], [], []
        for k in range(args.warmup + args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pl.run(dA, dB, d)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            tb = pl.traceback_nw(d)
            t2 = time.perf_counter()
            if k >= args.warmup:
                fill.append(pl.kernel_ms())
                wall.append((t1 - t0) * 1e3)
                walk.append((t2 - t1) * 1e3)
        res, info = pl.results()[0], pl.run_info()
        print(json.dumps(dict(plan=name, mode=pl.launch_info()["mode"], chunks=info["chunks"],
                              converged=info["converged"], score=res["score"], error=pl.error(),
                              fill_kernel_ms=dict(median=round(statistics.median(fill), 4), min=round(min(fill), 4),
                                                  max=round(max(fill), 4)),
                              run_wall_ms=round(statistics.median(wall), 4),
                              walk_fetch_wall_ms=round(statistics.median(walk), 4), ops=len(tb["ops"]),
                              cigar_head=tb["cigar"][:40])), flush=True)


if __name__ == "__main__":
    main()
