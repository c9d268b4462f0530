#!/usr/bin/env python3
"""Diagnostic: where a main_alignment_function boundary call's time goes at 10k (steady state):
the whole call (msa_main_alignment), a plan create + destroy, and the device work (fill + walk)
of a resident plan; and the wall time of two more host entries, api.nw_align on a 4,096 x 4,096 pair
with band 64 and api.sw_align_batch on 256 pairs of 1,024.  Prints one JSON line: per workload
(minimum, median) in ms.

    time_boundary.py [L [REPS [WARMUP]]]      (10000, 10 timed calls after 1 warm-up call)

MSA_LIB_PATH names another build of the library (cse305_parallel_sequence_alignment_amd/_lib.py), so two
builds are compared by alternating runs of this script."""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from cse305_parallel_sequence_alignment_amd import _lib as LB, api, data
from cse305_parallel_sequence_alignment_amd.plan import Plan

L = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WARMUP = int(sys.argv[3]) if len(sys.argv) > 3 else 1
A, B = data.bundled()[0][:L], data.bundled()[1][:L]
m, n = len(A), len(B)


def best(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(min(ts) * 1e3, 4), round(sorted(ts)[len(ts) // 2] * 1e3, 4)


out = {}
out["boundary_call_ms"] = best(lambda: api.main_alignment_text(b"\0" + A, b"\0" + B, m, n, 32, 1.0, 2.0))


def mk():
    p = Plan(LB.REF_GOTOH, LB.CELLS_DIR, [m], [n], [0], [0], match=1, mismatch=0, gap_open=3, gap_extend=1,
             start_type=-1)
    p.close() if hasattr(p, "close") else None
    del p


out["plan_create_destroy_ms"] = best(mk)
pl = Plan(LB.REF_GOTOH, LB.CELLS_DIR, [m], [n], [0], [0], match=1, mismatch=0, gap_open=3, gap_extend=1,
          start_type=-1)
dA = torch.from_numpy(data.encode(A)).cuda()
dB = torch.from_numpy(data.encode(B)).cuda()
D = torch.empty(pl.cells_elems, dtype=torch.uint8, device="cuda")
ops = torch.empty(m + n + 2, dtype=torch.uint8, device="cuda")
info = torch.zeros(8, dtype=torch.int64, device="cuda")


def dev():
    pl.run(dA, dB, D)
    pl.traceback_gotoh_async(D, ops, info, -1)
    torch.cuda.synchronize()


out["device_fill_walk_ms"] = best(dev)


def dev_res():
    pl.run(dA, dB, D)
    pl.traceback_gotoh_async(D, ops, info, -1)
    pl.results()
    k = int(info[0].item())
    ops[:k].cpu()


out["device_fill_walk_results_ops_ms"] = best(dev_res)

# two more host entries: one banded global pair, one Smith-Waterman batch
nwA = data.synth(4096, 11)
nwB = (data.mutate(nwA, 12) + data.synth(64, 13))[:4096]
out["nw_align_4096_band64_ms"] = best(lambda: api.nw_align(nwA, nwB, band=64))
swA = [data.synth(1024, 100 + k) for k in range(256)]
swB = [(data.mutate(a, 400 + k) + data.synth(16, 700 + k))[:1024] for k, a in enumerate(swA)]
out["sw_align_batch_256x1024_ms"] = best(lambda: api.sw_align_batch(swA, swB, match=2, mismatch=-1, gap_open=3,
                                                                    gap_extend=1))
print(json.dumps(out), flush=True)
