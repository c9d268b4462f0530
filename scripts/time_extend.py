"""Time the extension plan's fill against the global (scored) plan's (MI355X; there is no fallback: without a GPU it
fails).

What the extension alignment's end-cell tracker costs.  An MSA_NW_EXTEND fill is an unbanded MSA_NW_SCORED fill --
the same cell, the same borders, the same direction bytes -- with, in every phase of every stripe, one compare and
two selects per step (the first maximum of the row's H), a wave reduction per stripe and one more mode of the pair
reduction.  The MSA_NW_SCORED plans are the baseline.  The same sequences (seeded; B is A with a tenth of its symbols
substituted, so the extensions are long) run under both algorithms:
  8 codes    4 symbols, +2 / -3 as an 8 x 8 table (msa_plan_create_scored),
  32 codes   24 symbols, +5 on the diagonal and -2 off it as a 32 x 32 table (msa_plan_create_scored32);
  gap_open 5, gap_extend 2;
  single_dir / single_none   one 4,096 x 4,096 pair, with direction bytes / the scores alone (single = 1),
  batch_dir / batch_none     256 pairs of 1,024 x 1,024 likewise (single = 0),
  batch_walk                 msa_plan_traceback_batch over the batch's bytes, both plans (HIP events around the launch).
Per shape both plans are created once and warmed up twice, then run alternately in one process; every run's fill time
is msa_plan_last_kernel_ms (HIP events around the DP launch), over as many runs as make each plan's summed kernel time
exceed 0.5 s (at least 20, at most 2,000).  Reported: median, min and max per plan, and the ratio of the medians,
extension over scored.  Prints one JSON line.

--tree PATH imports the package (and with it its built libmsa.so) from another checkout of the repository, say the
parent commit's, and --plans scored times the baseline alone, so the baseline can be taken from a build that has no
MSA_NW_EXTEND:

    python scripts/time_extend.py [--len1 4096] [--pairs 256] [--len 1024] [--plans both|scored] [--tree PATH]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

LB = Plan = None  # the package's _lib module and Plan class, imported by main() from the chosen tree

GAP_OPEN, GAP_EXTEND = 5, 2
MIN_MS, MIN_RUNS, MAX_RUNS = 500.0, 20, 2000
NW_EXTEND = 10  # (by value: --tree may point at a checkout whose Python side does not know it)


def table(codes: int) -> np.ndarray:
    """8 x 8: +2 / -3 over 4 symbols; 32 x 32: +5 / -2 over 24; 0 elsewhere."""
    k, match, mismatch = (4, 2, -3) if codes == 8 else (24, 5, -2)
    t = np.zeros((codes, codes), dtype=np.int8)
    t[:k, :k] = np.where(np.eye(k, dtype=bool), match, mismatch)
    return t


def sequences(codes: int, k: int, m: int, n: int):
    """k pairs of codes: A random over the scoring's symbols, B = A's first n symbols (cyclically) with a tenth
    substituted."""
    syms = 4 if codes == 8 else 24
    rng = np.random.default_rng(0x5EED0000 + codes)
    A = rng.integers(0, syms, size=(k, m), dtype=np.uint8)
    B = np.take(A, np.arange(n) % m, axis=1).copy()
    hit = rng.random((k, n)) < 0.1
    B[hit] = (B[hit] + 1 + rng.integers(0, syms - 1, size=int(hit.sum()), dtype=np.uint8)) % syms
    return A, B


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=len(v))


def measure(torch, dev, algs, codes, cells, k, m, n, single, walk=False):
    A, B = sequences(codes, k, m, n)
    dA, dB = torch.from_numpy(A.reshape(-1)).to(dev), torch.from_numpy(B.reshape(-1)).to(dev)
    a_offs, b_offs = [p * m for p in range(k)], [p * n for p in range(k)]
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
    if "extend" in algs:
        # the best pair of prefixes is at least as good as the whole pair, and its fin[] is the scored plan's result
        assert all(e["score"] >= max(s["score"], 0) and e["fin"][0] == s["score"]
                   for e, s in zip(res["extend"], res["scored"]))
    first = next(iter(algs))
    ms = {name: [] for name in algs}
    while len(ms[first]) < MAX_RUNS and (len(ms[first]) < MIN_RUNS or min(sum(v) for v in ms.values()) < MIN_MS):
        for name in algs:
            ms[name].append(run(name))
    assert all(plans[name].error() == 0 for name in algs)
    out = {f"{name}_ms": summary(ms[name]) for name in algs}
    if "extend" in algs:
        out["ratio_extend_over_scored"] = round(statistics.median(ms["extend"]) / statistics.median(ms["scored"]), 4)
    out["grid"] = {name: plans[name].launch_info()["grid"] for name in algs}
    out["lds_bytes"] = {name: plans[name].launch_info()["lds_bytes"] for name in algs}
    if walk:
        # the batch walk: every pair's walk in one launch, timed by events of its own; the extension's walks start at
        # the end cells, the scored plan's at (m, n)
        off = torch.tensor(Plan.ops_layout([m] * k, [n] * k), dtype=torch.int64, device=dev)
        ops = torch.empty(int(off[-1]), dtype=torch.uint8, device=dev)
        info = torch.empty(8 * k, dtype=torch.int64, device=dev)
        wms = {name: [] for name in algs}
        for rep in range(2 + 30):
            for name in algs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                plans[name].traceback_batch_async(outs[name], ops, off, info)
                e1.record()
                e1.synchronize()
                if rep >= 2:
                    wms[name].append(e0.elapsed_time(e1))
                assert int(info.view(-1, 8)[:, 3].abs().max()) == 0
        out["batch_walk"] = {f"{name}_ms": summary(wms[name]) for name in algs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--len1", type=int, default=4096, help="rows and columns of the single pair")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--len", type=int, default=1024, help="rows and columns of a batch pair")
    ap.add_argument("--plans", choices=["both", "scored"], default="both")
    ap.add_argument("--tree", default=None, help="another checkout of the repository, built")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_extend.py needs a GPU (there is no fallback)")
    global LB, Plan
    sys.path.insert(0, os.path.abspath(args.tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan
    algs = {"scored": LB.NW_SCORED}
    if args.plans == "both":
        algs["extend"] = NW_EXTEND
    dev = torch.device("cuda", 0)
    line = dict(script="time_extend", plans=args.plans, tree=args.tree, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND,
                single=[args.len1, args.len1], batch=[args.pairs, args.len, args.len],
                device=torch.cuda.get_device_name(0))
    for codes in (8, 32):
        line[f"codes{codes}"] = dict(
            single_dir=measure(torch, dev, algs, codes, LB.CELLS_DIR, 1, args.len1, args.len1, True),
            single_none=measure(torch, dev, algs, codes, LB.CELLS_NONE, 1, args.len1, args.len1, True),
            batch_dir=measure(torch, dev, algs, codes, LB.CELLS_DIR, args.pairs, args.len, args.len, False, walk=True),
            batch_none=measure(torch, dev, algs, codes, LB.CELLS_NONE, args.pairs, args.len, args.len, False))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
