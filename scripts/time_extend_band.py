"""Time the banded extension plan's fill against its two neighbours (MI355X; there is no fallback: without a GPU it
fails).

Three plans per shape, on the same sequences (seeded; B is A with a tenth of its symbols substituted, so the extensions
are long and stay near the diagonal):
  (a) banded    MSA_NW_EXTEND_BAND with band w,
  (b) scored    a banded MSA_NW_SCORED plan on the stripe launch with the same band: the same cells, edge phases and
                bytes without the end-cell tracker -- a / b is what the tracker costs inside a band,
  (c) unbanded  MSA_NW_EXTEND: every cell -- a / c is what the band saves.
Shapes: one 4,096 x 4,096 pair (single = 1) and 256 pairs of 2,048 x 2,048 (single = 0); bands 64 and 256; 8 codes
(4 symbols as an 8 x 8 table) and 32 codes (24 symbols as a 32 x 32 table); with direction bytes and the scores alone;
gap_open 5, gap_extend 2.  Scores: +2 / -3 (8 codes), +5 / -2 (32 codes) -- but +121 / -3 for the 8-code single pair,
whose banded MSA_NW_SCORED plan would otherwise run the band kernel (choose_mode: a table whose largest entry plus
the gap costs passes 127 keeps the exact stripe launch); fill time does not depend on the scores.
Per shape the plans are created once and warmed up twice, then run alternately in one process; every run's fill time
is msa_plan_last_kernel_ms (HIP events around the DP launch); a plan leaves the rotation once it has at least 20 runs
and 0.5 s of summed kernel time (at most 2,000 runs).  Reported: median, min and max per plan and the two ratios of
medians.  Prints one JSON line.

--tree PATH imports the package (and with it its built libmsa.so) from another checkout of the repository, say the
parent commit's, and --plans parent times (b) and (c) alone, which a build without MSA_NW_EXTEND_BAND has:

    python scripts/time_extend_band.py [--len1 4096] [--pairs 256] [--len 2048] [--bands 64,256]
                                       [--plans all|parent] [--tree PATH]
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
NW_EXTEND, NW_EXTEND_BAND = 10, 11  # (by value: --tree may point at a checkout whose Python side does not know them)


def table(codes: int, single: bool) -> np.ndarray:
    """8 x 8: +2 / -3 over 4 symbols (+121 / -3 for a single pair: see the module docstring); 32 x 32: +5 / -2 over
    24; 0 elsewhere."""
    k, match, mismatch = (4, 121 if single else 2, -3) if codes == 8 else (24, 5, -2)
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


def measure(torch, dev, names, codes, cells, k, m, n, single, band):
    A, B = sequences(codes, k, m, n)
    dA, dB = torch.from_numpy(A.reshape(-1)).to(dev), torch.from_numpy(B.reshape(-1)).to(dev)
    a_offs, b_offs = [p * m for p in range(k)], [p * n for p in range(k)]
    kinds = {"banded": (NW_EXTEND_BAND, band), "scored": (LB.NW_SCORED, band), "unbanded": (NW_EXTEND, -1)}
    plans, outs = {}, {}
    for name in names:
        alg, w = kinds[name]
        plans[name] = Plan(alg, cells, [m] * k, [n] * k, a_offs, b_offs, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND,
                           band=w, single=single, sub=table(codes, single))
        assert plans[name].format_info()["codes"] == codes and plans[name].launch_info()["mode"] == "stripe", name
        outs[name] = torch.zeros(max(plans[name].cells_elems, 1), dtype=torch.uint8, device=dev) \
            if cells == LB.CELLS_DIR else None

    def run(name):
        plans[name].run(dA, dB, outs[name])
        return plans[name].kernel_ms()  # (synchronizes on the run's events)

    for name in names:  # warm-up of every kernel
        run(name)
        run(name)
    res = {name: plans[name].results() for name in names}  # (raises on a sticky plan error)
    if "banded" in names:
        # the banded extension's fin[] is the banded scored plan's result; the best in-band pair of prefixes is at least
        # as good as the whole pair and no better than the unbanded extension's
        assert all(e["fin"][0] == s["score"] and max(s["score"], 0) <= e["score"] <= u["score"]
                   for e, s, u in zip(res["banded"], res["scored"], res["unbanded"]))
    ms = {name: [] for name in names}

    def done(name):
        return len(ms[name]) >= MAX_RUNS or (len(ms[name]) >= MIN_RUNS and sum(ms[name]) >= MIN_MS)

    while not all(done(name) for name in names):
        for name in names:
            if not done(name):
                ms[name].append(run(name))
    assert all(plans[name].error() == 0 for name in names)
    out = {f"{name}_ms": summary(ms[name]) for name in names}
    med = {name: statistics.median(ms[name]) for name in names}
    if "banded" in names:
        out["ratio_banded_over_scored"] = round(med["banded"] / med["scored"], 4)
        out["ratio_banded_over_unbanded"] = round(med["banded"] / med["unbanded"], 4)
    out["grid"] = {name: plans[name].launch_info()["grid"] for name in names}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--len1", type=int, default=4096, help="rows and columns of the single pair")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--len", type=int, default=2048, help="rows and columns of a batch pair")
    ap.add_argument("--bands", default="64,256")
    ap.add_argument("--plans", choices=["all", "parent"], default="all")
    ap.add_argument("--tree", default=None, help="another checkout of the repository, built")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_extend_band.py needs a GPU (there is no fallback)")
    global LB, Plan
    sys.path.insert(0, os.path.abspath(args.tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan
    names = ["banded", "scored", "unbanded"] if args.plans == "all" else ["scored", "unbanded"]
    dev = torch.device("cuda", 0)
    line = dict(script="time_extend_band", plans=args.plans, tree=args.tree, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND,
                single=[args.len1, args.len1], batch=[args.pairs, args.len, args.len],
                device=torch.cuda.get_device_name(0))
    for codes in (8, 32):
        for band in (int(b) for b in args.bands.split(",")):
            line[f"codes{codes}_band{band}"] = dict(
                single_dir=measure(torch, dev, names, codes, LB.CELLS_DIR, 1, args.len1, args.len1, True, band),
                single_none=measure(torch, dev, names, codes, LB.CELLS_NONE, 1, args.len1, args.len1, True, band),
                batch_dir=measure(torch, dev, names, codes, LB.CELLS_DIR, args.pairs, args.len, args.len, False, band),
                batch_none=measure(torch, dev, names, codes, LB.CELLS_NONE, args.pairs, args.len, args.len, False,
                                   band))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
