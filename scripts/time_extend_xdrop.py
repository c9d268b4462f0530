"""Time the X-drop extension's fill (msa_xdrop.hip, one wave per pair) against the banded extension plan's (the stripe
kernel) on the same inputs (MI355X; there is no fallback: without a GPU it fails).

Shape: a batch of 256 pairs of 2,048 x 2,048, bands 64 and 256, 4 symbols, +2 / -3, gap_open 5, gap_extend 2, with
direction bytes.  Two workloads (seeded):
  (a) similar   B is A with a tenth of its symbols substituted: no pair ever stops.  X-drop with xdrop = -1 and 100.
  (b) flanks    a 200-symbol common prefix, then unrelated tails: every pair stops early.  xdrop = 50.
Per workload and band, in one process and alternately after two warm-up runs each:
  banded   an MSA_NW_EXTEND_BAND batch plan's fill, msa_plan_last_kernel_ms (HIP events around the DP launch) -- what
           msa_extend_align_batch_banded runs, here and on the parent commit (this kernel family touches no other);
  xdrop    msa_xdrop_extend_run between two events on the same stream.
A variant leaves the rotation once it has at least 20 runs and 0.5 s of summed kernel time (at most 2,000 runs).
Reported: median, min and max per variant, the ratio of medians xdrop / banded, and per pair the mean D and the mean
number of cells computed (in-band interior cells with i + j <= D) beside the band's total.  The end-to-end host calls
(api.extend_align_batch with band, with and without xdrop: uploads, walks and CIGARs included) are timed too, five
calls each after one warm-up, median wall-clock.  Prints one JSON line.

    python scripts/time_extend_xdrop.py [--pairs 256] [--len 2048] [--bands 64,256]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

GAP_OPEN, GAP_EXTEND, MATCH, MISMATCH = 5, 2, 2, -3
MIN_MS, MIN_RUNS, MAX_RUNS = 500.0, 20, 2000
NW_EXTEND_BAND = 11


def similar(k, m):
    rng = np.random.default_rng(0x5EED0008)
    A = rng.integers(0, 4, size=(k, m), dtype=np.uint8)
    B = A.copy()
    hit = rng.random((k, m)) < 0.1
    B[hit] = (B[hit] + 1 + rng.integers(0, 3, size=int(hit.sum()), dtype=np.uint8)) % 4
    return A, B


def flanks(k, m, prefix=200):
    rng = np.random.default_rng(0x5EED0009)
    A = rng.integers(0, 4, size=(k, m), dtype=np.uint8)
    B = rng.integers(0, 4, size=(k, m), dtype=np.uint8)
    B[:, :prefix] = A[:, :prefix]
    return A, B


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=len(v))


def measure(torch, LB, Plan, dev, A, B, band, xdrops):
    k, m = A.shape
    dA, dB = torch.from_numpy(A.reshape(-1)).to(dev), torch.from_numpy(B.reshape(-1)).to(dev)
    offs = np.arange(k, dtype=np.int64) * m
    sub = np.zeros((8, 8), dtype=np.int8)
    sub[:4, :4] = np.where(np.eye(4, dtype=bool), MATCH, MISMATCH)
    plan = Plan(NW_EXTEND_BAND, LB.CELLS_DIR, [m] * k, [m] * k, list(offs), list(offs), gap_open=GAP_OPEN,
                gap_extend=GAP_EXTEND, band=band, single=False, sub=sub)
    pdir = torch.zeros(plan.cells_elems, dtype=torch.uint8, device=dev)
    sizes = torch.full((k,), m, dtype=torch.int64, device=dev)
    doffs = torch.from_numpy(offs).to(dev)
    dir_off = torch.arange(k + 1, dtype=torch.int64, device=dev) * ((2 * band + 1) * (m + 1))
    xdir = torch.zeros((2 * band + 1) * (m + 1) * k, dtype=torch.uint8, device=dev)
    res = torch.zeros(8 * k, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def run(name):
        if name == "banded":
            plan.run(dA, dB, pdir)
            return plan.kernel_ms()
        e0.record(st)
        LB.check(LB.lib().msa_xdrop_extend_run(p(dA), p(dB), k, p(sizes), p(sizes), p(doffs), p(doffs), None, MATCH,
                                               MISMATCH, GAP_OPEN, GAP_EXTEND, band, name, p(xdir), p(dir_off), p(res),
                                               C.c_void_p(st.cuda_stream)), "msa_xdrop_extend_run")
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    names = ["banded"] + list(xdrops)
    out = {}
    banded = plan_res = None
    for name in names:  # warm-up, and what each variant computed
        run(name)
        run(name)
        if name == "banded":
            plan_res = plan.results()
            banded = [r["score"] for r in plan_res]
        else:
            r = res.cpu().numpy().reshape(k, 8)
            assert (r[:, 5] == 0).all()
            full = r[:, 3] == 2 * m
            # a pair that never stopped has the banded extension's score
            assert all(int(r[q, 0]) == banded[q] for q in range(k) if full[q])
            out[f"xdrop{name}"] = dict(mean_D=float(r[:, 3].mean()), mean_cells=float(r[:, 6].mean()),
                                       dropped=int((~full).sum()))
    band_cells = sum(min(m, i + band) - max(1, i - band) + 1 for i in range(1, m + 1))
    ms = {name: [] for name in names}

    def done(name):
        return len(ms[name]) >= MAX_RUNS or (len(ms[name]) >= MIN_RUNS and sum(ms[name]) >= MIN_MS)

    while not all(done(name) for name in names):
        for name in names:
            if not done(name):
                ms[name].append(run(name))
    assert plan.error() == 0
    out["band_cells"] = band_cells
    out["banded_ms"] = summary(ms["banded"])
    for x in xdrops:
        out[f"xdrop{x}"]["ms"] = summary(ms[x])
        out[f"xdrop{x}"]["ratio_over_banded"] = round(statistics.median(ms[x]) / statistics.median(ms["banded"]), 4)
    return out


def host_calls(api, A, B, band, xdrops):
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    As, Bs = [lut[a].tobytes() for a in A], [lut[b].tobytes() for b in B]
    kw = dict(match=MATCH, mismatch=MISMATCH, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND, band=band)
    out = {}
    for x in [None] + list(xdrops):
        t = []
        for rep in range(6):
            t0 = time.perf_counter()
            api.extend_align_batch(As, Bs, xdrop=x, **kw)
            t.append(1e3 * (time.perf_counter() - t0))
        out["banded_ms" if x is None else f"xdrop{x}_ms"] = summary(t[1:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--len", type=int, default=2048)
    ap.add_argument("--bands", default="64,256")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_extend_xdrop.py needs a GPU (there is no fallback)")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd import api
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    dev = torch.device("cuda", 0)
    line = dict(script="time_extend_xdrop", batch=[args.pairs, args.len, args.len], gap_open=GAP_OPEN,
                gap_extend=GAP_EXTEND, device=torch.cuda.get_device_name(0))
    for band in (int(b) for b in args.bands.split(",")):
        for name, (A, B), xdrops in (("similar", similar(args.pairs, args.len), (-1, 100)),
                                     ("flanks", flanks(args.pairs, args.len), (50,))):
            line[f"{name}_band{band}"] = dict(fill=measure(torch, LB, Plan, dev, A, B, band, xdrops),
                                              host=host_calls(api, A, B, band, xdrops))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
