"""Time seed chaining (MI355X; there is no fallback: without a GPU it fails): the chain kernel alone, through
msa_chain_run on device arrays between two stream events, and beside it one api.chain_seeds_batch call end to end
(the sort, the uploads, the kernel, the downloads, the chain extraction on the host and the result dictionaries).

Shapes: 1,024 problems of 2,000 anchors (one wave each, four per workgroup: 256 workgroups, one round of the device) and
64 problems of 20,000 anchors (16 workgroups: the latency of one wave, undisturbed), at lookback 64, 256 and 1,024.
Anchors (seeded): 15-mers advancing 1-8 symbols each along B, nine in ten on the main diagonal with a jitter of up to 3,
the others on one of eight diagonals 500 apart; band 50, max_dist 5,000, match 1, gap_open 3, gap_extend 1 -- so most
anchors have admissible predecessors throughout their window and no chunk of it is cut short by max_dist.
Per shape and lookback: three warm-up launches, then `--reps` timed ones, each between its own pair of events; reported
are the median, min and max in ms and ns_per_anchor = median / anchors per problem -- every problem is one wave's
dependent chain and the waves run side by side, so this is the latency of one anchor, not a throughput.  The results
are checked once against the host entry's f and pred.  The end-to-end call: one warm-up, `--calls` timed, wall clock.
Prints one JSON line.

    python scripts/time_chain.py [--reps 10] [--calls 3] [--shapes 1024x2000,64x20000] [--lookbacks 64,256,1024]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

MATCH, GAP_OPEN, GAP_EXTEND, BAND, MAX_DIST = 1, 3, 1, 50, 5000


def problems(k, n, seed=0x5EED0020):
    """k problems of n anchors in (be, ae) order: (a, b, len) as k x n int64 arrays."""
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.integers(1, 9, size=(k, n)), axis=1)
    diag = np.where(rng.random((k, n)) < 0.9, rng.integers(0, 4, size=(k, n)), 500 * rng.integers(1, 9, size=(k, n)))
    ln = np.full((k, n), 15, dtype=np.int64)
    a, b = (pos + diag).astype(np.int64), pos.astype(np.int64)
    order = np.lexsort((a + ln, b + ln), axis=1)
    return tuple(np.take_along_axis(x, order, axis=1) for x in (a, b, ln))


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=len(v))


def measure(LB, api, torch, k, n, lookback, reps, calls):
    dev = torch.device("cuda", 0)
    a, b, ln = problems(k, n)
    off = (np.arange(k + 1) * n).astype(np.int64)
    da, db, dl, doff = (torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev) for x in (a, b, ln, off))
    f = torch.empty(k * n, dtype=torch.int32, device=dev)
    pred = torch.empty(k * n, dtype=torch.int32, device=dev)
    status = torch.empty(k, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def launch():
        LB.check(LB.lib().msa_chain_run(ptr(da), ptr(db), ptr(dl), k, ptr(doff), MATCH, GAP_OPEN, GAP_EXTEND, BAND,
                                        MAX_DIST, lookback, ptr(f), ptr(pred), ptr(status),
                                        C.c_void_p(stream.cuda_stream)), "msa_chain_run")

    for _ in range(3):
        launch()
    torch.cuda.synchronize(dev)
    assert int(status.abs().max()) == 0
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    # the same f and pred from the host entry (and its chains, for the record)
    kw = dict(band=BAND, match=MATCH, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND, max_dist=MAX_DIST, lookback=lookback)
    cols = [list(x) for x in (a, b, ln)]
    chains, hf, hp = api.chain_seeds_batch(*cols, full=True, **kw)   # (warm-up of the end-to-end call as well)
    assert (np.concatenate(hf) == f.cpu().numpy()).all() and (np.concatenate(hp) == pred.cpu().numpy()).all()
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        api.chain_seeds_batch(*cols, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
    with_pred = float((pred >= 0).float().mean())
    return dict(kernel_ms=summary(ms), ns_per_anchor=round(1e6 * statistics.median(ms) / n, 1),
                chain_seeds_batch_ms=summary(wall), anchors_with_predecessor=round(with_pred, 4),
                best_chain_mean_anchors=round(float(np.mean([len(c[0]["anchors"]) for c in chains])), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--shapes", default="1024x2000,64x20000")
    ap.add_argument("--lookbacks", default="64,256,1024")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_chain.py needs a GPU (there is no fallback)")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd import api

    line = dict(script="time_chain", match=MATCH, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND, band=BAND,
                max_dist=MAX_DIST, device=torch.cuda.get_device_name(0))
    for shape in args.shapes.split(","):
        k, n = (int(x) for x in shape.split("x"))
        for lookback in (int(x) for x in args.lookbacks.split(",")):
            line[f"{k}x{n}_lookback{lookback}"] = measure(LB, api, torch, k, n, lookback, args.reps, args.calls)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
