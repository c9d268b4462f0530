"""Time one seed_align_batch call against what the library offered for the same answer before it: two
extend_align_batch(band=, xdrop=) calls on flanks cut and reversed on the host (MI355X; there is no fallback: without a
GPU it fails).

Shape: 256 seeds of 16 symbols in the middle of 2,048 x 2,048 pairs, bands 64 and 256, xdrop 50, 4 symbols, +2 / -3,
gap_open 5, gap_extend 2, with CIGARs.  Two workloads (seeded):
  (a) similar   B is A with a tenth of its symbols substituted: both flanks run to their ends.
  (b) flanks    200 common symbols on each side of the seed, then unrelated ones: both flanks stop early.
Per workload and band, in one process and alternately after one warm-up call each, `--calls` calls (wall-clock, uploads,
walks and CIGARs included):
  seed     api.seed_align_batch: one call, the left flanks read backwards in place;
  by_hand  cutting the four flanks of every seed and reversing the two left ones (bytes slices), then
           api.extend_align_batch on the left flanks and on the right flanks.  Adding the seed's score, fixing up the
           coordinates and gluing the three CIGARs -- what a caller still had to do -- is left out of the timing.
Before timing, every flank's score, end cell and diagonals of the one call are checked against the two calls'.
Reported: median, min and max per variant and the ratio of medians seed / by_hand.  Prints one JSON line.

    python scripts/time_seed_align.py [--seeds 256] [--len 2048] [--bands 64,256] [--calls 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

GAP_OPEN, GAP_EXTEND, MATCH, MISMATCH, XDROP, SEED_LEN = 5, 2, 2, -3, 50, 16


def similar(k, m):
    rng = np.random.default_rng(0x5EED0010)
    A = rng.integers(0, 4, size=(k, m), dtype=np.uint8)
    B = A.copy()
    hit = rng.random((k, m)) < 0.1
    B[hit] = (B[hit] + 1 + rng.integers(0, 3, size=int(hit.sum()), dtype=np.uint8)) % 4
    return A, B


def flanks(k, m, common=200):
    rng = np.random.default_rng(0x5EED0011)
    A = rng.integers(0, 4, size=(k, m), dtype=np.uint8)
    B = rng.integers(0, 4, size=(k, m), dtype=np.uint8)
    lo, hi = (m - SEED_LEN) // 2 - common, (m - SEED_LEN) // 2 + SEED_LEN + common
    B[:, lo:hi] = A[:, lo:hi]
    return A, B


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=len(v))


def measure(api, A, B, band, calls):
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    As, Bs = [lut[a].tobytes() for a in A], [lut[b].tobytes() for b in B]
    k, m = A.shape
    at = (m - SEED_LEN) // 2
    sa = sb = [at] * k
    sl = [SEED_LEN] * k
    kw = dict(match=MATCH, mismatch=MISMATCH, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND)

    def seed():
        return api.seed_align_batch(As, Bs, sa, sb, sl, band, xdrop=XDROP, **kw)

    def by_hand():
        la = [a[:at][::-1] for a in As]
        lb = [b[:at][::-1] for b in Bs]
        ra = [a[at + SEED_LEN:] for a in As]
        rb = [b[at + SEED_LEN:] for b in Bs]
        return (api.extend_align_batch(la, lb, band=band, xdrop=XDROP, **kw),
                api.extend_align_batch(ra, rb, band=band, xdrop=XDROP, **kw))

    one, (left, right) = seed(), by_hand()  # warm-up, and the same answers
    for r, L, R in zip(one, left, right):
        for f, x in ((r["left"], L), (r["right"], R)):
            assert all(f[key] == x[key] for key in ("score", "a_end", "b_end", "diagonals", "dropped")), (f, x)
    ms = dict(seed=[], by_hand=[])
    for _ in range(calls):
        for name, fn in (("seed", seed), ("by_hand", by_hand)):
            t0 = time.perf_counter()
            fn()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    return dict(seed_ms=summary(ms["seed"]), by_hand_ms=summary(ms["by_hand"]),
                ratio_seed_over_by_hand=round(statistics.median(ms["seed"]) / statistics.median(ms["by_hand"]), 4),
                mean_left_diagonals=float(np.mean([r["left"]["diagonals"] for r in one])),
                mean_right_diagonals=float(np.mean([r["right"]["diagonals"] for r in one])),
                dropped_flanks=int(sum(r[f]["dropped"] for r in one for f in ("left", "right"))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=256)
    ap.add_argument("--len", type=int, default=2048)
    ap.add_argument("--bands", default="64,256")
    ap.add_argument("--calls", type=int, default=7)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_seed_align.py needs a GPU (there is no fallback)")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cse305_parallel_sequence_alignment_amd import api

    line = dict(script="time_seed_align", batch=[args.seeds, args.len, args.len], seed_len=SEED_LEN, xdrop=XDROP,
                gap_open=GAP_OPEN, gap_extend=GAP_EXTEND, device=torch.cuda.get_device_name(0))
    for band in (int(b) for b in args.bands.split(",")):
        for name, (A, B) in (("similar", similar(args.seeds, args.len)), ("flanks", flanks(args.seeds, args.len))):
            line[f"{name}_band{band}"] = measure(api, A, B, band, args.calls)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
