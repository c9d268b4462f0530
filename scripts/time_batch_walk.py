"""Time the batch walk against the loop of single-pair walks (MI355X; there is no fallback: without a GPU it fails).

Workload: 256 pairs of 4,096 x 4,096, SW_AFFINE with direction bytes and track_end, match 2 / mismatch -1 / open 3 /
extend 1, as ONE batch plan; once with B = A mutated (data.mutate, seeded: long diagonal runs, a few short gaps) and
once with independent random A and B (short runs, many gaps: the walk's worst case).  Per input, after a warm-up
of every launch shape, HIP events time
  (a) the fill (msa_plan_run),
  (b) msa_plan_traceback_batch: every walk in one launch,
  (c) 256 msa_plan_traceback calls on the same stream: what there was before the batch walk,
each over enough repetitions to exceed 0.5 s per figure, (b) and (c) alternating, ROUNDS figures each (median,
min and max are reported: the spread is max - min).  (b)'s ops and info words 0-3 must equal (c)'s byte for byte.
Prints one JSON line.

    python scripts/time_batch_walk.py [--pairs 256] [--len 4096] [--rounds 5]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cse305_parallel_sequence_alignment_amd import _lib as LB  # noqa: E402
from cse305_parallel_sequence_alignment_amd import data  # noqa: E402
from cse305_parallel_sequence_alignment_amd.plan import Plan  # noqa: E402

SCORING = dict(match=2, mismatch=-1, gap_open=3, gap_extend=1)
MIN_S = 0.5  # seconds per figure


def make_pairs(kind: str, k: int, ln: int):
    As = [data.synth(ln, 0x5EEDB000 + p) for p in range(k)]
    if kind == "mutated":
        # (a mutated copy changes length: mutate a longer piece, cut to ln)
        Bs = [data.mutate(As[p] + data.synth(64, 0x5EEDC000 + p), 0x5EEDD000 + p)[:ln] for p in range(k)]
    else:
        Bs = [data.synth(ln, 0x5EEDE000 + p) for p in range(k)]
    assert all(len(b) == ln for b in Bs)
    return As, Bs


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps  # ms per call of fn


def figures(torch, fns, rounds):
    """{name: [ms per call] * rounds}: repetitions sized so that each figure takes > MIN_S, the fns alternating."""
    reps = {}
    for name, fn in fns.items():
        fn()  # warm-up of this launch shape
        torch.cuda.synchronize()
        once = timed(torch, fn, 2)
        reps[name] = max(2, math.ceil(1.1 * MIN_S * 1e3 / max(once, 1e-3)))
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms = timed(torch, fn, reps[name])
            assert ms * reps[name] > MIN_S * 1e3, (name, ms, reps[name])
            out[name].append(ms)
    return out, reps


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def measure(torch, dev, kind, k, ln, rounds):
    As, Bs = make_pairs(kind, k, ln)
    offs = [p * ln for p in range(k)]
    pl = Plan(LB.SW_AFFINE, LB.CELLS_DIR, [ln] * k, [ln] * k, offs, offs, track_end=True, single=False, **SCORING)
    dA = torch.from_numpy(data.encode(b"".join(As))).to(dev)
    dB = torch.from_numpy(data.encode(b"".join(Bs))).to(dev)
    D = torch.empty(pl.cells_elems, dtype=torch.uint8, device=dev)
    off = Plan.ops_layout(pl.ms, pl.ns)
    d_off = torch.tensor(off, dtype=torch.int64, device=dev)
    ops_b = torch.zeros(off[-1], dtype=torch.uint8, device=dev)
    ops_c = torch.zeros(off[-1], dtype=torch.uint8, device=dev)
    info_b = torch.zeros(8 * k, dtype=torch.int64, device=dev)
    info_c = torch.zeros(8 * k, dtype=torch.int64, device=dev)
    views = [(ops_c[off[p]:off[p + 1]], info_c[8 * p:8 * p + 8]) for p in range(k)]

    def fill():
        pl.run(dA, dB, D)

    def batch_walk():
        pl.traceback_batch_async(D, ops_b, d_off, info_b)

    def loop_walk():
        for p, (o, i) in enumerate(views):
            pl.traceback_async(D, o, i, pair=p)

    fill()
    torch.cuda.synchronize()
    pl.results()  # (raises on a sticky plan error)
    ms, reps = figures(torch, dict(fill=fill, batch_walk=batch_walk, loop_walk=loop_walk), rounds)
    torch.cuda.synchronize()
    assert pl.error() == 0
    ib, ic = info_b.cpu().numpy().reshape(k, 8), info_c.cpu().numpy().reshape(k, 8)
    assert (ib[:, 3] == 0).all() and (ic[:, 3] == 0).all(), "a walk failed"
    assert (ib[:, :4] == ic[:, :4]).all(), "the batch walk's info differs from the single walker's"
    hb, hc = ops_b.cpu().numpy(), ops_c.cpu().numpy()
    for p in range(k):
        n_ops = int(ib[p, 0])
        assert n_ops > 0 and (hb[off[p]:off[p] + n_ops] == hc[off[p]:off[p] + n_ops]).all(), p
    b, c, f = (statistics.median(ms[x]) for x in ("batch_walk", "loop_walk", "fill"))
    return dict(fill_ms=summary(ms["fill"]), batch_walk_ms=summary(ms["batch_walk"]), loop_walk_ms=summary(ms["loop_walk"]),
                reps=reps, loop_over_batch=round(c / b, 2), batch_walk_over_fill=round(b / f, 4),
                ops_per_walk=round(float(ib[:, 0].mean()), 1), stripes_per_walk=round(float(ib[:, 4].mean()), 1),
                groups_per_walk=round(float(ib[:, 5].mean()), 1), ticks_per_walk=round(float(ib[:, 6].mean()), 1),
                ticks_max=int(ib[:, 6].max()), ops_equal=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_batch_walk.py needs a GPU (there is no fallback)")
    dev = torch.device("cuda", 0)
    line = dict(script="time_batch_walk", pairs=args.pairs, m=args.len, n=args.len, alg="SW_AFFINE", cells="DIR",
                scoring=SCORING, rounds=args.rounds, device=torch.cuda.get_device_name(0))
    for kind in ("mutated", "random"):
        line[kind] = measure(torch, dev, kind, args.pairs, args.len, args.rounds)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
