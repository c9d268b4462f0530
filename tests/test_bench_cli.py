"""bench.py's command line (no GPU): a plain run is the default, --full and --dump-outputs are options."""
import sys

import bench


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup, a.workload) == (1, 7, 2, "c2")
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_outputs_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline", "--dump-outputs", "some/dir"])
    a = bench.parse()
    assert a.full is True and a.no_cpu_baseline is True and a.dump_outputs == "some/dir"


def test_dump_sample_fits_the_size_limit():
    # per sampled cell: (i, j) and the cell, float64 each; scores and traceback ops are far below the rest
    assert bench.DUMP_SAMPLE_CELLS * 3 * 8 <= 32 * 2**20
