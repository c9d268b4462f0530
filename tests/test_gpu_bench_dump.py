"""bench.py's plain run and --dump-outputs: the seeded cell sample addresses the plan's skewed cell output
exactly, and a plain C2 run writes the last timed step's outputs, equal to the oracle's."""
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
TR = bytes.maketrans(b"ACGT", b"\x00\x01\x02\x03")


def _dev(x, dev):
    import torch

    return torch.from_numpy(np.frombuffer(x.translate(TR), dtype=np.uint8).copy()).to(dev)


# one-row-per-lane stripes; the two-pass flow kernel's two rows per lane (several workgroups); a band (the
# sample stays inside it); direction bytes (16 per lane and block) in the two-rows-per-lane layout
@pytest.mark.parametrize("kind,m,n,band,rows_per_lane", [("sw_h", 700, 650, -1, 1), ("sw_h", 1500, 1203, -1, 2),
                                                        ("banded_h", 1000, 990, 64, 1),
                                                        ("affine_dir", 1000, 1300, -1, 2)])
def test_sample_cells_addresses_every_sampled_cell(dev, kind, m, n, band, rows_per_lane):
    import torch

    import bench
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    rng = np.random.default_rng(m + n)
    A, B = rng.choice(ACGT, m).tobytes(), rng.choice(ACGT, n).tobytes()
    if kind == "sw_h":
        pl = Plan(LB.SW_LINEAR, LB.CELLS_H, [m], [n], [0], [0], match=1, mismatch=0, gap_open=1, gap_extend=1,
                  single=rows_per_lane == 2)  # a one-pair batch runs the stripe kernel
    elif kind == "banded_h":
        pl = Plan(LB.NW_BANDED, LB.CELLS_H, [m], [n], [0], [0], match=1, mismatch=0, gap_open=3, gap_extend=1,
                  band=band)
    else:
        pl = Plan(LB.SW_AFFINE, LB.CELLS_DIR, [m], [n], [0], [0], match=1, mismatch=0, gap_open=3, gap_extend=1,
                  track_end=True)
    assert pl.geom[0].rows_per_lane == rows_per_lane
    out = torch.empty(pl.cells_elems, dtype=torch.uint8 if kind == "affine_dir" else torch.int32, device=dev)
    pl.run(_dev(A, dev), _dev(B, dev), out)
    ij, idx = bench.sample_cells(pl, count=20000, seed=3)
    ij2, idx2 = bench.sample_cells(pl, count=20000, seed=3)
    assert np.array_equal(ij, ij2) and np.array_equal(idx, idx2)
    i, j = ij[:, 0], ij[:, 1]
    assert i.min() == 1 and i.max() == m and j.min() == 1 and j.max() == n  # 20000 draws reach every edge
    if band >= 0:
        assert np.abs(i - j).max() == band
    assert idx.min() >= 0 and idx.max() < pl.cells_elems
    host = out.cpu().numpy()
    full = (pl.deskew_dir if kind == "affine_dir" else pl.deskew)(host, 0, pl.stripe_meta())
    assert np.array_equal(host[idx], full[i, j])


def test_plain_run_dumps_last_step_outputs(oracle, dev, tmp_path, monkeypatch, capsys):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` (in this process): one JSON line with the
    headline fields and none of --full's, and float64 files within 64 MB holding C2's score and the H cells
    of the seeded sample, equal to the oracle's."""
    import bench
    from cse305_parallel_sequence_alignment_amd import data

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                                      "--dump-outputs", str(tmp_path / "dump")])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "GCUPS" and d["higher_is_better"] is True
    assert d["dtype"] == "int32" and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(1e8 / (d["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
    assert "cpu_baseline" not in d and "roofline" not in d and "c4_strong" not in d["config"]
    files = sorted((tmp_path / "dump").glob("*"))
    assert [f.name for f in files] == ["cells_sample.npy", "cells_sample_ij.npy", "scores.npy"]
    assert sum(f.stat().st_size for f in files) <= 64 * 10**6
    arrs = {f.stem: np.load(f) for f in files}
    assert all(a.dtype == np.float64 for a in arrs.values())
    A, B = data.c2_pair(0)
    o = oracle.sw(A, B, 1, 0, 1, 1, want_h=True)
    assert arrs["scores"].tolist() == [o["score"]] == [d["config"]["score_rank0"]]
    ij = arrs["cells_sample_ij"].astype(np.int64)
    assert len(ij) == bench.DUMP_SAMPLE_CELLS and ij.min() == 1 and ij.max() == 10000
    assert np.array_equal(arrs["cells_sample"], o["H"][ij[:, 0], ij[:, 1]])
