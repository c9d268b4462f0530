"""The one-row-per-lane pass-2 block bodies (fill_block_aff, fill_block_got) against the stripe kernel and the oracle.

libmsa picks two rows per lane for the two-pass SW-affine and Gotoh flow plans; MSA_FLOW_AFF_R=1 /
MSA_FLOW_GOT_R=1 keep one row, and the library reads them once per process.  So the checks run in one fresh
child process that has both set (this file, run as a script); the pytest process keeps them unset
(test_gpu_plan_shapes asserts that).  The child reuses test_gpu_parity's comparisons: the direction / tag
bytes of every cell against the one-pass stripe kernel for in-launch pass 2 (the CALLER = 0 instantiations),
and a 70,000 x 300 pair each against the oracle for the separate pass-2 launch (CALLER = 1)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

R1_ENV = {"MSA_FLOW_AFF_R": "1", "MSA_FLOW_GOT_R": "1"}


def test_flow_one_row_per_lane_bodies():
    env = dict(os.environ)
    env.update(R1_ENV)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve())]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "one-row bodies ok: 8 plans" in r.stdout
    assert not [k for k in R1_ENV if k in os.environ]


def _child():
    import torch

    import conftest  # noqa: F401  (puts the repository root on sys.path)
    import test_gpu_parity as P
    from cse305_parallel_sequence_alignment_amd import _lib as LB
    from oracle import oracle as O

    assert all(os.environ.get(k) == v for k, v in R1_ENV.items())
    assert torch.cuda.is_available(), "no GPU visible"
    dev = torch.device("cuda", 0)
    O.build()
    plans = []

    def one_row_flow(pl, fill):
        info = pl.launch_info()
        assert info["mode"] == "flow" and info["rows_per_lane"] == 1 and (info["fill_grid"] > 0) == fill, info
        assert pl.run_info()["mode"] == "flow"
        assert pl.error() == 0
        plans.append(info)

    for (m, n) in [(65, 70), (300, 257), (1000, 1300)]:
        one_row_flow(P.check_sw_affine_flow_dir_bytes(dev, LB, m, n, (2, -3, 5, 2), rows=1), False)
    for (m, n) in [(65, 66), (129, 700), (1000, 1300)]:
        one_row_flow(P.check_gotoh_flow_dir_bytes(dev, LB, (1, 2), m, n), False)
    for kind in ("swa_neg", "gotoh"):  # 70,000 x 300: flow_fill_kernel
        one_row_flow(P.check_flow_fill_launch_tall_pair(O, dev, LB, kind), True)
    print(f"one-row bodies ok: {len(plans)} plans")


if __name__ == "__main__":
    _child()
