"""The compiled shape of the SW-linear pass-1 step (flow_kernel, G-space, two rows per lane) in libmsa.so's gfx950
code object: the benched C2 instantiation and its end-cell twin.

fl_step2_gs (msa_flow.hip) writes the step as one ordered asm block so that the two SDWA adds stand between the
previous step's row-2 v_max3 and the DPP that reads it (two wait states, no s_nop).  A lone chain wave pays an issue
slot for every instruction, padding included, so the order is the point: this file checks, on
the CPU, that the compiler kept it -- every step is `add, add, DPP, max3, max3` back to back, a phase has 16 of
them, and nothing spills inside the phase code.  The wait states themselves are test_host.py's
test_asm_hazards_have_their_wait_states."""
import importlib.util
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SO = ROOT / "cse305_parallel_sequence_alignment_amd" / "libmsa.so"
# flow_kernel<FLOOR = false, BEST = false, SAVE = true, TRACKPOS, R = 2, FK = 0>
KERNELS = ["_ZN3msa11flow_kernelILb0ELb0ELb1ELb0ELi2ELi0EEEvNS_5KArgsE",
           "_ZN3msa11flow_kernelILb0ELb0ELb1ELb1ELi2ELi0EEEvNS_5KArgsE"]
STEP = ["v_add_u32_sdwa", "v_add_u32_sdwa", "v_mov_b32_dpp", "v_max3_i32", "v_max3_i32"]


def _waitloops():
    sys.path.insert(0, str(ROOT / "scripts"))
    spec = importlib.util.spec_from_file_location("waitloops", ROOT / "scripts" / "waitloops.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def functions():
    if not SO.exists():
        pytest.skip("libmsa.so not built")
    W = _waitloops()
    return W.functions(W.disassemble(SO))


def _dst(ops: str) -> str:
    return ops.split(",")[0].strip()


def _reads(ops: str, reg: str) -> bool:
    return re.search(rf"\b{reg}\b", ops.split(",", 1)[1]) is not None


@pytest.mark.parametrize("kernel", KERNELS)
def test_sw_linear_step_is_one_ordered_block(functions, kernel):
    insts = functions[kernel]
    mn = [m for _, m, _ in insts]
    dpps = [k for k, (_, m, o) in enumerate(insts) if m == "v_mov_b32_dpp" and "wave_shr:1" in o]
    assert dpps and len(dpps) % 16 == 0, len(dpps)
    for k in dpps:
        assert mn[k - 2:k + 3] == STEP, (hex(insts[k][0]), mn[k - 2:k + 3])
        up, h1 = _dst(insts[k][2]), _dst(insts[k + 1][2])
        assert _reads(insts[k + 1][2], up) and _reads(insts[k + 2][2], h1), hex(insts[k][0])
        # the DPP's source is the previous step's row 2: not written by either add in front of it
        src = insts[k][2].split(",")[1].split()[0]
        assert src not in (_dst(insts[k - 1][2]), _dst(insts[k - 2][2])), hex(insts[k][0])
    # phases: 16 steps per hand-off (its 16th add-TID write), and no spill code among a phase's steps
    handoffs = [k for k, (_, m, o) in enumerate(insts) if m == "ds_write_addtid_b32" and "offset:60" in o]
    assert len(dpps) == 16 * len(handoffs), (len(dpps), len(handoffs))
    for p in range(0, len(dpps), 16):
        lo, hi = dpps[p], dpps[p + 15]
        assert not [m for m in mn[lo:hi] if m.startswith("scratch_")], hex(insts[lo][0])
        assert not [k for k in handoffs if lo < k < hi], hex(insts[lo][0])
