"""The compiled shape of the SW-linear chain wave's steady-state groups (msa_flow.hip: run_gphase / run_group) in
libmsa.so's gfx950 code object, for the benched C2 instantiation and its end-cell twin.

A group is 16 unrolled phases whose index J in the group -- the phase's slot in the 16-block rings -- is a
compile-time constant, so the per-phase bookkeeping of the generic phase (ring and code addresses, the
write-slot select, the dummy sink, the segment test, the loop and parity counters) is an immediate offset, a
carried register or gone.  A lone chain wave pays an issue slot for every instruction, so
the instruction count of a phase is the point.  The parent's leanest steady phase had 152 instructions from one
hand-off to the next; this file checks, on the CPU, that the library holds a straight-line run of at least 8
consecutive phases of at most 137 each (15 under), that their ring reads share one address register and differ
only in their immediate offsets, that no code address goes through a ring mask, and that nothing spills there."""
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
MAX_PHASE = 137  # instructions from one hand-off to the next: 15 under the parent's leanest phase (152)
MIN_RUN = 8


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


def _target(insts, ops):
    """Address a branch's operand points at, or None."""
    m = re.search(r"<(.+?)(?:\+0x([0-9a-f]+))?>", ops)
    if not m:
        return None
    return insts[0][0] + (int(m.group(2), 16) if m.group(2) else 0)


def _straight(insts, lo, hi):
    """insts(lo, hi] runs top to bottom: no unconditional transfer and no backward branch inside it (forward
    conditional branches -- to the out-of-line slow paths -- are what a phase has)."""
    for a, mn, ops in insts[lo + 1:hi + 1]:
        if mn in ("s_branch", "s_endpgm", "s_setpc_b64", "s_swappc_b64"):
            return False
        if mn.startswith("s_cbranch"):
            t = _target(insts, ops)
            if t is None or t <= a:
                return False
    return True


def _phases(insts):
    """[(lo, hi)]: instruction index ranges (lo, hi] from one add-TID offset:60 hand-off to the next in address
    order."""
    h = [k for k, (_, m, o) in enumerate(insts) if m == "ds_write_addtid_b32" and "offset:60" in o]
    return list(zip(h, h[1:]))


def _lean_runs(insts):
    """Maximal runs of consecutive straight-line phases of at most MAX_PHASE instructions with their 16 steps."""
    runs, cur = [], []
    for lo, hi in _phases(insts):
        steps = sum(1 for _, m, o in insts[lo + 1:hi + 1] if m == "v_mov_b32_dpp" and "wave_shr:1" in o)
        if hi - lo <= MAX_PHASE and steps == 16 and _straight(insts, lo, hi):
            cur.append((lo, hi))
        else:
            if cur:
                runs.append(cur)
            cur = []
    if cur:
        runs.append(cur)
    return runs


def _addr_reg(ops):
    # ds_read_b128 v[4:7], v1 offset:16  /  ds_read2_b64 v[4:7], v1 offset0:2 offset1:3
    return ops.split(",")[1].split()[0]


def _offset(ops):
    m = re.search(r"\boffset:(\d+)", ops)
    return int(m.group(1)) if m else 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_group_phases_are_lean_and_straight_line(functions, kernel):
    insts = functions[kernel]
    lens = [hi - lo for lo, hi in _phases(insts)]
    runs = _lean_runs(insts)
    print(f"{kernel}: hand-off to hand-off instruction counts {lens}; lean runs {[len(r) for r in runs]}")
    assert runs, f"no straight-line phase of <= {MAX_PHASE} instructions: {lens}"
    best = max(runs, key=len)
    assert len(best) >= MIN_RUN, (len(best), lens)
    lo, hi = best[0][0], best[-1][1]
    body = insts[lo + 1:hi + 1]
    assert max(h - l for l, h in best) <= MAX_PHASE
    # nothing spills in the run
    assert not [hex(a) for a, m, _ in body if m.startswith("scratch_")]
    # ring reads: one address register, every read its own immediate offset
    ring = [(a, _addr_reg(o), _offset(o)) for a, m, o in body if m == "ds_read_b128"]
    assert len(ring) == 4 * len(best), (len(ring), len(best))
    assert len({r for _, r, _ in ring}) == 1, sorted({r for _, r, _ in ring})
    offs = [off for _, _, off in ring]
    assert len(set(offs)) == len(offs), offs
    for p in range(len(best)):  # a phase's four reads: one 64-byte block
        blk = sorted(offs[4 * p:4 * p + 4])
        assert blk == [blk[0], blk[0] + 16, blk[0] + 32, blk[0] + 48] and blk[0] % 64 == 0, blk
    # code reads: one per phase, and no address that a v_and_b32 (the code ring's mask) wrote
    code = [k for k, (_, m, _) in enumerate(body) if m == "ds_read2_b64"]
    assert len(code) == len(best), (len(code), len(best))
    for k in code:
        reg = _addr_reg(body[k][2])
        for a, m, o in reversed(body[:k]):
            if m.startswith("v_") and re.match(rf"{reg}\b", o.split(",")[0].strip()):
                assert m != "v_and_b32_e32" and not m.startswith("v_and_b32"), (hex(a), m, o)
                break
