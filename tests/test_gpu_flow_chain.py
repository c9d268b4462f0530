"""The SW-linear pass-1 step of the two-pass flow kernel (flow_kernel, two rows per lane) at the shapes where a
step can go wrong, every H cell and the score against the oracle.

The G-space step (scores >= 0) is one hand-ordered asm block (fl_step2_gs, msa_flow.hip): two SDWA adds, the DPP
that brings the cell above, the two rows' v_max3.  Lane 0 takes the producer's ring value through the DPP's `old`
operand, the last lane of an odd m holds one row, and every 16th step reads a new block of ring inputs and codes.
  m: 1, 2 (one lane), 127 / 128 (the last lane with one row / two), 129 (a second stripe: lane 0 takes a producer's
     value), 257, 513 (a second item of four stripes: the row above arrives through granules and io-in), 1100
  n: 1, 15 / 16 / 17 (a phase boundary), 64 / 65 (the lane skew), 300, 1300 (a producer's last block, masked inputs)
Scores: (1, 0, g 1) is the benched G-space instantiation, (3, 0, g 2) G-space with other profile bytes, (2, -3, g 2)
X-space (zero floor), whose step is the compiler's.  Inputs: seeded random ACGT; A == B (the long diagonal, the
largest values); all-mismatch (everything at the floor); a 4-periodic repeat (ties between the three sources).
Integer DP: every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SCORINGS = [(1, 0, 1), (3, 0, 2), (2, -3, 2)]
PAIRS = [(1, 1), (1, 1300), (2, 17), (127, 16), (128, 15), (129, 64), (129, 300), (257, 65), (257, 1300), (513, 17),
         (513, 300), (1100, 1), (1100, 1300)]
KINDS = ["random", "equal", "mismatch", "periodic"]


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _enc(s: bytes) -> np.ndarray:
    return np.frombuffer(s.translate(bytes.maketrans(b"ACGT", b"\x00\x01\x02\x03")), dtype=np.uint8).copy()


def _dev(x, dev):
    import torch

    return torch.from_numpy(_enc(x)).to(dev)


def _pair(kind, m, n):
    rng = np.random.default_rng(1000 * m + n)
    if kind == "random":
        return rng.choice(ACGT, m).tobytes(), rng.choice(ACGT, n).tobytes()
    if kind == "equal":  # one sequence, cut to m and to n: the diagonal runs to min(m, n)
        s = rng.choice(ACGT, max(m, n)).tobytes()
        return s[:m], s[:n]
    if kind == "mismatch":
        return b"A" * m, b"C" * n
    return (b"ACGT" * (m // 4 + 1))[:m], (b"CGTA" * (n // 4 + 1))[:n]


def _check_h(oracle, dev, LB, scoring, kind, m, n, track_end):
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ma, mi, g = scoring
    A, B = _pair(kind, m, n)
    pl = Plan(LB.SW_LINEAR, LB.CELLS_H, [m], [n], [0], [0], match=ma, mismatch=mi, gap_open=g, gap_extend=g,
              track_end=track_end, single=True)
    info = pl.launch_info()
    assert info["mode"] == "flow" and info["rows_per_lane"] == 2, info
    H = torch.empty(pl.cells_elems, dtype=torch.int32, device=dev)
    pl.run(_dev(A, dev), _dev(B, dev), H)
    res = pl.results()[0]
    assert pl.error() == 0
    o = oracle.sw(A, B, ma, mi, g, g, want_h=True)
    assert res["score"] == o["score"], (kind, m, n)
    if track_end:
        assert tuple(res["end"]) == tuple(o["end"]), (kind, m, n)
    bad = np.argwhere(pl.deskew(H.cpu().numpy(), 0, pl.stripe_meta())[1:, 1:] != o["H"][1:, 1:])
    assert len(bad) == 0, (kind, m, n, len(bad), bad[:4] + 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scoring", SCORINGS)
def test_flow_chain_h_cells(oracle, dev, LB, scoring, kind):
    for (m, n) in PAIRS:
        _check_h(oracle, dev, LB, scoring, kind, m, n, False)


@pytest.mark.parametrize("scoring", SCORINGS)
def test_flow_chain_h_cells_with_end_cell(oracle, dev, LB, scoring):
    """The instantiation that also tracks the end cell (pass 1 is the same step)."""
    for (m, n) in [(129, 64), (257, 1300), (513, 300)]:
        _check_h(oracle, dev, LB, scoring, "random", m, n, True)


@pytest.mark.parametrize("scoring", SCORINGS)
def test_flow_chain_score_only(oracle, dev, LB, scoring):
    """CELLS_NONE: pass 1 alone keeps the best cell (one row per lane)."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ma, mi, g = scoring
    for kind, (m, n) in [("random", (129, 300)), ("equal", (257, 65)), ("periodic", (513, 1300)), ("mismatch", (65, 17))]:
        A, B = _pair(kind, m, n)
        pl = Plan(LB.SW_LINEAR, LB.CELLS_NONE, [m], [n], [0], [0], match=ma, mismatch=mi, gap_open=g, gap_extend=g,
                  track_end=False, single=True)
        assert pl.launch_info()["mode"] == "flow"
        pl.run(_dev(A, dev), _dev(B, dev))
        assert pl.error() == 0
        assert pl.results()[0]["score"] == oracle.sw(A, B, ma, mi, g, g)["score"], (kind, m, n)
