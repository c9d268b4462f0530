"""The steady-state groups of the SW-linear chain wave (msa_flow.hip: run_gphase / run_group) at the sizes where a
stripe starts, repeats and leaves them, every H cell and the score against the oracle.

A stripe runs phases [16, qa & ~15) in unrolled groups of 16 (ring slot = the phase's index in the group, a
compile-time constant) when the code rows fit LDS whole; its first 16 phases, its tail, its masked phases and
ring-code pairs run the generic phase.  The last stripe runs groups too, its blocks going to an out ring that nothing
reads (every pair below has one; at m 129 it is the second of two stripes).  A stripe enters its first group when
qa >= 32: stripe 0 at n = 449 (448 does not); other stripes shift by cs in [-15, 0] and by their producer's last
block, so around n = 440-480 some stripes of one pair run a group and others do not.
  n: 440, 448, 449, 450, 464, 465, 480 (zero or one group); 704, 705, 720 (a second group: ring slots reused);
     1300 (groups, then the masked tail)
  m: 129 (a dq 3 link), 257 (dq 4), 513 (a second item: the row above through granules, dq_in 0 on wave 0), 1100,
     2200 (stripes 16 and 17: cs wraps, dq 3 again); 510 (four stripes: the last one is an item's last wave, its
     out ring the io-out link's)
Scores: (1, 0, g 1) the benched G-space instantiation, (3, 0, g 2) G-space with other profile bytes, (2, -3, g 2)
X-space.  Inputs: seeded random ACGT, and A == B (the long diagonal: the largest values on the links).
Also: score-only plans (one row per lane, no pass 2: they keep the generic phase at every size), the end-cell twin,
a ring-code pair (n 20,500: the generic path), and one plan run twice on different inputs (the epoch advances
through the groups' SNAP stores).  Integer DP: every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SCORINGS = [(1, 0, 1), (3, 0, 2), (2, -3, 2)]
NS = [440, 448, 449, 450, 464, 465, 480, 704, 705, 720, 1300]
MS = [129, 257, 510, 513, 1100, 2200]
KINDS = ["random", "equal"]


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


def _enc(s: bytes) -> np.ndarray:
    return np.frombuffer(s.translate(bytes.maketrans(b"ACGT", b"\x00\x01\x02\x03")), dtype=np.uint8).copy()


def _dev(x, dev):
    import torch

    return torch.from_numpy(_enc(x)).to(dev)


def _pair(kind, m, n, seed=0):
    rng = np.random.default_rng(1000 * m + n + 7919 * seed)
    if kind == "random":
        return rng.choice(ACGT, m).tobytes(), rng.choice(ACGT, n).tobytes()
    s = rng.choice(ACGT, max(m, n)).tobytes()  # equal: one sequence, cut to m and to n
    return s[:m], s[:n]


def _plan(LB, cells, scoring, m, n, track_end=False):
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ma, mi, g = scoring
    pl = Plan(LB.SW_LINEAR, cells, [m], [n], [0], [0], match=ma, mismatch=mi, gap_open=g, gap_extend=g,
              track_end=track_end, single=True)
    assert pl.launch_info()["mode"] == "flow", pl.launch_info()
    return pl


def _run_check_h(oracle, dev, pl, scoring, A, B, track_end, what):
    import torch

    ma, mi, g = scoring
    H = torch.empty(pl.cells_elems, dtype=torch.int32, device=dev)
    pl.run(_dev(A, dev), _dev(B, dev), H)
    res = pl.results()[0]
    assert pl.error() == 0, what
    o = oracle.sw(A, B, ma, mi, g, g, want_h=True)
    assert res["score"] == o["score"], what
    if track_end:
        assert tuple(res["end"]) == tuple(o["end"]), what
    bad = np.argwhere(pl.deskew(H.cpu().numpy(), 0, pl.stripe_meta())[1:, 1:] != o["H"][1:, 1:])
    assert len(bad) == 0, (what, len(bad), bad[:4] + 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scoring", SCORINGS)
def test_group_h_cells(oracle, dev, LB, scoring, kind):
    for m in MS:
        for n in NS:
            pl = _plan(LB, LB.CELLS_H, scoring, m, n)
            assert pl.launch_info()["rows_per_lane"] == 2
            A, B = _pair(kind, m, n)
            _run_check_h(oracle, dev, pl, scoring, A, B, False, (kind, m, n))


@pytest.mark.parametrize("scoring", SCORINGS)
def test_group_h_cells_with_end_cell(oracle, dev, LB, scoring):
    """The instantiation that also tracks the end cell (pass 1 is the same code)."""
    for (m, n) in [(257, 449), (513, 705), (2200, 1300)]:
        pl = _plan(LB, LB.CELLS_H, scoring, m, n, track_end=True)
        A, B = _pair("random", m, n)
        _run_check_h(oracle, dev, pl, scoring, A, B, True, ("end", m, n))


@pytest.mark.parametrize("scoring", SCORINGS)
def test_group_score_only(oracle, dev, LB, scoring):
    """CELLS_NONE: pass 1 alone keeps the best cell (one row per lane, no SNAP; the generic phase throughout)."""
    ma, mi, g = scoring
    for kind, (m, n) in [("random", (129, 449)), ("equal", (257, 464)), ("random", (513, 705)), ("equal", (1100, 1300)),
                         ("random", (1100, 448))]:
        A, B = _pair(kind, m, n)
        pl = _plan(LB, LB.CELLS_NONE, scoring, m, n)
        pl.run(_dev(A, dev), _dev(B, dev))
        assert pl.error() == 0
        assert pl.results()[0]["score"] == oracle.sw(A, B, ma, mi, g, g)["score"], (kind, m, n)


def test_ring_code_pair_takes_the_generic_path(oracle, dev, LB):
    """n = 20,500: a whole code row per copy does not fit LDS, so the codes stream through the rings and no stripe
    runs a group (their code addresses are linear)."""
    m, n = 129, 20500
    pl = _plan(LB, LB.CELLS_H, (1, 0, 1), m, n)
    assert pl.launch_info()["lds_bytes"] < 8 * n, pl.launch_info()  # eight whole copies would need more
    A, B = _pair("random", m, n)
    _run_check_h(oracle, dev, pl, (1, 0, 1), A, B, False, ("ring codes", m, n))


@pytest.mark.parametrize("scoring", [(1, 0, 1), (2, -3, 2)])
def test_group_plan_runs_twice(oracle, dev, LB, scoring):
    """One plan, two runs on different inputs: the second run's epoch goes through the groups' SNAP stores and the
    granules, and no value of the first run survives."""
    m, n = 513, 720
    pl = _plan(LB, LB.CELLS_H, scoring, m, n)
    for seed in (0, 1):
        A, B = _pair("random", m, n, seed)
        _run_check_h(oracle, dev, pl, scoring, A, B, False, ("run", seed))
