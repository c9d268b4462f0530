"""CPU yardsticks, inputs and shape lists of the two-value flow kernels' cell-by-cell tests (test_gpu_flow_dir.py).

Not a test file.  Numpy and plain Python only; test_flow_dir_reference.py checks all of it on the CPU.

* SW affine: sw_reference is sw_scored_reference under the 4-symbol match / mismatch table -- H, E, F, the byte plane
  (bits 0-3 under the contract in that file's docstring), the end cell, ops and beg.
* Gotoh (the reference's T1 / T2 / T3 with start type -1; f = 1 on equal symbols else 0):
      T1(i,j) = f + max(T1, T2, T3)(i-1,j-1)
      T2(i,j) = max(T1(i,j-1) - g - h, T2(i,j-1) - g, T3(i,j-1) - g - h)        (consumes B: op 'D')
      T3(i,j) = max(T1(i-1,j) - g - h, T2(i-1,j) - g - h, T3(i-1,j) - g)        (consumes A: op 'I')
  gotoh_tags makes the tag byte of every interior cell from the tables (bits 0-1 / 2-3 / 4-5 = 4 - the table that
  T1's / T2's / T3's maximum comes from, the first of T1, T2, T3 on a tie), unswapped_tables undoes the oracle's swap
  of a pair with m > n, gotoh_walk restates msa_plan_traceback_gotoh's walk over a tag plane and gotoh_rescore sums
  what its ops cost.
* sw_stream / gotoh_stream restate both recurrences one row at a time in O(n) memory (int64) for the tall pairs: the
  final result and the byte / tag rows of any row window.
* Inputs: one seeded ACGT builder per kind (pair_of), the tall pair (tall_pair), the shape and scoring lists both test
  files read, the flow kernels' stripe arithmetic (stripe_class) and the rule that selects the separate pass-2 launch
  (fill_launch_min_m).
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

import sw_scored_reference as SR

ACGT = b"ACGT"
_SYM = np.frombuffer(ACGT, dtype=np.uint8)
NEG = -(1 << 40)   # -inf of the int64 restatements; anything <= _NEGH is -inf
_NEGH = NEG // 2


def codes(x: bytes) -> np.ndarray:
    """ACGT -> 0..3 (uint8)."""
    return np.frombuffer(x.translate(bytes.maketrans(ACGT, b"\x00\x01\x02\x03")), dtype=np.uint8).copy()


def rs(rng, n: int) -> bytes:
    return rng.choice(_SYM, n).tobytes()


# ---- SW affine ---------------------------------------------------------------------------------------------------
def table4(ma: int, mi: int) -> np.ndarray:
    S = np.full((4, 4), mi, dtype=np.int64)
    S[np.arange(4), np.arange(4)] = ma
    return S


def sw_reference(A: bytes, B: bytes, scoring) -> dict:
    """sw_scored_reference of (match, mismatch, gap_open, gap_extend)."""
    ma, mi, go, ge = scoring
    return SR.sw_scored_reference(A, B, ACGT, table4(ma, mi), go, ge)


def sw_rescore(A: bytes, B: bytes, beg, ops: bytes, scoring):
    ma, mi, go, ge = scoring
    return SR.rescore(A, B, beg, ops, ACGT, table4(ma, mi), go, ge)


def sw_stream(A: bytes, B: bytes, scoring, windows=()) -> dict:
    """dict(score, end, rows): the SW-affine recurrence one row at a time.  rows[(lo, hi)] = the bytes (bits 0-3) of
    rows lo..hi (1-based, inclusive), shape (hi - lo + 1, n).  A row needs the row above and, for E, a left-to-right
    prefix maximum: E(i,j) = max over k < j of X(i,k) - gap_open - (j-1-k) gap_extend with X = max(0, diagonal, F),
    the cell without its E term -- exact for gap_open >= gap_extend >= 0, since a gap that continues out of E(i,k)
    costs no more than one reopened there."""
    ma, mi, go, ge = scoring
    assert go >= ge >= 0
    a, b = codes(A), codes(B)
    m, n = len(a), len(b)
    Sb = table4(ma, mi)[:, b]
    kge = np.arange(n + 1, dtype=np.int64) * ge
    Hp = np.zeros(n + 1, dtype=np.int64)
    Fp = np.full(n + 1, NEG, dtype=np.int64)
    X = np.zeros(n + 1, dtype=np.int64)
    out = {w: np.zeros((w[1] - w[0] + 1, n), dtype=np.uint8) for w in windows}
    best, end = 0, (0, 0)
    for i in range(1, m + 1):
        fo = Hp[1:] - go
        F = np.maximum(Fp[1:] - ge, fo)
        dg = Hp[:-1] + Sb[a[i - 1]]
        X[1:] = np.maximum(np.maximum(dg, F), 0)
        c = np.maximum.accumulate(X + kge)
        E = c[:-1] - go - kge[:-1]
        H = np.maximum(X[1:], E)
        for (lo, hi), rows in out.items():
            if lo <= i <= hi:
                eo = np.concatenate(([0], H[:-1])) - go
                hs = np.where(H == 0, 0, np.where(H == dg, 1, np.where(H == E, 2, 3)))
                rows[i - lo] = hs | np.where(E == eo, 4, 0) | np.where(F == fo, 8, 0)
        r = int(H.max())
        if r > best:
            best, end = r, (i, int(np.argmax(H)) + 1)
        Hp[1:], Fp[1:] = H, F
    return dict(score=best, end=end, rows=out)


# ---- Gotoh -------------------------------------------------------------------------------------------------------
def gotoh_tags(T1, T2, T3, g, h):
    """The REF1 tag byte of every cell from the reference's double tables: bits 0-1 / 2-3 / 4-5 = 4 - the table
    find_alignment's T1 / T2 / T3 branch picks (the first of T1, T2, T3 whose candidate is the maximum,
    subproblem_alignment.cpp:150-171)."""
    def first(c):
        return 4 - np.argmax(np.stack(c), axis=0).astype(np.uint8) - 1

    t1 = first([T1[:-1, :-1], T2[:-1, :-1], T3[:-1, :-1]])
    t2 = first([T1[1:, :-1] - g - h, T2[1:, :-1] - g, T3[1:, :-1] - g - h])
    t3 = first([T1[:-1, 1:] - g - h, T2[:-1, 1:] - g - h, T3[:-1, 1:] - g])
    return t1 | (t2 << 2) | (t3 << 4)


def unswapped_tables(oracle, A: bytes, B: bytes, g, h):
    """(T1, T2, T3), each (m+1) x (n+1), of the pair as given.  The oracle's Subproblem swaps a pair with m > n; the
    recurrence is symmetric under that swap with T2 and T3 exchanged, so the tables of the unswapped pair are
    T1' = T1^T, T2' = T3^T, T3' = T2^T."""
    T1, T2, T3, inv = oracle.subproblem_tables(A, B, -1, float(g), float(h))
    assert inv == (len(A) > len(B))
    if inv:
        T1, T2, T3 = T1.T.copy(), T3.T.copy(), T2.T.copy()
    return T1, T2, T3


def gotoh_triple_loop(A: bytes, B: bytes, g, h):
    """(T1, T2, T3, tags) cell by cell in plain Python floats, start type -1, for the pair as given (no swap); tags is
    m x n.  Shares no code with gotoh_tags or gotoh_stream."""
    m, n = len(A), len(B)
    ninf = float("-inf")
    T = [[[ninf] * (n + 1) for _ in range(m + 1)] for _ in range(3)]
    T[0][0][0] = 0.0
    for j in range(1, n + 1):
        T[1][0][j] = -h - g * j
    for i in range(1, m + 1):
        T[2][i][0] = -h - g * i
    tags = [[0] * n for _ in range(m)]

    def pick(c):  # (value, tag) of the first maximum
        k = 0
        if c[1] > c[k]:
            k = 1
        if c[2] > c[k]:
            k = 2
        return c[k], 3 - k

    for i in range(1, m + 1):
        for j in range(1, n + 1):
            f = 1.0 if A[i - 1] == B[j - 1] else 0.0
            v1, t1 = pick([T[0][i - 1][j - 1], T[1][i - 1][j - 1], T[2][i - 1][j - 1]])
            v3, t3 = pick([T[0][i - 1][j] - g - h, T[1][i - 1][j] - g - h, T[2][i - 1][j] - g])
            T[0][i][j], T[2][i][j] = f + v1, v3
            v2, t2 = pick([T[0][i][j - 1] - g - h, T[1][i][j - 1] - g, T[2][i][j - 1] - g - h])
            T[1][i][j] = v2
            tags[i - 1][j - 1] = t1 | (t2 << 2) | (t3 << 4)
    return T[0], T[1], T[2], tags


def gotoh_walk(tags, fin, m: int, n: int, i0: int = 1):
    """(ops end -> start, stop cell) of msa_plan_traceback_gotoh's walk for end type -1 over a tag plane: tags[i - i0,
    j - 1] is the tag byte of cell (i, j) (gotoh_tags' m x n plane with i0 = 1, or a window of bottom rows).  The walk
    starts at (m, n) in the table the end rule picks from fin = (T1, T2, T3)(m, n) -- the largest, T1 before T2 before
    T3 --, writes one op per step for the table the step leaves ('M' T1, 'D' T2, 'I' T3), moves diagonally out of T1,
    left out of T2 and up out of T3 into the table that cell's tag names, and stops at i == 0 or j == 0."""
    t1, t2, t3 = fin
    ct = 1 if (t1 >= t2 and t1 >= t3) else (2 if (t2 >= t1 and t2 >= t3) else 3)
    i, j = m, n
    ops = bytearray()
    while i > 0 and j > 0:
        if i < i0:
            raise ValueError(f"the walk leaves the tag rows at {(i, j)}")
        ops += b"MDI"[ct - 1:ct]
        tag = (int(tags[i - i0][j - 1]) >> (2 * (ct - 1))) & 3
        assert 1 <= tag <= 3, (i, j, tag)
        if ct != 2:
            i -= 1
        if ct != 3:
            j -= 1
        ct = 4 - tag
    return bytes(ops), (i, j)


def gotoh_rescore(A: bytes, B: bytes, ops: bytes, g, h):
    """The value of the global alignment the ops (end -> start, from (m, n)) describe under (g, h): f per 'M', -g per
    gap symbol, -h more where a gap symbol's predecessor is another table -- the next op's, or after the last op the
    one table that is finite at the border cell the walk stopped at (T1 at (0, 0), T2 on row 0, T3 on column 0),
    whose border value is added."""
    i, j = len(A), len(B)
    total = 0
    for k in range(len(ops)):
        ct = b"MDI".index(ops[k:k + 1]) + 1
        assert i > 0 and j > 0
        if ct == 1:
            total += 1 if A[i - 1] == B[j - 1] else 0
        if ct != 2:
            i -= 1
        if ct != 3:
            j -= 1
        if k + 1 < len(ops):
            nt = b"MDI".index(ops[k + 1:k + 2]) + 1
        else:
            nt = 1 if (i, j) == (0, 0) else (2 if i == 0 else 3)
        if ct != 1:
            total -= g + (h if nt != ct else 0)
    assert i == 0 or j == 0, (i, j)
    return total - (0 if (i, j) == (0, 0) else h + g * max(i, j))


def _less(x, c):
    """x - c, with -inf staying -inf."""
    return np.where(x <= _NEGH, NEG, x - c)


def _first(c):
    return (3 - np.argmax(np.stack(c), axis=0)).astype(np.uint8)


def gotoh_stream(A: bytes, B: bytes, g: int, h: int, windows=()) -> dict:
    """dict(fin, rows): the Gotoh recurrence (start type -1) one row at a time.  fin = (T1, T2, T3)(m, n);
    rows[(lo, hi)] = the tag bytes of rows lo..hi (1-based, inclusive), shape (hi - lo + 1, n).  T1 and T3 of a row
    come from the row above alone; T2(i,j) = max over k < j of max(T1, T3)(i,k) - g - h - (j-1-k) g is a prefix
    maximum (a T2 cell's own T2 predecessor unrolls into the T1 / T3 cell its gap opened from)."""
    a, b = codes(A), codes(B)
    m, n = len(a), len(b)
    kg = np.arange(n + 1, dtype=np.int64) * g
    T1p = np.full(n + 1, NEG, dtype=np.int64)
    T1p[0] = 0
    T2p = -h - kg
    T2p[0] = NEG
    T3p = np.full(n + 1, NEG, dtype=np.int64)
    T1 = np.full(n + 1, NEG, dtype=np.int64)
    T3 = np.full(n + 1, NEG, dtype=np.int64)
    T2 = np.full(n + 1, NEG, dtype=np.int64)
    out = {w: np.zeros((w[1] - w[0] + 1, n), dtype=np.uint8) for w in windows}
    for i in range(1, m + 1):
        d = (T1p[:-1], T2p[:-1], T3p[:-1])
        mx = np.maximum(np.maximum(d[0], d[1]), d[2])
        T1[1:] = np.where(mx <= _NEGH, NEG, mx + (b == a[i - 1]))
        u = (_less(T1p[1:], g + h), _less(T2p[1:], g + h), _less(T3p[1:], g))
        T3[1:] = np.maximum(np.maximum(u[0], u[1]), u[2])
        T3[0] = -h - g * i
        c = np.maximum.accumulate(_less(np.maximum(T1, T3), g + h) + kg)
        v = c[:-1] - kg[:-1]
        T2[1:] = np.where(v <= _NEGH, NEG, v)
        for (lo, hi), rows in out.items():
            if lo <= i <= hi:
                e = (_less(T1[:-1], g + h), _less(T2[:-1], g), _less(T3[:-1], g + h))
                rows[i - lo] = _first(d) | (_first(e) << 2) | (_first(u) << 4)
        T1p, T1 = T1, T1p
        T2p, T2 = T2, T2p
        T3p, T3 = T3, T3p
        T1[0] = T2[0] = NEG
    return dict(fin=(int(T1p[n]), int(T2p[n]), int(T3p[n])), rows=out)


# ---- the flow kernels' stripe arithmetic (msa_flow.hip: fl_cs, fl_P, fl_dq, fl_bmax; two rows per lane) ----------
FL_PS, FL_PS_FILL = 8, 32   # phases per pass-2 segment: inside the flow launch / in the launch of its own


def fl_cs(k: int) -> int:
    return -((16 - (k & 15)) & 15)


def fl_P(k: int, m: int, n: int) -> int:
    rlast = min((m - 128 * k - 1) // 2, 63)
    return (n - fl_cs(k) + rlast) // 16 + 1


def fl_dq(kc: int) -> int:
    return 4 - (fl_cs(kc - 1) + 1 - fl_cs(kc)) // 16


def fl_bmax(kc: int, m: int, n: int) -> int:
    return fl_P(kc - 1, m, n) - 1 - fl_dq(kc)


def n_stripes(m: int) -> int:
    return (m + 127) // 128


def stripe_class(k: int, m: int, n: int) -> dict:
    """How pass 1 runs stripe k of an m x n pair: P phases; "head" (phases 0..5 keep the column-0 border, the rest
    run unmasked up to the producer's last block) when qa = min(P, Bin) >= 6, else "short" (every phase masked both
    ways); segs = the stripe's 8-phase pass-2 segments."""
    P = fl_P(k, m, n)
    Bin = P - 1 if k == 0 else min(P - 1, fl_bmax(k, m, n))
    qa = max(0, min(P, Bin))
    return dict(P=P, Bin=Bin, path="head" if qa >= 6 else "short", segs=(P + FL_PS - 1) // FL_PS, dq=fl_dq(k) if k else 0)


def locate(i: int, j: int) -> tuple:
    """(stripe, phase, lane) of cell (i, j) in the two-rows-per-lane flow layout."""
    s, lane = (i - 1) // 128, ((i - 1) % 128) // 2
    return s, (j - fl_cs(s) + lane) // 16, lane


def first_bad(got, want, i0: int = 1, limit: int = 6) -> list:
    """[(i, j, got, want, stripe, phase, lane)] of the first differing cells of two planes whose [0, 0] is (i0, 1)."""
    return [(int(r) + i0, int(c) + 1, int(got[r, c]), int(want[r, c]), *locate(int(r) + i0, int(c) + 1))
            for r, c in np.argwhere(got != want)[:limit]]


def fill_launch_min_m(ncu: int):
    """The smallest m whose plan runs pass 2 as a launch of its own (shape_flow, msa_plan.inc): pass 1 takes 8 x
    min(ceil(items / 8), CUs per XCD) workgroups, and the separate launch is chosen when that exceeds half the CUs;
    an item is 4 stripes of 128 rows.  65,537 on 256 CUs.  None where no m does."""
    per_xcd = max(1, ncu // 8)
    chunk = (ncu // 2) // 8 + 1
    if chunk > per_xcd:
        return None
    items = 8 * (chunk - 1) + 1
    return 128 * 4 * (items - 1) + 1


# ---- inputs ------------------------------------------------------------------------------------------------------
GAP_LEN = 8   # symbols of a planted insert: rows (columns) at - 3 .. at + 4 around the boundary at | at + 1
GAP_ARM = 48  # at most this many equal symbols on either side of it


def gap_room(kind: str, m: int, n: int) -> bool:
    """Whether the shape has room for the kind's insert with at least 16 equal symbols on either side."""
    if kind == "gaps_a128":
        return m >= 128 + 4 + 16 and n >= 32
    if kind == "gaps_a512":
        return m >= 512 + 4 + 16 and n >= 32
    if kind == "gaps_b128":
        return n >= 128 + 4 + 16 and m >= 140
    return True


def _gaps(rng, m: int, n: int, at: int, in_a: bool):
    """The insert in U (A if in_a, else B) straddling U's positions at | at + 1: U = random + X + Z + Y + random over
    A, C, G with Z at positions at - 3 .. at + 4, and V = T.. + X + Y + T.., X and Y of up to GAP_ARM symbols.  V's
    flanks match nothing in U, so X against X and Y against Y are the only matches a global alignment can make, and
    the gap between them is part of every optimal walk, local or global."""
    lu, lv = (m, n) if in_a else (n, m)
    arm = max(1, min(GAP_ARM, lv // 2, lu - at - 4, at - 4))
    acg = _SYM[:3]
    X, Y, Z = (rng.choice(acg, k).tobytes() for k in (arm, arm, GAP_LEN))
    u0 = at - 4 - arm                      # symbols of U before X
    U = rng.choice(acg, u0).tobytes() + X + Z + Y
    U += rng.choice(acg, lu - len(U)).tobytes()
    v0 = min(max(0, lv - 2 * arm), u0)     # V's equal part starts no later than U's
    V = b"T" * v0 + X + Y
    V += b"T" * (lv - len(V))
    assert (len(U), len(V)) == (lu, lv)
    return (U, V) if in_a else (V, U)


KINDS = ["random", "equal", "mismatch", "periodic", "gaps_a128", "gaps_a512", "gaps_b128"]


@functools.lru_cache(maxsize=None)
def pair_of(kind: str, m: int, n: int, salt: int = 0):
    """(A, B) of a kind, seeded by (kind, m, n, salt):
    random; equal -- one sequence cut to m and to n (the long diagonal, the largest values on the links); mismatch --
    A... against C... (everything at the floor or border); periodic -- ACGT... against CGTA... (ties between the three
    sources); gaps_a128 / gaps_a512 -- A = .. X Z Y .. against B = .. X Y .., the 8 rows of Z straddling rows 128 | 129
    (a stripe link) or 512 | 513 (an item boundary): a vertical gap across them; gaps_b128 -- the mirror image, the
    insert in B straddling columns 128 | 129 (a pass-2 segment restart of stripe 0): a horizontal gap."""
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{m}/{n}/{salt}".encode()))
    if kind == "random":
        return rs(rng, m), rs(rng, n)
    if kind == "equal":
        s = rs(rng, max(m, n))
        return s[:m], s[:n]
    if kind == "mismatch":
        return b"A" * m, b"C" * n
    if kind == "periodic":
        return (b"ACGT" * (m // 4 + 1))[:m], (b"CGTA" * (n // 4 + 1))[:n]
    if kind in ("gaps_a128", "gaps_a512"):
        assert gap_room(kind, m, n)
        return _gaps(rng, m, n, int(kind[6:]), True)
    if kind == "gaps_b128":
        assert gap_room(kind, m, n)
        return _gaps(rng, m, n, 128, False)
    raise KeyError(kind)


def kinds_for(m: int, n: int) -> list:
    """The input kinds of a shape: the gaps kinds only where the shape has room (m >= 148 at the least)."""
    return [k for k in KINDS if gap_room(k, m, n)]


TALL_N = 460  # every full stripe of the tall pair has 33 or 34 phases: a second 32-phase segment


@functools.lru_cache(maxsize=None)
def tall_pair(m: int, n: int = TALL_N, salt: int = 0):
    """A random A of m symbols and B = its last ~n symbols with a fifteenth redrawn and a dozen short indels, cut or
    padded at the front to n: the walk from the end climbs the last stripes."""
    rng = np.random.default_rng(4600 + salt)
    A = rs(rng, m)
    b = bytearray(A[m - n:])
    for k in rng.choice(len(b), size=len(b) // 15, replace=False):
        b[k] = _SYM[rng.integers(4)]
    for k in sorted(rng.choice(len(b) - 8, size=12, replace=False), reverse=True):
        if rng.integers(2):
            del b[k:k + int(rng.integers(1, 5))]
        else:
            b[k:k] = rs(rng, int(rng.integers(1, 5)))
    b = bytes(b)
    B = b[len(b) - n:] if len(b) >= n else rs(rng, n - len(b)) + b
    return A, B


# ---- shapes and scorings -----------------------------------------------------------------------------------------
MS = [1, 2, 127, 128, 129, 257, 513, 640, 2200]
NS = [1, 16, 17, 32, 33, 64, 65, 80, 81, 97, 192, 193, 300]
# every m at n = 33 (stripe 0 on the head path, every later stripe on the short one) and at n = 81 (stripes >= 1 on
# the head path), the 8 | 9 and 16 | 17 phase pairs of stripe 0, and the rest of the n on either side of m
SHAPES = [(m, 33) for m in MS] + [(m, 81) for m in MS] + [
    (1, 97), (129, 64), (129, 65), (257, 192), (257, 193), (513, 17), (640, 300), (2200, 300),
    (2, 1), (127, 16), (129, 32), (257, 80), (128, 300), (513, 193)]
REUSE_SHAPE = (513, 193)

# (match, mismatch, gap_open, gap_extend): the benched floor-less instantiation; the floor in every step; zero gap
# costs (the most ties); the profile bytes at the int8 bound
SW_SCORINGS = [(1, 0, 3, 1), (2, -3, 5, 2), (3, -2, 0, 0), (100, -128, 20, 7)]
GOTOH_GH = [(1, 2), (1, 0), (3, 5), (15, 1)]
# the scoring under which the CPU test looks for the planted gaps in the optimal walks
GAP_SW_SCORING, GAP_GH = (2, -3, 5, 2), (1, 2)
PER_SCORING = 4  # input kinds per (shape, scoring) at the most


def case_kinds(shape, ci: int) -> list:
    """The input kinds of a shape under scoring number ci: all of them where the shape has no more than PER_SCORING,
    else PER_SCORING consecutive ones, starting one further per scoring (and per shape), so that the four scorings
    together use every kind of the shape (at most 7: four windows of four cover them)."""
    ks = kinds_for(*shape)
    x = SHAPES.index(shape) + ci
    return [ks[(x + t) % len(ks)] for t in range(min(PER_SCORING, len(ks)))]


def cases(shape, scorings) -> list:
    """[(scoring, kind)] of a shape."""
    return [(sc, kind) for ci, sc in enumerate(scorings) for kind in case_kinds(shape, ci)]


@functools.lru_cache(maxsize=None)
def sw_case(kind: str, m: int, n: int, scoring, salt: int = 0):
    """(A, B, reference) of one SW-affine case; computed once, never modified."""
    A, B = pair_of(kind, m, n, salt)
    return A, B, sw_reference(A, B, scoring)


def ops_runs(ops: bytes, m_end, letter: bytes) -> list:
    """[(lo, hi)]: the rows ('I') or columns ('D') each run of the letter consumes in ops (end -> start) that start at
    the cell m_end = (i, j)."""
    i, j = m_end
    runs, cur = [], None
    for k in range(len(ops)):
        op = ops[k:k + 1]
        pos = i if letter == b"I" else j
        if op == letter:
            cur = (pos, cur[1]) if cur else (pos, pos)
        elif cur:
            runs.append(cur)
            cur = None
        if op != b"D":
            i -= 1
        if op != b"I":
            j -= 1
    if cur:
        runs.append(cur)
    return runs
