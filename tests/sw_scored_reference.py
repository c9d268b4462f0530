"""Local (Smith-Waterman, affine gaps) alignment under a substitution matrix: the yardstick of the MSA_SW_SCORED tests.

Not a test file.  A numpy restatement of the contract include/msa.h states for MSA_SW_SCORED, over any alphabet (up to
32 symbols; the kernels' sentinel code is the library's business, not the contract's) and any integer table S
(S[a][b] = alphabet[a] in A against alphabet[b] in B, it need not be symmetric), gap_open = cost of a gap's first
symbol, gap_extend = of every further one:

    E(i,j) = max(E(i,j-1) - gap_extend, H(i,j-1) - gap_open)        E(i,0) = -inf
    F(i,j) = max(F(i-1,j) - gap_extend, H(i-1,j) - gap_open)        F(0,j) = -inf
    H(i,j) = max(0, H(i-1,j-1) + S[A_i][B_j], E(i,j), F(i,j))       H(i,0) = H(0,j) = 0

The direction byte of cell (i, j): bits 0-1 = 0 if H == 0, else 1 if H equals the diagonal term, else 2 if H == E, else
3; bit 2 iff E(i,j) == H(i,j-1) - gap_open (a tie with the extension goes to "open"); bit 3 the same for F and
H(i-1,j).  The score is the largest H and the end cell the first cell attaining it in row-major order ((0, 0) for a
score of 0).  The walk starts there in state H.  H: byte 0 -> stop; 1 -> 'M', to (i-1, j-1), stop on row or column 0;
2 -> state E; 3 -> state F.  E: 'D', j--, back to H if bit 2.  F: 'I', i--, back to H if bit 3.  beg is the first
aligned cell, (i + 1, j + 1) of the cell the walk stopped at; no walk for a score of 0.

The cells are filled one anti-diagonal at a time (every cell of one depends on the two before it only).
test_sw_scored_reference.py checks all of it against the oracle's orc_sw on match / mismatch tables and against a
plain-Python triple loop on dense asymmetric ones.
"""
from __future__ import annotations

import functools

import numpy as np

import alphabet8 as A8
import wide_reference as W
from wide_reference import cigar_of, codes32  # noqa: F401

NEG = -(1 << 40)


def sw_scored_reference(A: bytes, B: bytes, alphabet: bytes, S, gap_open: int, gap_extend: int, walk=True) -> dict:
    """dict(score, end, H, E, F, byte [, ops (end -> start), beg, cigar]); H, E, F, byte are (m+1) x (n+1), row and
    column 0 being the borders (byte 0 there)."""
    a, b = codes32(A, alphabet), codes32(B, alphabet)
    S = np.asarray(S, dtype=np.int64)
    m, n = len(a), len(b)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    byte = np.zeros((m + 1, n + 1), dtype=np.uint8)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        eo, fo = H[i, j - 1] - gap_open, H[i - 1, j] - gap_open
        e = np.maximum(E[i, j - 1] - gap_extend, eo)
        f = np.maximum(F[i - 1, j] - gap_extend, fo)
        dg = H[i - 1, j - 1] + S[a[i - 1], b[j - 1]]
        h = np.maximum(np.maximum(dg, 0), np.maximum(e, f))
        H[i, j], E[i, j], F[i, j] = h, e, f
        hs = np.where(h == 0, 0, np.where(h == dg, 1, np.where(h == e, 2, 3)))
        byte[i, j] = hs | np.where(e == eo, 4, 0) | np.where(f == fo, 8, 0)
    score = int(H.max())
    end = (0, 0)
    if score > 0:
        k = int(np.argmax(H))  # the first maximum of the flattened, row-major array
        end = (k // (n + 1), k % (n + 1))
    r = dict(score=score, end=end, H=H, E=E, F=F, byte=byte)
    if walk:
        ops, beg = walk_bytes(byte, end) if score > 0 else (b"", (1, 1))
        r.update(ops=ops, beg=beg, cigar=cigar_of(ops))
    return r


def walk_bytes(byte: np.ndarray, end) -> tuple:
    """(ops end -> start, beg) of the walk over direction bytes from `end`."""
    i, j = end
    ops, st = bytearray(), 0
    while True:
        v = int(byte[i, j])
        if st == 0:
            if v & 3 == 0:
                break
            if v & 3 == 1:
                ops += b"M"
                i, j = i - 1, j - 1
                if i == 0 or j == 0:
                    break
            else:
                st = (v & 3) - 1
        elif st == 1:
            ops += b"D"
            st = 0 if v & 4 else 1
            j -= 1
        else:
            ops += b"I"
            st = 0 if v & 8 else 2
            i -= 1
    return bytes(ops), (i + 1, j + 1)


def rescore(A: bytes, B: bytes, beg, ops: bytes, alphabet: bytes, S, gap_open: int, gap_extend: int):
    """(score, end) of the alignment that starts at the 1-based cell `beg` and follows `ops` (given end -> start): the
    sum of S over its 'M's less gap_open for the first and gap_extend for every further symbol of each run of 'D' or
    'I'."""
    a, b = codes32(A, alphabet), codes32(B, alphabet)
    S = np.asarray(S, dtype=np.int64)
    i, j = beg[0] - 1, beg[1] - 1  # symbols consumed so far
    total, prev = 0, b""
    for k in range(len(ops) - 1, -1, -1):
        op = ops[k:k + 1]
        if op == b"M":
            total += int(S[a[i], b[j]])
            i, j = i + 1, j + 1
        else:
            total -= gap_extend if op == prev else gap_open
            if op == b"D":
                j += 1
            else:
                i += 1
        prev = op
    return total, (i, j)


def sw_triple_loop(A: bytes, B: bytes, alphabet: bytes, S, gap_open: int, gap_extend: int):
    """(H, E, F) as lists of Python ints (None = -inf), cell by cell; shares no code with sw_scored_reference."""
    ia = [alphabet.index(bytes([c])) for c in A]
    ib = [alphabet.index(bytes([c])) for c in B]
    S = np.asarray(S).tolist()
    m, n = len(A), len(B)
    H = [[0] * (n + 1) for _ in range(m + 1)]
    E = [[None] * (n + 1) for _ in range(m + 1)]
    F = [[None] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            e = H[i][j - 1] - gap_open
            if E[i][j - 1] is not None and E[i][j - 1] - gap_extend > e:
                e = E[i][j - 1] - gap_extend
            f = H[i - 1][j] - gap_open
            if F[i - 1][j] is not None and F[i - 1][j] - gap_extend > f:
                f = F[i - 1][j] - gap_extend
            E[i][j], F[i][j] = e, f
            H[i][j] = max(0, H[i - 1][j - 1] + S[ia[i - 1]][ib[j - 1]], e, f)
    return H, E, F


# ---- tables and inputs of the MSA_SW_SCORED tests ----------------------------------------------------------------
AL7 = A8.AL7
AL31 = W.AL32[:31]
GO, GE = 5, 2            # gap_open, gap_extend of most cases
T7 = np.asarray(A8.TABLE8[:7, :7], dtype=np.int64)      # dense, asymmetric, in [-3, 4]
T31 = np.asarray(W.table32()[:31, :31], dtype=np.int64)  # dense, asymmetric, in [-11, 17]


def sub8(S) -> np.ndarray:
    """The plan's 8 x 8 int8 table of an n_sym x n_sym matrix, n_sym <= 7 (unused codes, the sentinel's row and column
    included, score 0: the library must ignore the latter)."""
    S = np.asarray(S)
    out = np.zeros((8, 8), dtype=np.int8)
    out[:S.shape[0], :S.shape[1]] = S
    return out


def width(w: int):
    """(alphabet, table, plan table builder) of a code width: 8 -> 7 symbols, 32 -> 31."""
    return (AL7, T7, sub8) if w == 8 else (AL31, T31, W.sub32)


def rs(rng, n: int, alphabet: bytes) -> bytes:
    return W.rs32(rng, n, alphabet)


def homologous(rng, m: int, n: int, alphabet: bytes, frac=0.12):
    """A random A, and B = random flanks around a mutated copy of A's middle third with a short deletion and a short
    insertion: a local alignment with gaps of both kinds."""
    A = rs(rng, m, alphabet)
    core = bytearray(W.mutated(rng, A[m // 3:2 * m // 3], alphabet, frac))
    if len(core) > 24:
        del core[8:10]
        core[18:18] = rs(rng, 3, alphabet)
    core = bytes(core)[:n]
    left = (n - len(core)) // 2
    return A, rs(rng, left, alphabet) + core + rs(rng, n - len(core) - left, alphabet)


@functools.lru_cache(maxsize=None)
def every_cell(w: int):
    """The 330 x 300 pair of the every-cell tests: all 49 / 961 (row code, column code) pairs occur."""
    al = width(w)[0]
    rng = np.random.default_rng(810 + w)
    A, B = homologous(rng, 330, 300, al)
    return A, B


ALL_POS7 = np.asarray(T7) - int(T7.min()) + 1     # every entry >= 1
ALL_POS31 = np.asarray(T31) - int(T31.min()) + 1


@functools.lru_cache(maxsize=None)
def all_positive(w: int):
    """[(A, B)] for 70 x 40 and 40 x 70 under the all-positive table."""
    al = width(w)[0]
    rng = np.random.default_rng(820 + w)
    return [(rs(rng, 70, al), rs(rng, 40, al)), (rs(rng, 40, al), rs(rng, 70, al))]


BATCH = [(600, 150), (77, 90), (1, 40), (64, 64)]


@functools.lru_cache(maxsize=None)
def ragged_batch(w: int):
    """[(A, B)] of BATCH's shapes plus a (30, 50) pair that scores 0 under the table: A is one symbol z repeated, B is
    drawn from the symbols b with S[z][b] <= 0."""
    al, T, _ = width(w)
    rng = np.random.default_rng(830 + w)
    pairs = [homologous(rng, m, n, al) if min(m, n) >= 60 else (rs(rng, m, al), rs(rng, n, al)) for m, n in BATCH]
    z = int(np.argmax((T <= 0).sum(axis=1)))
    cols = bytes(al[b] for b in np.flatnonzero(T[z] <= 0))
    return pairs + [(al[z:z + 1] * 30, rs(rng, 50, cols))]


def planted_table(k: int) -> np.ndarray:
    """T7 / T31 with every entry off the diagonal made <= -1 and the diagonal 4 + code % 3: an exact copy of a query
    is its one best local alignment."""
    S = -np.abs(np.array(T7 if k == 7 else T31)) - 1
    c = np.arange(k)
    S[c, c] = 4 + c % 3
    return S


@functools.lru_cache(maxsize=None)
def planted_twice(w: int):
    """(A, B): a 40-symbol query and a 200-symbol reference that holds it exactly twice, apart: two equal maxima."""
    al = width(w)[0]
    rng = np.random.default_rng(840 + w)
    q = rs(rng, 40, al)
    return q, rs(rng, 30, al) + q + rs(rng, 50, al) + q + rs(rng, 40, al)


def self127(k: int) -> np.ndarray:
    """A k x k table with S[1][1] = 127 and -1 elsewhere."""
    S = np.full((k, k), -1, dtype=np.int64)
    S[1, 1] = 127
    return S


def extreme31():
    """(table, A, B): T31 with S[20][21] = 127 (asymmetric: [21][20] stays) and S[9][9] = -128 at codes >= 8, and a
    40 x 40 pair whose best local alignment takes ten 127s on each side of a 9 / 9 column it must gap round."""
    S = np.array(T31)
    S[20, 21] = 127
    S[9, 9] = -128
    rng = np.random.default_rng(850)
    c = lambda k: AL31[k:k + 1]  # noqa: E731
    A = rs(rng, 9, AL31[:8]) + c(20) * 10 + c(9) + c(20) * 10 + rs(rng, 10, AL31[:8])
    B = rs(rng, 10, AL31[:8]) + c(21) * 10 + c(9) + c(21) * 10 + rs(rng, 9, AL31[:8])
    return S, A, B


@functools.lru_cache(maxsize=None)
def protein_case():
    """(A, B, (a0, a1), (b0, b1)): two homologous 150-residue regions (B's a 5 % mutated copy of A's) inside
    unrelated flanks, over the 20 amino acids; the regions are A[a0:a1] and B[b0:b1]."""
    rng = np.random.default_rng(860)
    core = rs(rng, 150, W.AL20)
    A = rs(rng, 60, W.AL20) + core + rs(rng, 45, W.AL20)
    B = rs(rng, 35, W.AL20) + W.mutated(rng, core, W.AL20, 0.05) + rs(rng, 80, W.AL20)
    return A, B, (60, 210), (35, 185)


PGO, PGE = 11, 1


def gpu_cases():
    """[(name, A, B, alphabet, S, gap_open, gap_extend)]: every input the GPU tests align, for the CPU test that
    rescored ops equal the score."""
    out = []
    for w in (8, 32):
        al, T, _ = width(w)
        k = len(al)
        out.append((f"every_cell{w}", *every_cell(w), al, T, GO, GE))
        P = ALL_POS7 if w == 8 else ALL_POS31
        out += [(f"all_positive{w}_{x}", a, b, al, P, GO, GE) for x, (a, b) in enumerate(all_positive(w))]
        out += [(f"ragged{w}_{x}", a, b, al, T, GO, GE) for x, (a, b) in enumerate(ragged_batch(w))]
        out.append((f"planted{w}", *planted_twice(w), al, planted_table(k), GO, GE))
        for L in (516, 517):
            out.append((f"self127_{w}_{L}", al[1:2] * L, al[1:2] * L, al, self127(k), GO, GE))
    S, A, B = extreme31()
    out.append(("extreme31", A, B, AL31, S, GO, GE))
    A, B, _, _ = protein_case()
    out.append(("protein", A, B, W.AL20, W.protein20(), PGO, PGE))
    return out
