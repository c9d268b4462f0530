"""Inputs over a full eight-symbol alphabet, shared by test_alphabet8_inputs.py (CPU) and
test_gpu_full_alphabet.py (GPU).

Not a test file.  Every kernel picks a cell's score as one byte of an 8-byte per-row profile: codes 0-3 index its low
dword, codes 4-7 its high dword.  ACGT inputs reach the low dword only; the inputs here reach both.

A plan-level test hands the kernels enc8()'s codes (the index in AL8).  A host entry that encodes for itself
(msa_encode_pair: main_alignment, Subproblem, the partial entries, msa_nw_align, msa_sw_align) gives A, C, G, T the
codes 0-3 and every other symbol the next free code as it is first seen, A before B: first_seen() restates that map.
"""
from __future__ import annotations

import functools

import numpy as np

AL8 = b"ACGTNRYK"
AL7 = AL8[:7]
_SYM = np.frombuffer(AL8, dtype=np.uint8)

# dense, small range (every entry decides cells of a few hundred rows: test_alphabet8_inputs.py), not symmetric
TABLE8 = np.random.default_rng(0).integers(-3, 5, (8, 8))
G8, H8 = 1, 2
# largest entry 80: band_kernel's profile byte S + 2g + h is 84 under g = 1, h = 2 (fits int8) and 130 under g = 20,
# h = 10 (the plan must take the exact stripe launch)
TABLE8_WIDE = TABLE8 * 20


def rs8(rng, n: int, k: int = 8) -> bytes:
    """n symbols drawn uniformly from the first k of AL8 (one rng.integers call)."""
    return _SYM[rng.integers(0, k, n)].tobytes()


def pair8(seed: int, m: int, n: int, k: int = 8):
    rng = np.random.default_rng(seed)
    A = rs8(rng, m, k)
    return A, rs8(rng, n, k)


def enc8(seq: bytes) -> np.ndarray:
    """The plan-level codes of seq: the index of every symbol in AL8."""
    lut = np.full(256, 255, dtype=np.uint8)
    lut[_SYM] = np.arange(8, dtype=np.uint8)
    c = lut[np.frombuffer(seq, dtype=np.uint8)]
    assert (c < 8).all(), "a symbol outside AL8"
    return c


def first_seen(A: bytes, B: bytes) -> dict:
    """msa_encode_pair's map {symbol byte: code}: ACGT are 0-3, every other symbol gets the next code as it is
    first seen in A, then in B.  More than 8 symbols: ValueError (the entry returns MSA_ERR_ALPHABET)."""
    m = {c: k for k, c in enumerate(b"ACGT")}
    for c in A + B:
        if c not in m:
            if len(m) >= 8:
                raise ValueError("more than 8 symbols")
            m[c] = len(m)
    return m


def as_run(A: bytes, B: bytes):
    """(rows, columns) as Subproblem and main_alignment run a pair: the shorter sequence first (the reference's
    constructor swap), which is also the order in which msa_encode_pair sees them."""
    return (B, A) if len(A) > len(B) else (A, B)


def mutated8(seed: int, m: int, n: int, k: int = 8):
    """A random A and B = A with a tenth of its symbols redrawn and a short insertion or deletion every ~40
    symbols, cut or extended to n columns (long diagonal runs with gaps between them)."""
    rng = np.random.default_rng(seed)
    A = rs8(rng, m, k)
    b = bytearray(A)
    for p in rng.choice(m, size=max(1, m // 10), replace=False):
        b[p] = _SYM[rng.integers(k)]
    for p in sorted(rng.choice(m, size=max(1, m // 40), replace=False), reverse=True):
        if rng.integers(2):
            del b[p:p + int(rng.integers(1, 4))]
        else:
            b[p:p] = rs8(rng, int(rng.integers(1, 4)), k)
    return A, bytes(b[:n]) + rs8(rng, max(0, n - len(b)), k)


@functools.lru_cache(maxsize=None)
def tall_pair8(m: int = 70000, n: int = 300):
    """test_gpu_parity.py's tall pair over eight symbols: B = a piece from deep inside A with a twelfth redrawn."""
    rng = np.random.default_rng(7008)
    A = rs8(rng, m)
    b = bytearray(A[20000:20000 + n])
    for p in rng.choice(n, size=n // 12, replace=False):
        b[p] = _SYM[rng.integers(8)]
    return A, bytes(b)


def batch8(seed: int, ms, ns, k: int = 8):
    """Pairs of the given shapes, drawn from one generator (A before B, pair by pair)."""
    rng = np.random.default_rng(seed)
    out = []
    for m, n in zip(ms, ns):
        A = rs8(rng, m, k)
        out.append((A, rs8(rng, n, k)))
    return out


def similar8(rng, m: int, k: int = 8, sub=0.02, indel=0.002):
    """nw_reference.similar with the letters drawn from the first k of AL8."""
    A = rs8(rng, m, k)
    b = bytearray(A)
    for p in rng.choice(m, size=int(m * sub), replace=False):
        b[p] = _SYM[rng.integers(k)]
    for p in sorted(rng.choice(m - 16, size=int(m * indel), replace=False), reverse=True):
        if rng.integers(2):
            del b[p:p + int(rng.integers(1, 8))]
        else:
            b[p:p] = rs8(rng, int(rng.integers(1, 8)), k)
    return A, bytes(b)


@functools.lru_cache(maxsize=None)
def chunked8(m: int = 9001, w: int = 64):
    """nw_reference's chunked "similar" input (similar_9001_w64) over eight symbols."""
    A, B = similar8(np.random.default_rng(m + w), m)
    if abs(len(A) - len(B)) > w:
        B = B[:len(A) + w // 2]
    return A, B


def permuted(perm, codes=None, S=None):
    """codes mapped through perm, or the table S' with S'[perm[x]][perm[y]] = S[x][y]."""
    perm = np.asarray(perm)
    if codes is not None:
        return perm[codes].astype(np.uint8)
    out = np.empty_like(np.asarray(S))
    out[np.ix_(perm, perm)] = S
    return out


PERMS = [(7, 1, 2, 3, 4, 5, 6, 0), (5, 7, 0, 6, 2, 1, 3, 4)]

# ---- the named inputs of test_gpu_full_alphabet.py ---------------------------------------------------------
# name -> (kind, symbols, maker); kind names the oracle call test_alphabet8_inputs.py perturbs:
#   "sw"     oracle.sw's score or H, linear (2, -1, 1, 1)      "swa"  the same under affine (2, -3, 5, 2)
#   "banded32" / "banded" oracle.banded_ref's score or H (band 32 / none)    "main" oracle.main_alignment_text
#   "tables" oracle.subproblem_tables (start type -1)         "partial" oracle.partial_tables (start / end 1)
# A maker returns one pair, or a list of pairs for a batch (a symbol must then matter in some pair).
# HOST: the 8-symbol inputs whose codes msa_encode_pair hands out (the seeds are the first for which the symbol
# that receives code 7 sits where test_code7_is_handed_out asks).
HOST_SEEDS = {"main_65x66": 102, "main_300x290": 101, "sub_65x70": 101, "sub_129x129": 101, "partial_130x129": 101,
              "nw10_300x290": 101}
# (m, n, whether the entry swaps a pair with m > n before it encodes: as_run)
HOST_SHAPES = {"main_65x66": (65, 66, True), "main_300x290": (300, 290, True), "sub_65x70": (65, 70, True),
               "sub_129x129": (129, 129, True), "partial_130x129": (130, 129, False),
               "nw10_300x290": (300, 290, False)}


def host_pair(name):
    return pair8(HOST_SEEDS[name], *HOST_SHAPES[name][:2])


def host_run_order(name):
    """(rows, columns) in the order the entry encodes and runs them."""
    A, B = host_pair(name)
    return as_run(A, B) if HOST_SHAPES[name][2] else (A, B)


PACKED_SHAPES = [(700, 650), (700, 650), (64, 64), (64, 64), (1, 9), (1, 9), (2000, 1999), (2000, 1999), (130, 7),
                 (130, 7), (333, 1000)]  # test_gpu_parity.py::test_sw_linear_packed_pairs' batch


@functools.lru_cache(maxsize=None)
def packed_batch():
    """(As, B of every couple, a_off, b_off, Bcat): couples (2c, 2c + 1) share sizes and their column sequence."""
    rng = np.random.default_rng(81)
    As, Bs, ao, bo, Bcat = [], [], [], [], b""
    for p, (m, n) in enumerate(PACKED_SHAPES):
        if p % 2 == 0:
            off, B = len(Bcat), rs8(rng, n, 7)
            Bcat += B
        ao.append(sum(len(x) for x in As))
        As.append(B[:m] if (p % 4 == 1 and m <= n) else rs8(rng, m, 7))
        Bs.append(B)
        bo.append(off)
    return As, Bs, ao, bo, Bcat


@functools.lru_cache(maxsize=None)
def split_batch():
    """37 pairs of 1500 x 1400 against one shared B (test_batch_split_pairs' packed batch)."""
    rng = np.random.default_rng(82)
    As = [rs8(rng, 1500, 7) for _ in range(37)]
    return As, rs8(rng, 1400, 7)


INPUTS = {
    "swl_65x100": ("sw", 7, lambda: pair8(61, 65, 100, 7)),
    "swl_130x70": ("sw", 7, lambda: pair8(62, 130, 70, 7)),
    "swl_flow_1500x1203": ("sw", 7, lambda: pair8(63, 1500, 1203, 7)),
    "swl_score_300x1200": ("sw", 7, lambda: pair8(64, 300, 1200, 7)),
    "swl_packed": ("sw", 7, lambda: list(zip(*packed_batch()[:2]))),
    "swl_split": ("sw", 7, lambda: [(a, split_batch()[1]) for a in split_batch()[0]]),
    "swa_65x70": ("swa", 7, lambda: mutated8(65, 65, 70, 7)),
    "swa_300x257": ("swa", 7, lambda: mutated8(66, 300, 257, 7)),
    "swa_batch": ("swa", 7, lambda: [mutated8(67 + p, 130 + 7 * p, 125 + 11 * p, 7) for p in range(3)]),
    "got_65x66": ("tables", 8, lambda: pair8(71, 65, 66)),
    "got_129x700": ("tables", 8, lambda: mutated8(72, 129, 700)),
    "got_tall_70000x300": ("tables", 8, lambda: tall_pair8()),
    "banded_300x290": ("banded32", 8, lambda: pair8(73, 300, 290)),
    "nw_500x480": ("banded", 8, lambda: pair8(74, 500, 480)),
}
_HOST_KIND = {"main": "main", "sub": "tables", "partial": "partial", "nw10": "banded32"}
INPUTS.update({name: (_HOST_KIND[name.split("_")[0]], 8, functools.partial(host_pair, name)) for name in HOST_SHAPES})


@functools.lru_cache(maxsize=None)
def named(name):
    """The input of a name: one (A, B), or a list of pairs; computed once and never modified."""
    return INPUTS[name][2]()


# ---- NW_ALIGN / NW_SCORED edge shapes: (m, n, band) ----------------------------------------------------------
EDGE_SHAPES = [(1, 1, -1), (1, 1, 0), (1, 2, 1), (2, 1, 1), (1, 40, -1), (40, 1, -1), (64, 1, -1), (1, 64, 63),
               (5, 5, 0), (63, 63, 0), (64, 64, 0), (65, 65, 0), (63, 60, 8), (64, 70, 8), (65, 64, 1),
               (128, 128, 16), (129, 127, 2), (70, 6, 64), (7, 70, 63)]
EDGE_GH = [(1, 2), (0, 0), (2, 0), (0, 3)]          # the brute-force check's gap costs
EDGE_EXTRA = [((64, 70, 8), (0, 0)), ((64, 70, 8), (0, 3)), ((1, 40, -1), (0, 0)), ((1, 40, -1), (0, 3))]


def edge_pair(m, n):
    return pair8(5000 + 131 * m + n, m, n)
