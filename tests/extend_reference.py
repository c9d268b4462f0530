"""Extension (anchored-start, free-end) alignment with direction bytes, restated in numpy: the yardstick of the
NW_EXTEND tests.

Not a test file.  The cells ARE the unbanded global alignment's: H, the bytes and their masks come from
nw_scored_reference.nw_scored_reference (wide_reference.nw_reference32 for more than 8 symbols) unchanged, in
nw_reference's band form with w = max(m, n).  What this file adds is the contract include/msa.h documents at
msa_extend_align: the end cell is the FIRST maximum of H over the interior cells 1 <= i <= m, 1 <= j <= n in row-major
order (the smallest i, then the smallest j); a maximum <= 0 is the empty extension -- score 0, end cell (0, 0), no walk;
the walk is msa_plan_traceback_nw's from the end cell in state H to the first border cell, completed by the global
border gap (i x 'I', else j x 'D': the start is anchored at (0, 0)); and the global score H(m, n) is reported beside it.
"""
from __future__ import annotations

import numpy as np

import alphabet8 as A8
import nw_scored_reference as RS
import wide_reference as WR
from fit_reference import edited
from nw_reference import NEG, rs
from nw_scored_reference import SCORE_SETS, cigar_of, match_mismatch  # noqa: F401


def codes(seq: bytes, alphabet: bytes) -> np.ndarray:
    """The codes of seq's symbols (their indices in alphabet): up to 8 symbols, or up to 32."""
    return WR.codes32(seq, alphabet) if len(alphabet) > 8 else RS.codes(seq, alphabet)


def global_reference(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int, walk=False) -> dict:
    """The unbanded global yardstick's dictionary for up to 32 symbols."""
    fn = WR.nw_reference32 if len(alphabet) > 8 else RS.nw_scored_reference
    return fn(A, B, alphabet, S, g, h, -1, walk)


def extend_reference(A: bytes, B: bytes, alphabet: bytes, S, g: int, h: int) -> dict:
    """dict(score, end, stop, global_score, best, w, H, byte, efin, ffin, valid, walk_ops, ops): end = the end cell
    (a_end, b_end); stop = the border cell where the walk stopped; walk_ops = the walk's own ops end -> start, ops =
    those and the border gap (they consume exactly a_end and b_end); best = the interior maximum itself (<= 0 for an
    empty extension); the per-cell arrays are the global yardstick's own objects."""
    glob = global_reference(A, B, alphabet, S, g, h)
    m, n, w = len(A), len(B), glob["w"]
    assert m >= 1 and n >= 1 and w == max(m, n)
    Hv = np.where(glob["valid"], glob["H"], NEG)
    flat = int(np.argmax(Hv))  # the first maximum of the flattened band form: rows ascend, and within a row columns do
    i, d = divmod(flat, Hv.shape[1])
    best = int(Hv[i, d])
    end = (i, d + i - w)
    assert 1 <= end[0] <= m and 1 <= end[1] <= n and best > NEG // 2
    score = best
    if best <= 0:
        score, end = 0, (0, 0)
    walk_ops, stop = walk_from(glob["byte"], end, w)
    ops = walk_ops + b"I" * stop[0] + b"D" * stop[1]
    return dict(score=score, end=end, stop=stop, global_score=glob["score"], best=best, w=w, H=glob["H"],
                byte=glob["byte"], efin=glob["efin"], ffin=glob["ffin"], valid=glob["valid"], walk_ops=walk_ops, ops=ops)


def walk_from(byte: np.ndarray, end, w: int):
    """msa_plan_traceback_nw's walk over band-form bytes from the end cell in state H, to the first cell with i == 0
    or j == 0: (ops end -> start without the border gap, that cell).  The end cell (0, 0) is no walk."""
    i, j = end
    st = 0
    ops = bytearray()
    while i > 0 and j > 0:
        v = int(byte[i, j - i + w])
        if st == 0:
            lo = v & 3
            assert lo != 0, (i, j)
            if lo == 1:
                ops.append(ord("M"))
                i -= 1
                j -= 1
            else:
                st = lo - 1  # 1: E, 2: F
        elif st == 1:
            ops.append(ord("D"))
            j -= 1
            st = 0 if v & 4 else 1
        else:
            ops.append(ord("I"))
            i -= 1
            st = 0 if v & 8 else 2
    return bytes(ops), (i, j)


def rescore(A: bytes, B: bytes, end, ops: bytes, alphabet: bytes, S, g: int, h: int) -> int:
    """Score of the alignment `ops` (end -> start, border gap included) describes between the prefixes A[:end[0]] and
    B[:end[1]]: S per 'M', h + g L per gap run of length L; asserts that it consumes exactly both.  No ops: 0."""
    assert 0 <= end[0] <= len(A) and 0 <= end[1] <= len(B)
    if not ops:
        assert tuple(end) == (0, 0)
        return 0
    a, b = A[:end[0]], B[:end[1]]
    if len(alphabet) > 8:
        return WR.rescore32(a, b, ops, alphabet, S, g, h)
    return RS.rescore(a, b, ops, alphabet, S, g, h)


# ---- scorings beside nw_scored_reference.SCORE_SETS ("dna": +2 / -3, g = 2, h = 3; "asym"; "unit": +1 / -1, g = 1) --
# gaps are free: both borders are 0 (they tie with the empty extension) and H(i, j) is the longest common subsequence of
# the two prefixes, so a maximum is attained on a whole rectangle of cells: every tie rule at once
ZERO = (b"ACGT", match_mismatch(b"ACGT", 1, -1), 0, 0)


def score_set(name: str):
    return ZERO if name == "zero" else SCORE_SETS[name]


# ---- the named shapes: name -> (score set, (A, B)) ----------------------------------------------------------------
def _rnd(seed, m, n):
    rng = np.random.default_rng(seed)
    return rs(rng, m), rs(rng, n)


def _prefix(seed, L, m, n):
    """A and B share their first L symbols and nothing after them (A goes on with 'A's, B with 'C's): under "dna" the
    only maximum is 2 L at (L, L)."""
    P = rs(np.random.default_rng(seed), L)
    return P + b"A" * (m - L), P + b"C" * (n - L)


def _tie(seed, L, m, n):
    """_prefix with 2 mismatches and 3 matches after the common prefix: under "dna" H(L, L) = H(L + 5, L + 5) = 2 L, the
    two maxima."""
    P = rs(np.random.default_rng(seed), L)
    return P + b"AATGT" + b"A" * (m - L - 5), P + b"CCTGT" + b"C" * (n - L - 5)


def _row_m66():
    """A is B's first 66 symbols, and B goes on with 134 'A's -- the symbol of code 0, which a lane without a row
    (rows 67..128 of the last stripe) holds: along B's diagonal those lanes would see nothing but matches."""
    P = rs(np.random.default_rng(88), 66)
    return P, P + b"A" * 134


def _late_zero():
    """Under ZERO: U (110 symbols without 'A') is A's start and sits behind 2,400 'A's in B; A goes on with 'A's, B
    with 'C's.  The longest common subsequence is U: H = 110 on every cell with i >= 110, j >= 2,510 -- the first of
    them in an unmasked body phase of stripe 1 (row m = 200 is in stripe 3), the same row's later ones up to column n
    = 5,000 in the last, masked phases."""
    U = np.random.default_rng(71).choice(np.frombuffer(b"CGT", dtype=np.uint8), 110).tobytes()
    return U + b"A" * 90, b"A" * 2400 + U + b"C" * 2490


def _single_1000x3000():
    """A's first 700 symbols are an edited copy of B's first 700, the rest is unrelated: one pair over several
    workgroups, the end cell in stripe 10 (the third workgroup's)."""
    rng = np.random.default_rng(72)
    ref = rs(rng, 3000)
    return edited(rng, ref[:700]) + b"A" * 300, ref[:700] + b"C" * 2300


SHAPES = {
    # ---- where the end cell lies
    "first_stripe": ("dna", lambda: _prefix(81, 30, 300, 400)),       # (30, 30); stripes 1..4 hold negative H only
    "middle_stripe": ("dna", lambda: _prefix(82, 150, 300, 400)),     # stripe 2 of 5
    "last_stripe": ("dna", lambda: _prefix(83, 290, 300, 400)),       # stripe 4 of 5
    "row64": ("dna", lambda: _prefix(84, 64, 200, 260)),              # lane 63 of stripe 0
    "row65": ("dna", lambda: _prefix(85, 65, 200, 260)),              # lane 0 of stripe 1
    "row128": ("dna", lambda: _prefix(86, 128, 200, 260)),            # lane 63 of stripe 1
    "row129": ("dna", lambda: _prefix(87, 129, 200, 260)),            # lane 0 of stripe 2
    "row_m66": ("dna", _row_m66),                                     # on row m = 66, in lane 1 of the last stripe
    "col_n": ("dna", lambda: _prefix(89, 90, 200, 90)),               # on column n: the masked tail's last in-range step
    "corner": ("dna", lambda: (rs(np.random.default_rng(90), 150),) * 2),  # (m, n): the global alignment
    "cell_1_1": ("dna", lambda: (b"A" + b"C" * 99, b"A" + b"G" * 149)),    # (1, 1)
    "col_1": ("zero", lambda: (b"C" * 69 + b"A" + b"C" * 30, b"A" + b"G" * 199)),  # (70, 1): column 1, the masked head's
                                                                      # first in-range step; H = 1 on every later cell
    # ---- shape extremes
    "m1": ("dna", lambda: _prefix(91, 1, 1, 200)),                    # a single row: (1, 1) or nothing
    "n1": ("dna", lambda: _prefix(92, 1, 200, 1)),                    # a single column
    "q130_n40": ("dna", lambda: _prefix(93, 35, 130, 40)),            # n < 64
    "m64": ("dna", lambda: _prefix(94, 64, 64, 300)),                 # row m = the last lane of the only stripe
    "m65": ("dna", lambda: _prefix(95, 65, 65, 300)),                 # ... lane 0 of a second stripe
    "m65_random": ("dna", lambda: _rnd(95, 65, 300)),                 # unrelated sequences: nothing positive
    "late_zero": ("zero", _late_zero),                                # many phases; a tie unmasked / masked
    # ---- ties
    "tie_two_stripes": ("dna", lambda: _tie(96, 62, 200, 260)),       # rows 62 and 67: the smaller row wins
    "tie_two_lanes": ("dna", lambda: _tie(97, 30, 200, 260)),         # rows 30 and 35 of one stripe
    "tie_zero_rect": ("zero", lambda: (b"G" * 20 + b"ACGT" * 10 + b"G" * 140, b"T" * 30 + b"ACGT" * 10 + b"T" * 230)),
    # ---- empty and negative
    "all_negative": ("dna", lambda: (b"A" * 70, b"C" * 200)),         # every interior H < 0: the empty extension
    "best_zero": ("unit", lambda: (b"CA" + b"G" * 70, b"GA" + b"C" * 90)),  # the interior maximum is exactly 0: empty
    "zero_borders": ("zero", lambda: (b"A" * 70, b"C" * 200)),        # g = h = 0: borders and every H are 0: empty
    # ---- one pair over several workgroups
    "single_1000x3000": ("dna", _single_1000x3000),
}
# what the definition gives where the answer is known in advance: score, end cell, CIGAR
KNOWN = {
    "first_stripe": (60, (30, 30), "30M"),
    "middle_stripe": (300, (150, 150), "150M"),
    "last_stripe": (580, (290, 290), "290M"),
    "row64": (128, (64, 64), "64M"),
    "row65": (130, (65, 65), "65M"),
    "row128": (256, (128, 128), "128M"),
    "row129": (258, (129, 129), "129M"),
    "row_m66": (132, (66, 66), "66M"),
    "col_n": (180, (90, 90), "90M"),
    "corner": (300, (150, 150), "150M"),
    "cell_1_1": (2, (1, 1), "1M"),
    "col_1": (1, (70, 1), "69I1M"),
    "late_zero": (110, (110, 2510), "2400D110M"),
    "tie_two_stripes": (124, (62, 62), "62M"),
    "tie_two_lanes": (60, (30, 30), "30M"),
    "m1": (2, (1, 1), "1M"),
    "n1": (2, (1, 1), "1M"),
    "q130_n40": (70, (35, 35), "35M"),
    "m64": (128, (64, 64), "64M"),
    "m65": (130, (65, 65), "65M"),
    "m65_random": (0, (0, 0), ""),
    "tie_zero_rect": (40, (60, 70), "20I30D40M"),
    "all_negative": (0, (0, 0), ""),
    "best_zero": (0, (0, 0), ""),
    "zero_borders": (0, (0, 0), ""),
}

# cells that hold the same H as the end cell, later in row-major order: in another stripe, another lane, the same row
TIES = {
    "tie_two_stripes": [(67, 67)],
    "tie_two_lanes": [(35, 35)],
    "tie_zero_rect": [(60, 71), (60, 300), (61, 70), (64, 70), (65, 70), (200, 300)],
    "col_1": [(70, 2), (70, 200), (71, 1), (100, 200)],
    "late_zero": [(110, 2511), (110, 5000), (111, 2510), (200, 5000)],
}

# a batch for one plan: a long extension, a short one, the empty extension, the global alignment, one row
BATCH_MS, BATCH_NS = [200, 150, 64, 77, 1], [700, 200, 300, 77, 50]


def batch_pairs():
    rng = np.random.default_rng(73)
    ref = rs(rng, 700)
    same = rs(rng, 77)
    return [(edited(rng, ref[:180]) + b"A" * 20, ref[:180] + b"C" * 520),
            _prefix(74, 40, 150, 200),
            (b"A" * 64, b"C" * 300),
            (same, same),
            (b"G", b"G" + rs(rng, 49))]


def shared_b_batch():
    """(As, B): five reads against one 300-symbol B -- prefixes of it of three lengths (one edited), a read that has
    nothing in common with its start, and B itself with a tail."""
    rng = np.random.default_rng(75)
    ref = rs(rng, 300)
    other = b"ACGT"[(b"ACGT".index(ref[0]) + 1) % 4:][:1]
    return [ref[:70] + b"A" * 30, edited(rng, ref[:130]), ref[:5], other * 40, ref + rs(rng, 35)], ref


def eight_symbols():
    """(A, B, alphabet, S, g, h): an 8-symbol alphabet under alphabet8's asymmetric dense table; the first 150 symbols
    of both are, up to substitutions, the same, and all eight codes occur in them."""
    rng = np.random.default_rng(76)
    ov = bytearray(A8.rs8(rng, 150))
    ov[40] = ov[41] = ov[100] = A8.AL8[7]
    cp = bytearray(ov)
    for k in range(3, 150, 6):  # (substitutions: the table's off-diagonal, asymmetric entries decide too)
        cp[k] = A8.AL8[(A8.AL8.index(cp[k]) + 3) % 8]
    return bytes(ov) + A8.rs8(rng, 100), bytes(cp) + A8.rs8(rng, 180), A8.AL8, A8.TABLE8, A8.G8, A8.H8


AL24 = WR.AL32[:24]


def protein32(k: int = 0):
    """(A, B, alphabet, S, g, h): 24 symbols under wide_reference.table32's first 24 rows and columns; a 150 x 330
    pair whose first 80 symbols are, up to mutations, the same (k: the seed's offset, for a batch of such pairs)."""
    rng = np.random.default_rng(77 + k)
    ov = WR.rs32(rng, 80, AL24)
    return ov + WR.rs32(rng, 70, AL24), WR.mutated(rng, ov, AL24) + WR.rs32(rng, 250, AL24), AL24, \
        WR.table32()[:24, :24], 2, 9
