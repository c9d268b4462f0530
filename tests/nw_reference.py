"""Banded global (Gotoh) alignment with direction bytes, restated in numpy: the yardstick of the NW_ALIGN tests.

Not a test file.  The recurrence, byte format and walk are the ones include/msa.h documents for
msa_plan_traceback_nw (f = 1 on equal symbols else 0, g = gap extension, h = gap open - extension >= 0,
open = g + h; cells with |i - j| > band are -inf in all three states):

    H(0,0) = 0, H(0,j) = -h - g j (1 <= j <= band), H(i,0) = -h - g i (1 <= i <= band), E(i,0) = F(0,j) = -inf
    E(i,j) = max(H(i,j-1) - open, E(i,j-1) - g)        F(i,j) = max(H(i-1,j) - open, F(i-1,j) - g)
    H(i,j) = max(H(i-1,j-1) + f, E(i,j), F(i,j))       score = H(m,n)

Rows are vectorised: F and the diagonal term are elementwise in the row above; with X = max(diag, F) and
Y(k) = X(k) + g k, E(i,j) = max_{k<j} Y(k) - open - g (j - 1) is a prefix maximum (going through E(i,k) and
opening again never beats extending, because h >= 0).  The byte's bits are derived from the final values.

All per-cell arrays are in BAND FORM: shape (m+1, 2w+1), entry [i, d] is cell (i, j = i - w + d); w = band, or
max(m, n) when there is no band.  `to_band` brings a row-major (m+1) x (n+1) matrix into that form.
"""
from __future__ import annotations

import numpy as np

NEG = -(1 << 40)  # -inf; anything below NEG // 2 is -inf (it may have drifted by a few gap costs)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rs(rng, n: int) -> bytes:
    return rng.choice(ACGT, n).tobytes()


def similar(rng, m: int, sub=0.02, indel=0.002):
    """A random A and B = A with substitutions and short indels (length ~m)."""
    A = rs(rng, m)
    b = bytearray(A)
    for k in rng.choice(m, size=int(m * sub), replace=False):
        b[k] = ACGT[rng.integers(4)]
    for k in sorted(rng.choice(m - 16, size=int(m * indel), replace=False), reverse=True):
        if rng.integers(2):
            del b[k:k + int(rng.integers(1, 8))]
        else:
            b[k:k] = rs(rng, int(rng.integers(1, 8)))
    return A, bytes(b)


def band_width(m: int, n: int, band: int) -> int:
    return max(m, n) if band < 0 else band


def band_cols(m: int, n: int, w: int):
    """(j, valid): the column of every band-form entry and whether it is an in-band interior cell."""
    i = np.arange(m + 1)[:, None]
    j = i - w + np.arange(2 * w + 1)[None, :]
    return j, (i >= 1) & (j >= 1) & (j <= n)


def to_band(full: np.ndarray, w: int, fill=0) -> np.ndarray:
    """Band form of a row-major (m+1) x (n+1) matrix (entries outside the matrix = fill)."""
    m, n = full.shape[0] - 1, full.shape[1] - 1
    j, _ = band_cols(m, n, w)
    ok = (j >= 0) & (j <= n)
    out = np.full(j.shape, fill, dtype=full.dtype)
    ii = np.broadcast_to(np.arange(m + 1)[:, None], j.shape)
    out[ok] = full[ii[ok], j[ok]]
    return out


def nw_reference(A: bytes, B: bytes, g: int, h: int, band: int = -1, walk=True) -> dict:
    """dict(score, w, H, byte, efin, ffin, valid [, ops, stop]): H int64 (NEG = -inf), byte uint8, efin / ffin =
    "E / F is finite" (bits 2 / 3 mean nothing elsewhere), valid = in-band interior cells -- all in band form;
    ops = the complete ops end -> start (the walk's, then the border gap), stop = the border cell where the walk
    stopped."""
    assert g >= 0 and h >= 0
    a = np.frombuffer(A, dtype=np.uint8)
    b = np.frombuffer(B, dtype=np.uint8)
    m, n = len(a), len(b)
    w = band_width(m, n, band)
    assert abs(m - n) <= w
    op = g + h
    W = 2 * w + 1
    H = np.full((m + 1, W), NEG, dtype=np.int64)
    byte = np.zeros((m + 1, W), dtype=np.uint8)
    efin = np.zeros((m + 1, W), dtype=bool)
    ffin = np.zeros((m + 1, W), dtype=bool)
    # rows as absolute-column arrays (n + 1), -inf outside the row's band
    Hp = np.full(n + 1, NEG, dtype=np.int64)
    Fp = np.full(n + 1, NEG, dtype=np.int64)
    Hp[0] = 0
    jb = np.arange(1, min(n, w) + 1)
    Hp[jb] = -h - g * jb
    H[0, w - 0 + np.arange(0, min(n, w) + 1)] = Hp[:min(n, w) + 1]
    for i in range(1, m + 1):
        jlo, jhi = max(1, i - w), min(n, i + w)
        js = np.arange(jlo, jhi + 1)
        diag = Hp[js - 1] + (b[js - 1] == a[i - 1])
        F = np.maximum(Hp[js] - op, Fp[js] - g)
        X = np.maximum(diag, F)
        # the left neighbour of the row's first cell: the border column 0 (rows <= band), else out of band
        left0 = -h - g * i if (jlo == 1 and i <= w) else NEG
        Y = np.concatenate(([left0 + g * (jlo - 1)], X[:-1] + g * js[:-1]))
        E = np.maximum.accumulate(Y) - op - g * (js - 1)
        Hc = np.maximum(X, E)
        Hl = np.concatenate(([left0], Hc[:-1]))  # H(i, j-1)
        for v in (diag, E, F, Hc, Hl):
            v[v < NEG // 2] = NEG
        lo = np.where(Hc == diag, 1, np.where(Hc == E, 2, 3)).astype(np.uint8)
        bt = lo | (((E == Hl - op) & (Hl > NEG // 2)).astype(np.uint8) << 2) | \
            (((F == Hp[js] - op) & (Hp[js] > NEG // 2)).astype(np.uint8) << 3)
        d = js - i + w
        H[i, d] = Hc
        byte[i, d] = bt
        efin[i, d] = E > NEG // 2
        ffin[i, d] = F > NEG // 2
        Hn = np.full(n + 1, NEG, dtype=np.int64)
        Fn = np.full(n + 1, NEG, dtype=np.int64)
        Hn[js] = Hc
        Fn[js] = F
        if i <= w:
            Hn[0] = -h - g * i
        Hp, Fp = Hn, Fn
    _, valid = band_cols(m, n, w)
    out = dict(score=int(H[m, n - m + w]), w=w, H=H, byte=byte, efin=efin, ffin=ffin, valid=valid)
    if walk:
        out["ops"], out["stop"] = walk_bytes(byte, m, n, w)
    return out


def walk_bytes(byte: np.ndarray, m: int, n: int, w: int):
    """The walk of msa_plan_traceback_nw over band-form bytes: (complete ops end -> start, stop cell)."""
    i, j, st = m, n, 0
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
    stop = (i, j)
    ops += b"I" * i + b"D" * j
    return bytes(ops), stop


def rescore(A: bytes, B: bytes, ops: bytes, g: int, h: int, band: int = -1) -> int:
    """Score of the alignment `ops` (end -> start) describes; asserts that it consumes exactly m and n, that
    every visited cell has |i - j| <= band, and charges every gap run of length L h + g L."""
    a = np.frombuffer(A, dtype=np.uint8)
    b = np.frombuffer(B, dtype=np.uint8)
    o = np.frombuffer(ops, dtype=np.uint8)[::-1]  # start -> end
    assert np.isin(o, np.frombuffer(b"MID", dtype=np.uint8)).all()
    isM, isI, isD = o == ord("M"), o == ord("I"), o == ord("D")
    i = np.cumsum(isM | isI)
    j = np.cumsum(isM | isD)
    assert (i[-1] if len(o) else 0) == len(a) and (j[-1] if len(o) else 0) == len(b), "ops do not consume (m, n)"
    if band >= 0:
        assert int(np.abs(i - j).max(initial=0)) <= band, "the path leaves the band"
    matches = int((a[i[isM] - 1] == b[j[isM] - 1]).sum())
    gap = ~isM
    runs = int((gap & np.concatenate(([True], o[1:] != o[:-1]))).sum())
    return matches - g * int(gap.sum()) - h * runs


def digest_h(H: np.ndarray, n: int, w: int) -> int:
    """The oracle's order-independent digest (orc_checksum_h) of the in-band interior cells of a band-form H."""
    m = H.shape[0] - 1
    j, valid = band_cols(m, n, w)
    i = np.broadcast_to(np.arange(m + 1)[:, None], j.shape)
    with np.errstate(over="ignore"):
        x = (i[valid].astype(np.uint64) << np.uint64(32)) | j[valid].astype(np.uint64)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = (x ^ (x >> np.uint64(31))) | np.uint64(1)
        v = (H[valid] & 0xFFFFFFFF).astype(np.uint64)
        return int((x * v).sum(dtype=np.uint64))


def cigar_of(ops_end_to_start: bytes) -> str:
    out, k = [], len(ops_end_to_start) - 1
    while k >= 0:
        c, run = ops_end_to_start[k], 0
        while k >= 0 and ops_end_to_start[k] == c:
            run += 1
            k -= 1
        out.append(f"{run}{chr(c)}")
    return "".join(out)


# ---- the shapes both test files use: name -> (A, B, band, g, h) -------------------------------------
def _rnd(seed, m, n):
    rng = np.random.default_rng(seed)
    return rs(rng, m), rs(rng, n)


def _sim(seed, m, n=None):
    A, B = similar(np.random.default_rng(seed), m)
    return A, (B if n is None else B[:n])


def _chunked_input(kind, m, w):
    """The inputs of test_gpu_parity.py::test_banded_chunked."""
    rng = np.random.default_rng(m + w)
    A, B = (rs(rng, m), rs(rng, m + 37)) if kind == "random" else similar(rng, m)
    if abs(len(A) - len(B)) > w:
        B = B[:len(A) + w // 2]
    return A, B


def _border(mirror):
    X = rs(np.random.default_rng(4025), 400)
    return (X[25:], X) if mirror else (X, X[25:])


SMALL = {
    # band_kernel, exact chain
    "similar_1000_w64": lambda: _sim(11, 1000) + (64, 1, 2),
    "random_1000x1030_w64": lambda: _rnd(12, 1000, 1030) + (64, 1, 2),
    "random_300x290_w32": lambda: _rnd(13, 300, 290) + (32, 1, 2),
    "random_65x70_w8": lambda: _rnd(14, 65, 70) + (8, 1, 2),
    "random_193x193_w64": lambda: _rnd(15, 193, 193) + (64, 1, 2),
    "random_700x700_w1": lambda: _rnd(16, 700, 700) + (1, 1, 2),
    "ties_A400_A390_w16": lambda: (b"A" * 400, b"A" * 390, 16, 1, 2),
    "ties_A300_C300_w16": lambda: (b"A" * 300, b"C" * 300, 16, 1, 2),
    "border_25I_w40": lambda: _border(False) + (40, 1, 2),
    "border_25D_w40": lambda: _border(True) + (40, 1, 2),
    "random_300x290_w32_g2h0": lambda: _rnd(13, 300, 290) + (32, 2, 0),
    "random_300x290_w32_g0h3": lambda: _rnd(13, 300, 290) + (32, 0, 3),
    # stripe_kernel, one pair without a band
    "random_500x480_noband": lambda: _rnd(17, 500, 480) + (-1, 1, 2),
    "similar_500x480_noband": lambda: _sim(18, 500, 480) + (-1, 1, 2),
}
BAND_EXACT = [k for k in SMALL if "noband" not in k]
NOBAND = [k for k in SMALL if "noband" in k]
# band_kernel, chunked: (kind, m, band) of test_banded_chunked
CHUNKED = {"similar_9001_w64": ("similar", 9001, 64), "random_12000_w512": ("random", 12000, 512)}
# a batch for the stripe kernel: rows, columns
BATCH_MS, BATCH_NS = [200, 150, 77], [180, 200, 90]


def batch_pairs():
    rng = np.random.default_rng(19)
    return [(rs(rng, m), rs(rng, n)) for m, n in zip(BATCH_MS, BATCH_NS)]


# ... and one whose middle stripes lie a full stripe away from the matrix borders with band >= 64: the stripe
# kernel's v_writelane edge fix-ups (rows 129..192 of the first pair: 129 - 64 > 1 and 192 + 64 < n)
BATCH_WIDE_MS, BATCH_WIDE_NS, BATCH_WIDE_BAND = [400, 330], [400, 350], 64


def batch_wide_pairs():
    rng = np.random.default_rng(20)
    return [(rs(rng, m), rs(rng, n)) for m, n in zip(BATCH_WIDE_MS, BATCH_WIDE_NS)]


def chunked_case(name):
    kind, m, w = CHUNKED[name]
    return _chunked_input(kind, m, w) + (w, 1, 2)
