"""Alignment of a sequence against a position-specific score profile: the yardstick of the profile tests.

Not a test file.  sw_scored_reference.sw_scored_reference, nw_scored_reference.nw_scored_reference (unbanded) and
fit_reference.fit_reference index their table as S[a[i-1], b[j-1]] already, a = the codes of A.  The references here are
those three functions called with the row lookup replaced by the row INDEX -- a = arange(m), S = the profile, m rows
by len(alphabet) columns -- the way wide_reference replaces `codes`, so recurrence, borders, tie order, byte format, walk
and the returned dictionaries are theirs by construction.  test_profile_reference.py checks them key by key against
the table yardsticks on profiles made from a table, and against `profile_brute`, a plain-Python three-matrix DP with
S(i, j) = P[i][b_j] that shares no code with them.

Gap costs: (go, ge) = the cost of a gap's first and of every further symbol, for every mode (the global yardsticks'
g = ge, h = go - ge).
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np

import fit_reference as FR
import nw_scored_reference as RS
import sw_scored_reference as SS
import wide_reference as W
from wide_reference import cigar_of  # noqa: F401

MODES = ("local", "global", "fit")
GO, GE = 5, 2
AL31, AL32 = W.AL32[:31], W.AL32


def alphabet_of(mode: str) -> bytes:
    """31 symbols for a local alignment (the kernels keep the highest code), 32 otherwise."""
    return AL31 if mode == "local" else AL32


class Rows:
    """The "sequence" on the rows of a profile alignment: positions 0..m-1 of the profile."""

    def __init__(self, m: int):
        self.m = int(m)

    def __len__(self):
        return self.m


def _lookup(seq, alphabet: bytes) -> np.ndarray:
    return np.arange(seq.m, dtype=np.int64) if isinstance(seq, Rows) else W.codes32(seq, alphabet)


@contextlib.contextmanager
def _row_lookup():
    """The yardsticks' symbol lookup replaced for the duration of one call: a Rows object looks up its own indices."""
    saved = (RS.codes, FR.codes, SS.codes32)
    RS.codes = FR.codes = SS.codes32 = _lookup
    try:
        yield
    finally:
        RS.codes, FR.codes, SS.codes32 = saved


def _prof(P, alphabet: bytes) -> np.ndarray:
    P = np.asarray(P, dtype=np.int64)
    assert P.ndim == 2 and P.shape[0] >= 1 and P.shape[1] == len(alphabet)
    return P


def profile_reference(mode: str, P, B: bytes, alphabet: bytes, go: int = GO, ge: int = GE) -> dict:
    """The table yardstick's dictionary for the profile P (m x len(alphabet)) against B: local =
    sw_scored_reference's (score, end, H, E, F, byte, ops, beg, cigar), global = nw_scored_reference's (score, w, H,
    byte, efin, ffin, valid, ops, stop), fit = fit_reference's (the same and end_j, beg_j)."""
    P = _prof(P, alphabet)
    with _row_lookup():
        if mode == "local":
            return SS.sw_scored_reference(Rows(len(P)), B, alphabet, P, go, ge)
        if mode == "global":
            return RS.nw_scored_reference(Rows(len(P)), B, alphabet, P, ge, go - ge)
        assert mode == "fit"
        return FR.fit_reference(Rows(len(P)), B, alphabet, P, ge, go - ge)


def table_reference(mode: str, A: bytes, B: bytes, alphabet: bytes, S, go: int = GO, ge: int = GE) -> dict:
    """The same three yardsticks as they are, for the sequence A under the table S."""
    if mode == "local":
        return SS.sw_scored_reference(A, B, alphabet, S, go, ge)
    if mode == "global":
        return W.nw_reference32(A, B, alphabet, S, ge, go - ge)
    return W.fit_reference32(A, B, alphabet, S, ge, go - ge)


def rescore(mode: str, P, B: bytes, alphabet: bytes, ops: bytes, beg=None, span=None, go: int = GO, ge: int = GE):
    """The ops (end -> start) rescored under the profile: local (needs beg, the 1-based start cell) -> (score, end
    cell); global -> score; fit (needs span = (beg_j, end_j)) -> score."""
    P = _prof(P, alphabet)
    with _row_lookup():
        if mode == "local":
            return SS.rescore(Rows(len(P)), B, beg, ops, alphabet, P, go, ge)
        if mode == "global":
            return RS.rescore(Rows(len(P)), B, ops, alphabet, P, ge, go - ge)
        return FR.rescore(Rows(len(P)), B, span[0], span[1], ops, alphabet, P, ge, go - ge)


def result_of(mode: str, ref: dict, m: int, n: int) -> dict:
    """What the host entries and api.profile_align report for a yardstick dictionary: score, beg, end, cigar."""
    if mode == "local":
        return dict(score=ref["score"], beg=ref["beg"], end=ref["end"], cigar=ref["cigar"])
    if mode == "global":
        return dict(score=ref["score"], beg=(0, 0), end=(m, n), cigar=cigar_of(ref["ops"]))
    return dict(score=ref["score"], beg=(0, ref["beg_j"]), end=(m, ref["end_j"]), cigar=cigar_of(ref["ops"]))


def profile_brute(mode: str, P, B: bytes, alphabet: bytes, go: int = GO, ge: int = GE):
    """(H, E, F) as (m+1) x (n+1) lists of Python ints (None = -inf), cell by cell, S(i, j) = P[i-1][code of B_j]:
    E(i,j) = max(H(i,j-1) - go, E(i,j-1) - ge), F(i,j) = max(H(i-1,j) - go, F(i-1,j) - ge), H = max(diagonal + S, E, F
    [, 0: local]).  Borders: local H = 0 all round; global H(0,j) = -(go - ge) - ge j, H(i,0) = F(i,0) = -(go - ge) -
    ge i; fit: the global left border under a zero top border."""
    P = [[int(v) for v in row] for row in np.asarray(P).tolist()]
    b = [alphabet.index(bytes([c])) for c in B]
    m, n, h = len(P), len(b), go - ge
    H = [[None] * (n + 1) for _ in range(m + 1)]
    E = [[None] * (n + 1) for _ in range(m + 1)]
    F = [[None] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, n + 1):
        H[0][j] = -h - ge * j if mode == "global" else 0
    for i in range(1, m + 1):
        if mode == "local":
            H[i][0] = 0
        else:
            H[i][0] = F[i][0] = -h - ge * i
        for j in range(1, n + 1):
            e = H[i][j - 1] - go
            if E[i][j - 1] is not None and E[i][j - 1] - ge > e:
                e = E[i][j - 1] - ge
            f = H[i - 1][j] - go
            if F[i - 1][j] is not None and F[i - 1][j] - ge > f:
                f = F[i - 1][j] - ge
            d = H[i - 1][j - 1] + P[i - 1][b[j - 1]]
            E[i][j], F[i][j] = e, f
            H[i][j] = max(d, e, f, 0) if mode == "local" else max(d, e, f)
    return H, E, F


def pad32(P) -> np.ndarray:
    """The plan's rows x 32 int8 profile of a rows x n_sym one (codes no symbol has score 0)."""
    P = np.asarray(P)
    out = np.zeros((P.shape[0], 32), dtype=np.int8)
    out[:, :P.shape[1]] = P
    return out


# ---- profiles and inputs of the GPU tests (test_profile_reference.py asserts what each is meant to be) ----------
def table_of(mode: str) -> np.ndarray:
    k = len(alphabet_of(mode))
    return W.table32()[:k, :k]


@functools.lru_cache(maxsize=None)
def table_case(mode: str):
    """(A, B): the 330 x 300 pair of the table-equivalence test, a local alignment with gaps of both kinds inside."""
    rng = np.random.default_rng(900 + MODES.index(mode))
    return SS.homologous(rng, 330, 300, alphabet_of(mode))


def specific_profile(seed: int, m: int, k: int, shift=None) -> np.ndarray:
    """m rows over k symbols in a log-odds-like range: background scores in [-4, 1], the row's preferred symbol in
    [5, 11], the last symbol -3 in every row (a sequence of it scores nothing anywhere).  Preferred symbols repeat
    with period 7 over codes 0..k-2, so many positions prefer the same symbol with different rows; in the rows of
    `shift` (a slice) the preferred column is moved up by one."""
    rng = np.random.default_rng(seed)
    P = rng.integers(-4, 2, size=(m, k))
    pref = (np.arange(m) * 5) % 7 + 8 * (np.arange(m) % 3)          # codes in 0..22: below, at and above 8 and 16
    if shift is not None:
        pref[shift] = pref[shift] + 1
    assert pref.max() < k - 1
    P[np.arange(m), pref] = rng.integers(5, 12, size=m)
    P[:, k - 1] = -3
    return P.astype(np.int64)


def consensus(P, alphabet: bytes) -> bytes:
    return bytes(alphabet[c] for c in np.asarray(P).argmax(axis=1))


def sample(rng, P, alphabet: bytes, lo: int, hi: int, frac=0.08) -> bytes:
    """A mutated copy of the consensus of rows [lo, hi) with a two-symbol deletion and a two-symbol insertion (the
    same length again); no symbol is the alphabet's last."""
    al = alphabet[:-1]
    s = bytearray(W.mutated(rng, consensus(P[lo:hi], alphabet), al, frac))
    third = len(s) // 3
    if third >= 12:
        del s[third:third + 2]
        s[2 * third:2 * third] = W.rs32(rng, 2, al)
    return bytes(s)


@functools.lru_cache(maxsize=None)
def specific_case(mode: str):
    """(P, B): 330 position-specific rows, rows 150..179 with the preferred column shifted; B a 300-symbol mutated
    sample of rows 15..314."""
    al = alphabet_of(mode)
    P = specific_profile(910 + MODES.index(mode), 330, len(al), shift=slice(150, 180))
    B = sample(np.random.default_rng(915 + MODES.index(mode)), P, al, 15, 315)
    return P, B


BATCH_ROWS = 580
BATCH_NS = [1, 64, 65, 240, 50]   # the last: the alphabet's last symbol only, nothing positive anywhere


@functools.lru_cache(maxsize=None)
def batch_case(mode: str):
    """(P, [B]): one 580-row profile and BATCH_NS' sequences -- samples of its rows, and one unrelated sequence."""
    al = alphabet_of(mode)
    P = specific_profile(920 + MODES.index(mode), BATCH_ROWS, len(al))
    rng = np.random.default_rng(925 + MODES.index(mode))
    Bs = [sample(rng, P, al, 100, 100 + n) for n in BATCH_NS[:4]] + [al[-1:] * BATCH_NS[4]]
    return P, Bs


SLICES = [(0, 580), (37, 64), (515, 65)]   # (a_off, m): the last ends exactly at the profile's last row


@functools.lru_cache(maxsize=None)
def slice_case(mode: str):
    """(P, [B]): batch_case's profile and one sequence per slice of SLICES, a sample of the slice's own rows."""
    al = alphabet_of(mode)
    P, _ = batch_case(mode)
    rng = np.random.default_rng(930 + MODES.index(mode))
    return P, [sample(rng, P, al, a + m // 8, a + m // 8 + min(m - m // 8, 90)) + W.rs32(rng, 7, al[:-1])
               for a, m in SLICES]


EDGE_MS, EDGE_N = (1, 64, 65), 70


@functools.lru_cache(maxsize=None)
def edge_case(mode: str, m: int):
    al = alphabet_of(mode)
    P = specific_profile(940 + m + MODES.index(mode), m, len(al))
    rng = np.random.default_rng(945 + m)
    core = sample(rng, P, al, 0, min(m, EDGE_N - 10))
    return P, (W.rs32(rng, 5, al[:-1]) + core + W.rs32(rng, EDGE_N, al[:-1]))[:EDGE_N]


@functools.lru_cache(maxsize=None)
def all_positive_case():
    """(P, [B]): 70 rows of scores >= 1 over 31 symbols, against 40 and 90 random symbols."""
    rng = np.random.default_rng(950)
    P = rng.integers(1, 9, size=(70, 31)).astype(np.int64)
    return P, [W.rs32(rng, 40, AL31), W.rs32(rng, 90, AL31)]


def self127(L: int):
    """(P, B): L rows that score 127 against symbol 1 and -1 against the others; B = symbol 1, L times."""
    P = np.full((L, 31), -1, dtype=np.int64)
    P[:, 1] = 127
    return P, AL31[1:2] * L


EXT_ROW0 = 70   # the first extreme row: beyond the first stripe


@functools.lru_cache(maxsize=None)
def extreme_case(mode: str):
    """(P, B, codes): 100 + k - 8 rows; row EXT_ROW0 + t scores 127 against code 8 + t and -128 against the next code
    up (cyclically in 8..k-1), for every code t of 8..k-1 (local: the last symbol's column stays out of B, so its 127
    is not needed there: codes 8..k-2); B follows the 127s with every third symbol replaced by the row's -128 one."""
    al = alphabet_of(mode)
    k = len(al)
    hi = k - 1 if mode == "local" else k          # codes 8 .. hi-1 carry the extremes
    cs = list(range(8, hi))
    m = EXT_ROW0 + len(cs) + 30
    P = specific_profile(960 + MODES.index(mode), m, k)
    b = []
    for t, c in enumerate(cs):
        r = EXT_ROW0 + t
        nxt = cs[(t + 1) % len(cs)]
        P[r, :] = -2
        P[r, c] = 127
        P[r, nxt] = -128
        b.append(nxt if t % 3 == 2 else c)
    rng = np.random.default_rng(965)
    head = sample(rng, P, al, 40, EXT_ROW0)
    tail = sample(rng, P, al, EXT_ROW0 + len(cs), m - 4)
    # (... and every extreme code once more, in falling order: each -128 meets its symbol in cells of its row)
    return P, head + bytes(al[c] for c in b) + bytes(al[c] for c in reversed(cs)) + tail, cs
