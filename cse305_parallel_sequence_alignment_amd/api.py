"""Python mirror of the reference's C++ interface for the hot path.

Same names and argument meanings as the reference headers; every call goes
through libmsa.so's C-ABI into the gfx950 kernels (no CPU fallback; a missing
library or GPU raises ``MsaError`` / ``ImportError``).

Reference interfaces mirrored (D-2n/CSE305_Parallel_Sequence_Alignment):
  main_alignment_function   alignment_algorithm/main_alignment.h:38, .cpp:353-410
  optimal_alignment         main_alignment.h:34, .cpp:158-351 (multi-subproblem stitch)
  Subproblem                alignment_algorithm/subproblem_alignment.h:16-97
  Align                     subproblem_alignment.h:8-13 (``align``)
  findPartialBalancedPartitionParallel  sequence_alignment/partial.h:41, partial.cpp:149-163
  partial tables            partial.h:25-35 (initialize*/fill*Parallel)

Character buffers follow the reference: ``A``/``B`` passed to
``main_alignment_function`` and ``Subproblem`` are 1-based (element 0 is
never read, testing.cpp:124-128); the partial.cpp functions read A[i-1].
"""
from __future__ import annotations

import ctypes as C
import sys
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib as LB


def _buf(x) -> bytes:
    if isinstance(x, str):
        x = x.encode("latin-1")
    return bytes(x)


@dataclass
class Align:
    """``align`` (subproblem_alignment.h:8-13): a path node; ``next`` links the list."""
    i: int
    j: int
    t: int
    next: Optional["Align"] = field(default=None, repr=False)

    def as_tuple(self):
        return (self.i, self.j, self.t)


def _link(nodes: List[Align]) -> Optional[Align]:
    for a, b in zip(nodes, nodes[1:]):
        a.next = b
    return nodes[0] if nodes else None


def main_alignment_text(A: bytes, B: bytes, m: int, n: int, p: int = 32, g: float = 1.0, h: float = 2.0):
    """The exact stdout of ``main_alignment_function`` and the score max(T1,T2,T3)[m][n]."""
    A, B = _buf(A), _buf(B)
    if len(A) < m + 1 or len(B) < n + 1:
        raise ValueError("A/B must be 1-based buffers of at least m+1 / n+1 bytes")
    L = LB.lib()
    need = C.c_size_t()
    score = C.c_double()
    # five progress lines + two alignment lines of at most m+n characters: one call fits
    buf = C.create_string_buffer(64 + 2 * (m + n + 2))
    LB.check(L.msa_main_alignment(A, B, m, n, p, g, h, buf, len(buf), C.byref(need), C.byref(score)),
             "msa_main_alignment")
    return buf.raw[:need.value].decode("latin-1"), score.value


def main_alignment_function(A: bytes, B: bytes, m: int, n: int, p: int, g: float, h: float) -> int:
    """Drop-in for ``int main_alignment_function(char*,char*,size_t,size_t,size_t,double,double)``:
    prints the same lines as the reference and returns 0."""
    text, _ = main_alignment_text(A, B, m, n, p, g, h)
    sys.stdout.write(text)
    sys.stdout.flush()
    return 0


class Subproblem:
    """``class Subproblem`` (subproblem_alignment.h:16-97) backed by the GPU fill.

    After ``compute_tables()`` the public ``T1``, ``T2``, ``T3`` are float64
    (m+1) x (n+1) arrays with ``-inf`` where the reference holds -infinity.
    """

    def __init__(self, A, B, m, n, id_A, id_B, p, start, end, g, h):
        A, B = _buf(A), _buf(B)
        # constructor swap (subproblem_alignment.h:37-54)
        if m <= n:
            self.A, self.B, self.m, self.n, self.id_A, self.id_B, self.invert = A, B, m, n, id_A, id_B, False
        else:
            self.A, self.B, self.m, self.n, self.id_A, self.id_B, self.invert = B, A, n, m, id_B, id_A, True
        self._orig = (A, B, m, n, id_A, id_B)
        self.p = p
        self.start_type = start
        self.end_type = end
        self.g = float(g)
        self.h = float(h)
        self.T1 = self.T2 = self.T3 = None
        self.alignment_begin: Optional[Align] = None
        self.alignment_end: Optional[Align] = None
        self._tables_int = None

    # subproblem_alignment.h:83-88
    def f(self, i: int, j: int) -> float:
        return 1.0 if self.A[self.id_A + i] == self.B[self.id_B + j] else 0.0

    # subproblem_alignment.h:91-96
    def h_prime(self, k: int) -> float:
        return self.h if (k == self.end_type and self.end_type <= -2) else 0.0

    def _call(self, tables: bool, nodes: bool):
        A, B, m, n, ida, idb = self._orig
        L = LB.lib()
        mm, nn = self.m, self.n
        T = [np.empty((mm + 1, nn + 1), dtype=np.int32) for _ in range(3)] if tables else [None] * 3
        cap = (m + n + 2) if nodes else 0
        nd = (LB.Node * max(cap, 1))()
        nn_ = C.c_size_t()
        endn = LB.Node()
        inv = C.c_int()
        tp = [t.ctypes.data_as(C.c_void_p) if t is not None else None for t in T]
        LB.check(L.msa_subproblem(A, B, m, n, ida, idb, self.start_type, self.end_type, self.g, self.h, tp[0], tp[1],
                                  tp[2], nd if nodes else None, cap, C.byref(nn_), C.byref(endn), C.byref(inv)),
                 "msa_subproblem")
        return T, [(nd[k].i, nd[k].j, nd[k].t) for k in range(nn_.value)] if nodes else None, endn

    def compute_tables(self) -> None:
        """subproblem_alignment.cpp:329-355 (the parallel row sweep) -- on the GPU."""
        T, _, _ = self._call(tables=True, nodes=False)
        self._tables_int = T
        conv = lambda t: np.where(t == np.iinfo(np.int32).min, -np.inf, t.astype(np.float64))
        self.T1, self.T2, self.T3 = (conv(t) for t in T)

    def non_parallel_tables_text(self) -> str:
        """The text subproblem_alignment.cpp:401-421 prints, from the GPU tables (msa_non_parallel_tables)."""
        A, B, m, n, ida, idb = self._orig
        L = LB.lib()
        need = C.c_size_t()
        LB.check(L.msa_non_parallel_tables(A, B, m, n, ida, idb, self.start_type, self.end_type, self.g, self.h,
                                           None, 0, C.byref(need)), "msa_non_parallel_tables")
        buf = C.create_string_buffer(need.value + 1)
        LB.check(L.msa_non_parallel_tables(A, B, m, n, ida, idb, self.start_type, self.end_type, self.g, self.h,
                                           buf, need.value + 1, C.byref(need)), "msa_non_parallel_tables")
        return buf.raw[:need.value].decode("latin-1")

    def non_parallel_tables(self) -> None:
        """subproblem_alignment.cpp:357-422: the same tables (GPU fill), printed as the reference does."""
        self.compute_tables()
        sys.stdout.write(self.non_parallel_tables_text())
        sys.stdout.flush()

    def find_alignment(self) -> None:
        """subproblem_alignment.cpp:105-172 (tie order, quirks Q1/Q2 included)."""
        _, nodes, endn = self._call(tables=False, nodes=True)
        objs = [Align(int(i), int(j), int(t)) for (i, j, t) in nodes]
        # the list runs alignment_begin -> ... -> alignment_end (the (m, n) node)
        self.alignment_begin = _link(objs)
        self.alignment_end = objs[-1] if objs else Align(int(endn.i), int(endn.j), int(endn.t))

    def alignment_list(self):
        out, a = [], self.alignment_begin
        while a is not None:
            out.append(a.as_tuple())
            a = a.next
        return out

    def print_alignment(self) -> None:
        """subproblem_alignment.cpp:174-180."""
        for (i, j, t) in self.alignment_list():
            print(f"({i}, {j}, {t})")


def _nodes_in(partial_bp):
    arr = (LB.Node * max(1, len(partial_bp)))()
    for k, a in enumerate(partial_bp):
        i, j, t = a.as_tuple() if isinstance(a, Align) else a
        arr[k].i, arr[k].j, arr[k].t = i, j, t
    return arr


def optimal_alignment_text(A, B, partial_bp, m, n, p=32, g=1.0, h=2.0, fix_all=False):
    """``optimal_alignment`` (main_alignment.cpp:202-351) over the partition ``partial_bp``
    (Align nodes or (i, j, t) tuples): returns (stdout text, stitched path as (i, j, t) tuples).

    fix_all=False keeps the reference's behaviour (2-3 subproblems: only the first is
    solved; the link into the last subproblem is never made, :344-348)."""
    A, B = _buf(A), _buf(B)
    if len(A) < m + 1 or len(B) < n + 1:
        raise ValueError("A/B must be 1-based buffers of at least m+1 / n+1 bytes")
    L = LB.lib()
    bp = _nodes_in(partial_bp)
    fl = 1 if fix_all else 0
    need, npath = C.c_size_t(), C.c_size_t()
    cap = m + n + 2 * len(partial_bp) + 2
    path = (LB.Node * cap)()
    LB.check(L.msa_optimal_alignment(A, B, m, n, p, g, h, bp, len(partial_bp), fl, None, 0, C.byref(need), path,
                                     cap, C.byref(npath)), "msa_optimal_alignment")
    buf = C.create_string_buffer(need.value + 1)
    LB.check(L.msa_optimal_alignment(A, B, m, n, p, g, h, bp, len(partial_bp), fl, buf, need.value + 1,
                                     C.byref(need), None, 0, None), "msa_optimal_alignment")
    nodes = [(int(path[k].i), int(path[k].j), int(path[k].t)) for k in range(npath.value)]
    return buf.raw[:need.value].decode("latin-1"), nodes


def optimal_alignment(A, B, partial_bp, m, n, p, g, h) -> None:
    """Drop-in for ``void optimal_alignment(char*, char*, std::vector<align>, size_t m, size_t n,
    size_t p, double g, double h)``: prints what the reference prints."""
    text, _ = optimal_alignment_text(A, B, partial_bp, m, n, p, g, h)
    sys.stdout.write(text)
    sys.stdout.flush()


def main_alignment_partitioned_text(A, B, m, n, p=4, g=1.0, h=2.0, fix_all=False) -> str:
    """main_alignment_function with its commented-out partition step enabled
    (main_alignment.cpp:365,372): GPU partition -> optimal_alignment."""
    A, B = _buf(A), _buf(B)
    if len(A) < m + 1 or len(B) < n + 1:
        raise ValueError("A/B must be 1-based buffers of at least m+1 / n+1 bytes")
    L = LB.lib()
    need = C.c_size_t()
    fl = 1 if fix_all else 0
    LB.check(L.msa_main_alignment_partitioned(A, B, m, n, p, g, h, fl, None, 0, C.byref(need)),
             "msa_main_alignment_partitioned")
    buf = C.create_string_buffer(need.value + 1)
    LB.check(L.msa_main_alignment_partitioned(A, B, m, n, p, g, h, fl, buf, need.value + 1, C.byref(need)),
             "msa_main_alignment_partitioned")
    return buf.raw[:need.value].decode("latin-1")


def print_seq(A: bytes, B: bytes, begin: Optional[Align]) -> str:
    """main_alignment.cpp:32-55 (returns the two lines instead of printing)."""
    A, B = _buf(A), _buf(B)
    l1, l2 = [], []
    a = begin
    while a is not None:
        l1.append(chr(A[a.i]) if a.t in (1, 3) and a.i < len(A) else ("?" if a.t in (1, 3) else "-"))
        l2.append(chr(B[a.j]) if a.t in (1, 2) and a.j < len(B) else ("?" if a.t in (1, 2) else "-"))
        a = a.next
    return "".join(l1) + "\n" + "".join(l2) + "\n"


def findPartialBalancedPartitionParallel(A, B, m, n, p, g, h, start_type, end_type, partition=None) -> List[Align]:
    """partial.cpp:149-163 (int32 wrap semantics, as the reference's -O0 build)."""
    A, B = _buf(A), _buf(B)
    out = (LB.Node * (p + 2))()
    nout = C.c_size_t()
    LB.check(LB.lib().msa_partial_partition(A, B, m, n, p, g, h, start_type, end_type, out, p + 2, C.byref(nout)),
             "msa_partial_partition")
    res = [Align(int(out[k].i), int(out[k].j), int(out[k].t)) for k in range(nout.value)]
    if partition is not None:
        partition.clear()
        partition.extend(res)
    return res


def partial_tables(A, B, m, n, g, h, start_type, end_type):
    """The six int32 tables partial.cpp builds (T* (m+1)x(n+1), TR* (m+2)x(n+2))."""
    A, B = _buf(A), _buf(B)
    T = [np.empty((m + 1, n + 1), dtype=np.int32) for _ in range(3)]
    R = [np.empty((m + 2, n + 2), dtype=np.int32) for _ in range(3)]
    ptr = [x.ctypes.data_as(C.c_void_p) for x in T + R]
    LB.check(LB.lib().msa_partial_tables(A, B, m, n, g, h, start_type, end_type, *ptr), "msa_partial_tables")
    return T, R


# The alignment calls of the build extension.  LB.KINDS declares each kind once; _align (or _profile_align) and
# _call marshal every one of them, a single pair being a batch of one handed to the single-pair entry.


def _scoring(kind, seqs, match, mismatch, alphabet, matrix, max_symbols):
    """The scoring of one call (``max_symbols`` 8 or 32): None for the kind's plain entry, else (alphabet bytes,
    n_sym x n_sym int8 matrix, row = A's symbol).  ``matrix`` needs ``alphabet`` and excludes ``match`` / ``mismatch``
    (ValueError).  Without one, ``match`` / ``mismatch`` (None: 1 / 0) score the distinct symbols of ``seqs`` in
    first-seen order, at most ``max_symbols`` -- one fewer for a kind whose kernels keep the highest code as the
    out-of-matrix sentinel -- else MsaError with the ALPHABET status.  The plain entries take 8 symbols only: sw's
    whenever there is no matrix (it has ``match`` / ``mismatch`` itself), nw's when nothing is given (+1 / 0)."""
    if matrix is not None:
        if match is not None or mismatch is not None:
            raise ValueError("give either matrix (with alphabet) or match / mismatch, not both")
        if alphabet is None:
            raise ValueError("matrix needs alphabet")
        alphabet = _buf(alphabet)
        S = np.asarray(matrix)
        if S.ndim != 2 or (S != S.astype(np.int8)).any():
            raise ValueError("matrix must be a square array of scores in [-128, 127]")
        # (the library checks the alphabet and that the matrix is n_sym x n_sym before it reads either)
        if S.shape != (len(alphabet), len(alphabet)):
            raise ValueError("matrix must be len(alphabet) x len(alphabet)")
        return alphabet, np.ascontiguousarray(S, dtype=np.int8)
    if alphabet is not None:
        raise ValueError("alphabet comes with matrix")
    if kind.plain is not None and max_symbols == 8 and ("match" in kind.plain
                                                          or (match is None and mismatch is None)):
        return None
    seen = dict.fromkeys(b"".join(seqs))  # first-seen order
    if len(seen) > max_symbols - kind.sentinel:
        raise LB.MsaError(-2, "sw_align" if kind.sentinel else "nw_align")
    ma, mi = (1 if match is None else int(match)), (0 if mismatch is None else int(mismatch))
    if not (-128 <= ma <= 127 and -128 <= mi <= 127):
        raise LB.MsaError(-5, "nw_align")
    k = len(seen)
    S = np.full((k, k), mi, dtype=np.int8)
    np.fill_diagonal(S, ma)
    return bytes(seen), S


def _concat(seqs):
    """(the sequences end to end, their offsets in that buffer, their lengths), the last two as int64 arrays."""
    seqs = [_buf(s) for s in seqs]
    n = np.array([len(s) for s in seqs], dtype=np.int64)
    return b"".join(seqs), np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.int64), n


def _batch_in(As, Bs):
    """(A buffer, B buffer, a_off, m, b_off, n as int64 arrays) of a batch; ``Bs`` one bytes object = shared by
    every pair (sent once)."""
    A, a_off, m = _concat(As)
    if isinstance(Bs, (bytes, bytearray, str, memoryview)):
        B = _buf(Bs)
        n = np.full(len(m), len(B), dtype=np.int64)
        b_off = np.zeros(len(m), dtype=np.int64)
    else:
        B, b_off, n = _concat(Bs)
        if len(n) != len(m):
            raise ValueError("Bs must be as long as As, or one bytes object shared by every pair")
    return A, B, a_off, m, b_off, n


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ref(a, i):
    """A pointer to element ``i`` of the C-contiguous array ``a`` (None: NULL), as ctypes.byref gives one."""
    if a is None:
        return None
    return C.byref(np.ctypeslib.as_ctypes_type(a.dtype).from_buffer(a.reshape(-1), i * a.itemsize))


def _call(kind, single, vals, m, n, traceback, scored=True, wide=False, banded=False, xdrop=False):
    """One call of ``kind``'s single-pair or batch entry over the len(m) pairs whose input slots ``vals`` holds (pair p
    is m[p] x n[p]) -> the list of their result dicts.  The outputs are arrays with one row per pair, which either
    flavour of entry fills; the argument order is the entry's slot order."""
    k = len(m)
    name, slots = kind.entry(not single, scored, banded, wide, xdrop)
    outs = {o: np.zeros((k, 2), dtype=np.int64) if o in kind.pairs
            else np.zeros((k, 2) if kind.flanks and o in ("flank_score", "diagonals") else k,
                          dtype=np.int64 if o == "diagonals" else np.int32) for o in kind.outputs(xdrop)}
    coff = np.zeros(k + 1, dtype=np.int64)
    cap = int(4 * (m.sum() + n.sum()) + 16 * k) if traceback else 0
    cig = C.create_string_buffer(cap) if traceback else None
    vals = dict(vals, k=k, cigar=cig, cap=cap, cigar_off=_ptr(coff) if traceback else None)
    for o, a in outs.items():
        if o in kind.withheld and not traceback:
            a = None
        # (a single pair's {i, j}: one pointer, or one to each)
        vals[o] = vals[o + "_i"] = _ref(a, 0)
        vals[o + "_j"] = _ref(a, 1) if o in kind.pairs else None
    LB.check(getattr(LB.lib(), name)(*(vals[s] for s in slots)), name)
    res = []
    for p in range(k):
        r = kind.result(traceback, *(a[p] for a in outs.values()))
        if traceback:
            r["cigar"] = cig.value.decode() if single else cig.raw[coff[p]:coff[p + 1] - 1].decode()
        res.append(r)
    return res


def _align(kind, single, As, Bs, gap_open, gap_extend, traceback, match, mismatch, alphabet, matrix, max_symbols,
           band=None, xdrop=None, extra=None):
    """The sequence-against-sequence kinds: ``As`` / ``Bs`` as for the batch functions, or one sequence each with
    ``single``; ``band`` None = the entry without one; ``xdrop`` None = the entry without X-drop termination;
    ``extra``: the kind's int64 inputs per pair, name -> array (a single entry takes element 0).  -> the list of
    result dicts."""
    if max_symbols not in (8, 32):
        raise ValueError("max_symbols must be 8 or 32")
    if xdrop is not None and band is None:
        raise ValueError("xdrop needs a band")
    if single:
        As, Bs = [As], [Bs]
    elif len(As) == 0:
        return []
    A, B, a_off, m, b_off, n = _batch_in(As, Bs)
    scoring = _scoring(kind, (A, B), match, mismatch, alphabet, matrix, max_symbols)
    vals = dict(A=A, a_len=len(A), B=B, b_len=len(B), a_off=_ptr(a_off), m=_ptr(m), b_off=_ptr(b_off), n=_ptr(n),
                gap_open=gap_open, gap_extend=gap_extend, band=band, xdrop=xdrop)
    for name, x in (extra or {}).items():
        if len(x) != len(m):
            raise ValueError(f"{name} must hold one entry per pair")
        vals[name], vals[name + "0"] = _ptr(x), int(x[0])
    if scoring is None:
        vals.update(match=1 if match is None else match, mismatch=0 if mismatch is None else mismatch)
    else:
        alpha, S = scoring
        vals.update(alphabet=alpha, n_sym=len(alpha), sub=_ptr(S))
    res = _call(kind, single, vals, m, n, traceback, scoring is not None, max_symbols == 32,
                bool(kind.band) and band is not None, xdrop is not None)
    if xdrop is not None and not kind.flanks:  # (the fill stopped before the clipped pair's last anti-diagonal)
        for r, mp, np_ in zip(res, m, n):
            r["dropped"] = _dropped(r["diagonals"], int(mp), int(np_), band)
    return res


def _dropped(diagonals, m, n, band):
    """The fill of an m x n extension stopped before its clipped pair's last anti-diagonal."""
    return diagonals < min(m, n + band) + min(n, m + band)


def sw_align(A, B, match=None, mismatch=None, gap_open=1, gap_extend=1, traceback=True, alphabet=None, matrix=None,
             max_symbols=8):
    """Smith-Waterman local alignment (build extension) -> dict(score, end, beg, cigar).

    ``match`` / ``mismatch`` (None: 1 / 0) over the symbols of A and B, at most 7 (msa_sw_align).  Or ``alphabet``
    (up to 7 distinct bytes) with ``matrix``, len(alphabet) x len(alphabet) scores in [-128, 127], ``matrix[a][b]`` =
    alphabet[a] in A against alphabet[b] in B (msa_sw_align_scored); giving ``match`` or ``mismatch`` with it is a
    ValueError, as for nw_align.  ``max_symbols=32`` (msa_sw_align_scored32; any value but 8 or 32 is a ValueError):
    ``alphabet`` may hold up to 31 bytes -- proteins, IUPAC DNA --, and ``match`` / ``mismatch`` score the symbols of
    A and B themselves, at most 31.  The matrix-scored calls run the stripe kernel whatever the pair's size."""
    return _align(LB.KINDS["sw"], True, A, B, gap_open, gap_extend, traceback, match, mismatch, alphabet, matrix,
                  max_symbols)[0]


def nw_align(A, B, gap_open=3, gap_extend=1, band=-1, traceback=True, match=None, mismatch=None, alphabet=None,
             matrix=None, max_symbols=8):
    """Global (Gotoh) alignment (build extension) -> dict(score, cigar).

    +1 on equal symbols, 0 otherwise; a gap of L costs (gap_open - gap_extend) + gap_extend * L.  ``band`` >= 0
    restricts the alignment to |i - j| <= band (-1: none).  The fill writes one direction byte per in-band cell,
    the walk runs on the device, and the CIGAR (start -> end, I consumes A, D consumes B) consumes all of A and
    B.  ``traceback=False`` returns the score only.

    Other scores (msa_nw_align_scored): ``match`` and / or ``mismatch`` (the other stays 1 / 0) over the symbols
    of A and B, at most 8; or ``alphabet`` (up to 8 distinct bytes) with ``matrix``, len(alphabet) x len(alphabet)
    scores in [-128, 127], ``matrix[a][b]`` = alphabet[a] in A against alphabet[b] in B (it need not be
    symmetric).  With none of the four given, today's +1 / 0 call runs.

    ``max_symbols=32`` (msa_nw_align_scored32; any value but 8 or 32 is a ValueError): proteins, IUPAC DNA --
    ``alphabet`` may hold up to 32 bytes, ``match`` / ``mismatch`` take up to 32 distinct symbols, and with none of
    the four given the call scores +1 / 0 over the symbols of A and B."""
    return _align(LB.KINDS["nw"], True, A, B, gap_open, gap_extend, traceback, match, mismatch, alphabet, matrix,
                  max_symbols, band)[0]


def sw_align_batch(As, Bs, match=None, mismatch=None, gap_open=1, gap_extend=1, traceback=True, alphabet=None,
                   matrix=None, max_symbols=8):
    """A batch of Smith-Waterman local alignments (msa_sw_align_batch) -> a list of sw_align()'s dicts.

    ``Bs``: a list as long as ``As``, or one bytes object every A is aligned against (uploaded once).  One symbol
    map serves the whole call: at most 7 distinct symbols in all of As and Bs together.  The pairs run as batch
    plans (one fill and one walk launch per chunk of pairs that fits a quarter of the device budget).
    ``match`` / ``mismatch`` / ``alphabet`` / ``matrix`` / ``max_symbols`` as for sw_align (msa_sw_align_batch_scored,
    msa_sw_align_batch_scored32), over one alphabet for the whole call: up to 7 symbols, or 31."""
    return _align(LB.KINDS["sw"], False, As, Bs, gap_open, gap_extend, traceback, match, mismatch, alphabet, matrix,
                  max_symbols)


def nw_align_batch(As, Bs, gap_open=3, gap_extend=1, band=-1, traceback=True, match=None, mismatch=None,
                   alphabet=None, matrix=None, max_symbols=8):
    """A batch of global (Gotoh) alignments (msa_nw_align_batch) -> a list of nw_align()'s dicts.

    ``Bs`` as for sw_align_batch; scoring and ``band`` as for nw_align (the band holds for every pair).  One
    symbol map serves the whole call: at most 8 distinct symbols in all of As and Bs together.  ``match`` /
    ``mismatch`` / ``alphabet`` / ``matrix`` as for nw_align (msa_nw_align_batch_scored); the alphabet of ``match`` /
    ``mismatch`` is the distinct symbols of all As, then all Bs, in first-seen order.  ``max_symbols=32`` as for
    nw_align (msa_nw_align_batch_scored32): up to 32 distinct symbols in the whole call."""
    return _align(LB.KINDS["nw"], False, As, Bs, gap_open, gap_extend, traceback, match, mismatch, alphabet, matrix,
                  max_symbols, band)


def fit_align(query, ref, gap_open=3, gap_extend=1, traceback=True, match=None, mismatch=None, alphabet=None,
              matrix=None, max_symbols=8):
    """Fit ("glocal", "semi-global", "infix") alignment (build extension, msa_fit_align): ALL of ``query`` against
    the substring of ``ref`` it fits best -> dict(score, beg, end[, cigar]), ``ref[beg:end]`` being that substring.

    Reference symbols before ``beg`` and from ``end`` on are free; a gap of L costs (gap_open - gap_extend) +
    gap_extend * L.  Of equally good alignments the one ending first in the reference is reported.  The CIGAR
    (start -> end, I consumes the query, D the reference) consumes all of the query and ``end - beg`` reference
    symbols; ``beg == end`` when the best alignment inserts the whole query.  ``traceback=False`` gives the score
    and ``end`` only (``beg`` is None).  Scoring as for nw_align: ``match`` / ``mismatch``, or ``alphabet`` with
    ``matrix``; with none given +1 / 0.  ``max_symbols=32`` (msa_fit_align32): up to 32 symbols, as for nw_align."""
    return _align(LB.KINDS["fit"], True, query, ref, gap_open, gap_extend, traceback, match, mismatch, alphabet,
                  matrix, max_symbols)[0]


def fit_align_batch(queries, refs, gap_open=3, gap_extend=1, traceback=True, match=None, mismatch=None,
                    alphabet=None, matrix=None, max_symbols=8):
    """A batch of fit alignments (msa_fit_align_batch) -> a list of fit_align()'s dicts.

    ``refs``: a list as long as ``queries``, or one bytes object every query is aligned against (uploaded once),
    exactly like nw_align_batch's ``Bs``; scoring as for fit_align, over one alphabet for the whole call (``match``
    / ``mismatch``: the distinct symbols of all queries, then all refs, in first-seen order).  ``max_symbols=32``
    (msa_fit_align_batch32): up to 32 symbols in the whole call."""
    return _align(LB.KINDS["fit"], False, queries, refs, gap_open, gap_extend, traceback, match, mismatch, alphabet,
                  matrix, max_symbols)


def overlap_align(A, B, gap_open=3, gap_extend=1, traceback=True, match=None, mismatch=None, alphabet=None,
                  matrix=None, max_symbols=8):
    """Overlap ("dovetail", "ends-free") alignment (build extension, msa_overlap_align): the best alignment of a
    suffix of one sequence with a prefix of the other, or of one sequence inside the other -> dict(score, a_beg,
    a_end, b_beg, b_end[, cigar]): ``A[a_beg:a_end]`` against ``B[b_beg:b_end]``.

    All four ends are free: ``a_beg == 0 or b_beg == 0``, and ``a_end == len(A) or b_end == len(B)``.  A gap of L
    costs (gap_open - gap_extend) + gap_extend * L.  Of equally good end cells one on A's last symbol wins (the
    leftmost there), then the topmost on B's last symbol.  No positive score: the empty overlap, score 0,
    ``a_beg == a_end == len(A)``, ``b_beg == b_end == 0`` and an empty CIGAR.  The CIGAR (start -> end, I consumes A,
    D consumes B) consumes exactly ``a_end - a_beg`` and ``b_end - b_beg``.  ``traceback=False`` gives the score and
    the two ends only (``a_beg`` and ``b_beg`` are None).  Scoring and ``max_symbols`` as for fit_align."""
    return _align(LB.KINDS["overlap"], True, A, B, gap_open, gap_extend, traceback, match, mismatch, alphabet, matrix,
                  max_symbols)[0]


def overlap_align_batch(As, Bs, gap_open=3, gap_extend=1, traceback=True, match=None, mismatch=None, alphabet=None,
                        matrix=None, max_symbols=8):
    """A batch of overlap alignments (msa_overlap_align_batch) -> a list of overlap_align()'s dicts.

    ``Bs``: a list as long as ``As``, or one bytes object every A is aligned against (uploaded once), exactly like
    nw_align_batch's; scoring as for overlap_align, over one alphabet for the whole call (``match`` / ``mismatch``:
    the distinct symbols of all As, then all Bs, in first-seen order).  ``max_symbols=32``
    (msa_overlap_align_batch32): up to 32 symbols in the whole call."""
    return _align(LB.KINDS["overlap"], False, As, Bs, gap_open, gap_extend, traceback, match, mismatch, alphabet,
                  matrix, max_symbols)


def extend_align(A, B, gap_open=3, gap_extend=1, traceback=True, match=None, mismatch=None, alphabet=None,
                 matrix=None, max_symbols=8, band=-1, xdrop=None):
    """Extension alignment (build extension, msa_extend_align): the alignment starts at the first symbols of both
    sequences and may stop anywhere -> dict(score, a_end, b_end, global_score[, cigar]): the best-scoring pair of
    prefixes, ``A[:a_end]`` against ``B[:b_end]``.

    What a seed-and-extend pipeline runs on each flank of a seed (rightwards on the flanks, leftwards on the reversed
    ones).  A gap of L costs (gap_open - gap_extend) + gap_extend * L.  Of equally good end cells the first in
    row-major order wins (the smallest ``a_end``, then the smallest ``b_end``).  No positive score: the empty
    extension, score 0, ``a_end == b_end == 0`` and an empty CIGAR.  The CIGAR (start -> end, I consumes A, D consumes
    B) consumes exactly ``a_end`` and ``b_end``.  ``global_score`` is the end-to-end score of all of A against all of
    B -- nw_align's -- from the same fill: compare it with ``score`` to choose between clipping and aligning to the
    end.  ``traceback=False`` gives the scores and the end cell only.  Scoring and ``max_symbols`` as for fit_align.

    ``band`` >= 0 (msa_extend_align_banded): only cells with ``|i - j| <= band`` exist, so the work is bounded by the
    lengths and the band -- about ``(2 band + 1) min(m, n)`` cells instead of ``m n`` -- and the extension is the best
    one with at most ``band`` net indels at every point.  Rows past ``len(B) + band`` and columns past ``len(A) +
    band`` hold no such cell: the call clips the longer sequence there, and ``global_score`` is then ``None`` (there
    is no end-to-end alignment inside the band); otherwise it is nw_align's under the same band.  A negative band
    other than the default -1 is an MsaError (ARG).

    ``xdrop`` (msa_extend_align_xdrop; needs ``band`` >= 0, else ValueError; at most ``_lib.XDROP_BAND_MAX``, else an
    MsaError (UNSUPPORTED)): X-drop termination, BLAST's.  The fill goes anti-diagonal by anti-diagonal (``i + j``) and
    stops after the first one at which the maxima of the last two anti-diagonals both lie more than ``xdrop`` (raw score
    units) below the best score so far; cells on later anti-diagonals do not exist for the result.  The dict gains
    ``diagonals`` (the last anti-diagonal filled) and ``dropped`` (the fill stopped before the clipped pair's last one;
    ``global_score`` is then ``None``).  ``xdrop`` < 0 never stops: the banded call's result.  One wave fills one pair:
    made for batches of short flanks, not for one long pair."""
    return _align(LB.KINDS["extend"], True, A, B, gap_open, gap_extend, traceback, match, mismatch, alphabet, matrix,
                  max_symbols, None if band == -1 else int(band), None if xdrop is None else int(xdrop))[0]


def extend_align_batch(As, Bs, gap_open=3, gap_extend=1, traceback=True, match=None, mismatch=None, alphabet=None,
                       matrix=None, max_symbols=8, band=-1, xdrop=None):
    """A batch of extension alignments (msa_extend_align_batch) -> a list of extend_align()'s dicts.

    ``Bs``: a list as long as ``As``, or one bytes object every A is aligned against (uploaded once), exactly like
    nw_align_batch's; scoring as for extend_align, over one alphabet for the whole call (``match`` / ``mismatch``:
    the distinct symbols of all As, then all Bs, in first-seen order).  ``max_symbols=32``
    (msa_extend_align_batch32): up to 32 symbols in the whole call.  ``band`` >= 0 (msa_extend_align_batch_banded): one
    band for every pair, each clipped to it on its own, as extend_align does.  ``xdrop`` (msa_extend_align_batch_xdrop):
    one X-drop for every pair, as for extend_align; each pair stops on its own."""
    return _align(LB.KINDS["extend"], False, As, Bs, gap_open, gap_extend, traceback, match, mismatch, alphabet,
                  matrix, max_symbols, None if band == -1 else int(band), None if xdrop is None else int(xdrop))


def _seed(single, As, Bs, seed_a, seed_b, seed_len, band, xdrop, gap_open, gap_extend, traceback, match, mismatch,
          alphabet, matrix, max_symbols):
    """seed_align / seed_align_batch: the call through _align, then each flank's end cell and ``dropped`` from the
    seed's coordinates (an empty flank is never dropped)."""
    sa, sb, sl = (np.atleast_1d(np.asarray(x, dtype=np.int64)) for x in (seed_a, seed_b, seed_len))
    band = -1 if band is None else int(band)  # (no band: the entries' MSA_ERR_ARG)
    res = _align(LB.KINDS["seed"], single, As, Bs, gap_open, gap_extend, traceback, match, mismatch, alphabet, matrix,
                 max_symbols, band, int(xdrop), extra=dict(seed_a=sa, seed_b=sb, seed_len=sl))
    lens = [(len(_buf(As)), len(_buf(Bs)))] if single else \
        [(len(_buf(a)), len(_buf(Bs if isinstance(Bs, (bytes, bytearray, str, memoryview)) else Bs[p])))
         for p, a in enumerate(As)]
    for r, (m, n), a, b, k in zip(res, lens, sa.tolist(), sb.tolist(), sl.tolist()):
        r["left"].update(a_end=a - r["a_beg"], b_end=b - r["b_beg"])
        r["right"].update(a_end=r["a_end"] - a - k, b_end=r["b_end"] - b - k)
        for f, fm, fn in ((r["left"], a, b), (r["right"], m - a - k, n - b - k)):
            f["dropped"] = fm > 0 and fn > 0 and _dropped(f["diagonals"], fm, fn, band)
    return res


def seed_align(A, B, seed_a, seed_b, seed_len, band, xdrop=-1, gap_open=3, gap_extend=1, traceback=True, match=None,
               mismatch=None, alphabet=None, matrix=None, max_symbols=8):
    """Seed extension (build extension, msa_seed_align): the alignment through the seed ``A[seed_a:seed_a+seed_len]``
    against ``B[seed_b:seed_b+seed_len]``, extended on both flanks in one call -> dict(score, a_beg, b_beg, a_end,
    b_end, seed_score, left, right[, cigar]): ``A[a_beg:a_end]`` against ``B[b_beg:b_end]``.

    Each flank is exactly ``extend_align(..., band=band, xdrop=xdrop)`` of its two byte strings -- the right flank
    ``A[seed_a+seed_len:]`` against ``B[seed_b+seed_len:]``, the left flank ``A[:seed_a][::-1]`` against
    ``B[:seed_b][::-1]``, which the kernel reads backwards in place: nothing is reversed or copied.  ``left`` and
    ``right`` are dict(score, a_end, b_end, diagonals, dropped) in the flank's own coordinates (``a_end`` symbols of A
    away from the seed); a flank with no symbols on one side is not launched and is the empty extension (score 0,
    ``a_end == b_end == diagonals == 0``, not dropped).  ``seed_score`` is the sum of the seed's column scores (it may
    hold mismatches; ``seed_len=0`` is a bare anchor) and ``score = left + seed_score + right``.  The CIGAR (start ->
    end, I consumes A, D consumes B) consumes exactly ``a_end - a_beg`` and ``b_end - b_beg``: the left flank's
    alignment, ``seed_len`` M, the right flank's.  ``band`` is required (None or a negative one: an MsaError (ARG);
    above ``_lib.XDROP_BAND_MAX``: UNSUPPORTED); ``xdrop`` < 0 never stops.  ``traceback=False`` gives everything but
    the CIGAR and runs no walk.  Scoring and ``max_symbols`` as for extend_align."""
    return _seed(True, A, B, seed_a, seed_b, seed_len, band, xdrop, gap_open, gap_extend, traceback, match, mismatch,
                 alphabet, matrix, max_symbols)[0]


def seed_align_batch(As, Bs, seed_a, seed_b, seed_len, band, xdrop=-1, gap_open=3, gap_extend=1, traceback=True,
                     match=None, mismatch=None, alphabet=None, matrix=None, max_symbols=8):
    """A batch of seed extensions (msa_seed_align_batch) -> a list of seed_align()'s dicts.

    One seed per pair: ``seed_a`` / ``seed_b`` / ``seed_len`` hold one entry per pair, relative to it.  ``Bs``: a list
    as long as ``As``, or one bytes object every A is aligned against (uploaded once): many seeds against one reference.
    Several seeds on one pair are pairs whose sequences coincide.  One band, one xdrop and one alphabet for the whole
    call; every launched flank is one wave's task, the two flanks of a seed next to each other."""
    return _seed(False, As, Bs, seed_a, seed_b, seed_len, band, xdrop, gap_open, gap_extend, traceback, match, mismatch,
                 alphabet, matrix, max_symbols)


def _chain(single, seed_a, seed_b, seed_len, band, match, gap_open, gap_extend, max_dist, lookback, min_score):
    """chain_seeds / chain_seeds_batch: every problem sorted by (be, ae, the caller's index), the library's call over the
    sorted anchors, and its results mapped back -> per problem (chains, f, pred), f and pred in the caller's indexing."""
    probs = []
    for x in zip(seed_a, seed_b, seed_len):
        a, b, ln = (np.asarray(v, dtype=np.int64).reshape(-1) for v in x)
        if not len(a) == len(b) == len(ln):
            raise ValueError("seed_a, seed_b and seed_len must hold one entry per anchor")
        # (lexsort is stable: equal (be, ae) stay in the caller's order)
        probs.append((a, b, ln, np.lexsort((a + ln, b + ln))))
    off = np.concatenate(([0], np.cumsum([len(p[0]) for p in probs]))).astype(np.int64)
    total = int(off[-1])
    a, b, ln = (np.ascontiguousarray(np.concatenate([p[k][p[3]] for p in probs]), dtype=np.int64) for k in range(3))
    f, pred, chain_of, score = (np.zeros(max(total, 1), dtype=np.int32) for _ in range(4))
    n_chains = np.zeros(len(probs), dtype=np.int32)
    params = (int(match), int(gap_open), int(gap_extend), -1 if band is None else int(band), int(max_dist),
              int(lookback), int(min_score))
    outs = (_ptr(f), _ptr(pred), _ptr(chain_of), _ptr(n_chains), _ptr(score))
    if single:
        name = "msa_chain_seeds"
        rc = LB.lib().msa_chain_seeds(_ptr(a), _ptr(b), _ptr(ln), total, *params, *outs)
    else:
        name = "msa_chain_seeds_batch"
        rc = LB.lib().msa_chain_seeds_batch(_ptr(a), _ptr(b), _ptr(ln), len(probs), _ptr(off), *params, *outs)
    LB.check(rc, name)
    res = []
    for p, (pa, pb, pl, order) in enumerate(probs):
        lo, hi = int(off[p]), int(off[p + 1])
        co = chain_of[lo:hi]
        # the anchors of every kept chain, by rank, each in ascending sorted position: chain order
        kept = np.flatnonzero(co >= 0)
        kept = kept[np.argsort(co[kept], kind="stable")]
        ends = np.cumsum(np.bincount(co[kept], minlength=int(n_chains[p])))
        chains = []
        for r in range(int(n_chains[p])):
            members = order[kept[ends[r - 1] if r else 0:ends[r]]]
            first, last = int(members[0]), int(members[-1])
            chains.append(dict(score=int(score[lo + r]), anchors=[int(t) for t in members], a_beg=int(pa[first]),
                               b_beg=int(pb[first]), a_end=int(pa[last] + pl[last]), b_end=int(pb[last] + pl[last])))
        fc, pc = np.zeros(hi - lo, dtype=np.int32), np.full(hi - lo, -1, dtype=np.int32)
        fc[order] = f[lo:hi]
        has = pred[lo:hi] >= 0
        pc[order[has]] = order[pred[lo:hi][has]]
        res.append((chains, fc, pc))
    return res


def chain_seeds(seed_a, seed_b, seed_len, band, match=1, gap_open=3, gap_extend=1, max_dist=5000, lookback=64,
                min_score=0):
    """Seed chaining (build extension, msa_chain_seeds): the chains of one pair's anchors, rank 0 (the best) first ->
    a list of dict(score, anchors, a_beg, b_beg, a_end, b_end).

    Anchor t is ``A[seed_a[t] : seed_a[t] + seed_len[t]]`` seeded against ``B[seed_b[t] : ...]`` (seed_align's
    coordinates), in any order: the call sorts them by (b end, a end, index), and ``anchors`` holds the CALLER's
    indices in chain order; the chain spans ``A[a_beg:a_end]`` and ``B[b_beg:b_end]``.  With ``ae = a + len``,
    ``be = b + len``, ``da = ae_i - ae_j`` and ``db = be_i - be_j``, anchor j (earlier in the sorted order) may precede
    i iff it is at most ``lookback`` places before it, ``0 < da, db <= max_dist`` and ``|da - db| <= band``; then
    ``f(i) = max(match len_i, max_j f(j) + match min(da, db, len_i) - gc(|da - db|))``, ``gc(L) = (gap_open -
    gap_extend) + gap_extend L``, ``gc(0) = 0``, the predecessor being the latest j that gives the maximum.  Chains are
    cut from the anchors in order of ``f`` descending: follow the predecessors until there is none or one is taken by an
    earlier chain (the chain then scores the difference); chains below ``min_score`` are dropped, their anchors stay
    taken.  All integers: the result is exact.  ``band`` is required (None or negative: an MsaError (UNSUPPORTED), as
    for every parameter outside its bounds: ``match`` 1..15, ``gap_open >= gap_extend >= 0``, ``max_dist >= 1``,
    ``lookback`` 1.. ``_lib.CHAIN_LOOKBACK_MAX``); a negative coordinate, ``len < 1`` or an end above 2**26: ARG.  The
    recurrence runs on the device, one wave per problem; a problem of at most one anchor needs none."""
    return _chain(True, [seed_a], [seed_b], [seed_len], band, match, gap_open, gap_extend, max_dist, lookback,
                  min_score)[0][0]


def chain_seeds_batch(seed_a, seed_b, seed_len, band, match=1, gap_open=3, gap_extend=1, max_dist=5000, lookback=64,
                      min_score=0, full=False):
    """A batch of chaining problems (msa_chain_seeds_batch) -> a list of chain_seeds()'s lists.

    ``seed_a`` / ``seed_b`` / ``seed_len``: lists holding one array per problem; one set of parameters for the call.
    ``full=True`` -> (that list, f, pred): per problem the int32 arrays ``f`` and ``pred`` in the caller's indexing
    (``pred[t]`` = the caller's index of t's predecessor, or -1)."""
    if not (len(seed_a) == len(seed_b) == len(seed_len)):
        raise ValueError("seed_a, seed_b and seed_len must hold one array per problem")
    res = _chain(False, seed_a, seed_b, seed_len, band, match, gap_open, gap_extend, max_dist, lookback,
                 min_score) if len(seed_a) else []
    chains = [r[0] for r in res]
    return (chains, [r[1] for r in res], [r[2] for r in res]) if full else chains


def _runs(cigar):
    """[[run, op]] of a CIGAR string."""
    out, run = [], 0
    for c in cigar:
        if c.isdigit():
            run = 10 * run + int(c)
        else:
            out.append([run, c])
            run = 0
    return out


def _split_runs(runs, ca, cb):
    """(head, tail) of a run list: head consumes exactly ``ca`` symbols of A (M, I) and ``cb`` of B (M, D)."""
    head, runs = [], [list(r) for r in runs]
    while ca or cb:
        run, op = runs[0]
        take = min(run, ca if op == "I" else cb if op == "D" else min(ca, cb))
        if take == 0:
            raise LB.MsaError(-9, "chain_align")  # (cannot happen: the flanks' ends are the walk's own)
        head.append([take, op])
        ca, cb = ca - take * (op != "D"), cb - take * (op != "I")
        if take == run:
            runs.pop(0)
        else:
            runs[0][0] -= take
    return head, runs


def _chain_align(single, As, Bs, seed_a, seed_b, seed_len, band, xdrop, chain_match, chain_gap_open, chain_gap_extend,
                 max_dist, lookback, min_score, gap_open, gap_extend, traceback, match, mismatch, alphabet, matrix,
                 max_symbols):
    """chain_align / chain_align_batch: three device calls per batch -- chain_seeds_batch, ONE nw_align_batch over the
    gaps between the anchors of every pair's best chain, ONE seed_align_batch for the two outer flanks (a bare anchor
    between ``A[:a_beg]`` and ``A[a_end:]`` joined, and the same of B: its left and right flank are the chain's) -- and
    the sum of the parts."""
    if max_symbols not in (8, 32):
        raise ValueError("max_symbols must be 8 or 32")
    As = [_buf(x) for x in As]
    Bs = [_buf(Bs)] * len(As) if isinstance(Bs, (bytes, bytearray, str, memoryview)) else [_buf(x) for x in Bs]
    if not (len(As) == len(Bs) == len(seed_a) == len(seed_b) == len(seed_len)):
        raise ValueError("Bs, seed_a, seed_b and seed_len must hold one entry per pair")
    if not As:
        return []
    go, ge = int(gap_open), int(gap_extend)
    skw = dict(gap_open=go, gap_extend=ge, traceback=traceback, match=match, mismatch=mismatch, alphabet=alphabet,
               matrix=matrix, max_symbols=max_symbols)
    _scoring(LB.KINDS["seed"], (), match, mismatch, alphabet, matrix, max_symbols)  # (the argument rules, before work)
    chains = _chain(single, seed_a, seed_b, seed_len, band,
                    chain_match, go if chain_gap_open is None else chain_gap_open,
                    ge if chain_gap_extend is None else chain_gap_extend, max_dist, lookback, min_score)
    if matrix is not None:
        S, lut = np.asarray(matrix, dtype=np.int64), np.full(256, -1, dtype=np.int64)
        lut[np.frombuffer(_buf(alphabet), dtype=np.uint8)] = np.arange(len(_buf(alphabet)))
    ma, mi = (1 if match is None else int(match)), (0 if mismatch is None else int(mismatch))

    def columns(x, y):  # the score of the columns x[t] against y[t]
        x, y = np.frombuffer(x, dtype=np.uint8), np.frombuffer(y, dtype=np.uint8)
        if matrix is None:
            return int(np.where(x == y, ma, mi).sum())
        if (lut[x] < 0).any() or (lut[y] < 0).any():
            raise LB.MsaError(-2, "chain_align")
        return int(S[lut[x], lut[y]].sum())

    # per pair with a chain: its parts in order, ("M", k, score) | ("I" / "D", L, score) | ("gap", index into the nw
    # batch); the gaps of all pairs are one batch, the flanks of all pairs another
    plans, gap_a, gap_b, fl_a, fl_b, fl_sa, fl_sb = [], [], [], [], [], [], []
    for A, B, sa, sb, sl, (found, _, _) in zip(As, Bs, seed_a, seed_b, seed_len, chains):
        if not found:
            plans.append(None)
            continue
        sa, sb, sl = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (sa, sb, sl))
        ch = found[0]
        t0 = ch["anchors"][0]
        pae, pbe = int(sa[t0] + sl[t0]), int(sb[t0] + sl[t0])
        if pae > len(A) or pbe > len(B):
            raise LB.MsaError(-1, "chain_align")
        parts = [("M", int(sl[t0]), columns(A[ch["a_beg"]:pae], B[ch["b_beg"]:pbe]))]
        for t in ch["anchors"][1:]:
            ae, be = int(sa[t] + sl[t]), int(sb[t] + sl[t])
            if ae > len(A) or be > len(B):
                raise LB.MsaError(-1, "chain_align")
            k = min(ae - pae, be - pbe, int(sl[t]))  # the anchor keeps its last k columns
            ga, gb = ae - k - pae, be - k - pbe
            if ga and gb:
                parts.append(("gap", len(gap_a)))
                gap_a.append(A[pae:ae - k])
                gap_b.append(B[pbe:be - k])
            elif ga or gb:
                parts.append(("I" if ga else "D", ga + gb, -((go - ge) + ge * (ga + gb))))
            parts.append(("M", k, columns(A[ae - k:ae], B[be - k:be])))
            pae, pbe = ae, be
        fa, fb = A[:ch["a_beg"]] + A[pae:], B[:ch["b_beg"]] + B[pbe:]
        plans.append((ch, parts, len(fl_a) if fa and fb else None))
        if fa and fb:
            fl_a.append(fa), fl_b.append(fb), fl_sa.append(ch["a_beg"]), fl_sb.append(ch["b_beg"])
    gaps = nw_align_batch(gap_a, gap_b, band=-1 if band is None else int(band), **skw) if gap_a else []
    flanks = seed_align_batch(fl_a, fl_b, fl_sa, fl_sb, [0] * len(fl_a), band, xdrop=xdrop, **skw) if fl_a else []
    empty = dict(score=0, a_end=0, b_end=0, diagonals=0, dropped=False)
    res = []
    for plan in plans:
        if plan is None:
            res.append(None)
            continue
        ch, parts, fl = plan
        left, right = (flanks[fl]["left"], flanks[fl]["right"]) if fl is not None else (dict(empty), dict(empty))
        score, runs = left["score"] + right["score"], []
        if traceback:
            runs, tail = _split_runs(_runs(flanks[fl]["cigar"]), left["a_end"], left["b_end"]) if fl is not None \
                else ([], [])
        for part in parts:
            if part[0] == "gap":
                g = gaps[part[1]]
                score += g["score"]
                more = _runs(g["cigar"]) if traceback else []
            else:
                score += part[2]
                more = [[part[1], part[0]]] if part[1] else []
            runs += more
        r = dict(score=score, a_beg=ch["a_beg"] - left["a_end"], b_beg=ch["b_beg"] - left["b_end"],
                 a_end=ch["a_end"] + right["a_end"], b_end=ch["b_end"] + right["b_end"], chain_score=ch["score"],
                 anchors=ch["anchors"], left=left, right=right)
        if traceback:
            merged = []
            for run, op in runs + tail:
                if merged and merged[-1][1] == op:
                    merged[-1][0] += run
                else:
                    merged.append([run, op])
            r["cigar"] = "".join(f"{run}{op}" for run, op in merged)
        res.append(r)
    return res


def chain_align(A, B, seed_a, seed_b, seed_len, band, xdrop=-1, chain_match=1, chain_gap_open=None,
                chain_gap_extend=None, max_dist=5000, lookback=64, min_score=0, gap_open=3, gap_extend=1,
                traceback=True, match=None, mismatch=None, alphabet=None, matrix=None, max_symbols=8):
    """The alignment of a pair through the best chain of its anchors -> dict(score, a_beg, b_beg, a_end, b_end,
    chain_score, anchors, left, right[, cigar]), or None for a pair without a chain (no anchors, or none reaching
    ``min_score``): ``A[a_beg:a_end]`` against ``B[b_beg:b_end]``.

    A Python composition of three device calls, not an alignment kind of the library: chain_seeds picks the rank-0 chain
    (``chain_match``, ``chain_gap_open`` / ``chain_gap_extend`` -- None: the alignment's ``gap_open`` / ``gap_extend``
    --, ``max_dist``, ``lookback``, ``min_score``; ``anchors`` are the caller's indices in chain order, ``chain_score``
    the chain's); then every part is a call the library already has, and ``score`` is their sum:
      * overlapping anchors are trimmed: after anchor j, anchor i keeps its last ``k = min(da, db, len_i)`` columns;
        each kept column scores under the call's scoring (mismatches allowed, as seed_align's ``seed_score``);
      * between them ``ga = da - k`` symbols of A and ``gb = db - k`` of B remain: nothing; or, one side empty, one I
        (A's) or D (B's) run costing ``(gap_open - gap_extend) + gap_extend L``; or ``nw_align(..., band=band)`` of the
        two substrings, which exists because the chain keeps ``|ga - gb| <= band`` -- all gaps of a call are one
        nw_align_batch call;
      * ``left`` and ``right`` are seed_align's dictionaries of the flank left of the first anchor and right of the
        last: ``extend_align(..., band=band, xdrop=xdrop)`` of those byte strings, the left ones reversed -- all
        flanks of a call are one seed_align_batch call.
    The CIGAR is the parts in order, neighbouring runs of one op merged, and consumes exactly ``a_end - a_beg`` and
    ``b_end - b_beg``.  ``traceback=False`` runs no walks.  Scoring and ``max_symbols`` as for seed_align."""
    return _chain_align(True, [A], [B], [seed_a], [seed_b], [seed_len], band, xdrop, chain_match, chain_gap_open,
                        chain_gap_extend, max_dist, lookback, min_score, gap_open, gap_extend, traceback, match,
                        mismatch, alphabet, matrix, max_symbols)[0]


def chain_align_batch(As, Bs, seed_a, seed_b, seed_len, band, xdrop=-1, chain_match=1, chain_gap_open=None,
                      chain_gap_extend=None, max_dist=5000, lookback=64, min_score=0, gap_open=3, gap_extend=1,
                      traceback=True, match=None, mismatch=None, alphabet=None, matrix=None, max_symbols=8):
    """A batch of chain_align() -> a list of its results (None for a pair without a chain).

    ``seed_a`` / ``seed_b`` / ``seed_len``: one array of anchors per pair; ``Bs``: a list as long as ``As``, or one bytes
    object every A is aligned against.  Three device calls for the whole batch: the chains, the gaps, the flanks."""
    return _chain_align(False, As, Bs, seed_a, seed_b, seed_len, band, xdrop, chain_match, chain_gap_open,
                        chain_gap_extend, max_dist, lookback, min_score, gap_open, gap_extend, traceback, match,
                        mismatch, alphabet, matrix, max_symbols)


_PROFILE_MODES = {"local": LB.PROFILE_LOCAL, "global": LB.PROFILE_GLOBAL, "fit": LB.PROFILE_FIT}


def profile_from_matrix(A, alphabet, matrix) -> np.ndarray:
    """The ``len(A) x len(alphabet)`` int8 profile whose row i is ``matrix[code(A_i)]``, a symbol's code being its
    index in ``alphabet``: the profile under which profile_align gives exactly what the matrix-scored call gives for
    A -- the starting profile of an iterated search.  A symbol of A outside the alphabet, a matrix that is not
    len(alphabet) x len(alphabet) or not int8-representable: ValueError."""
    A, alphabet = _buf(A), _buf(alphabet)
    S = np.asarray(matrix)
    if S.ndim != 2 or S.shape != (len(alphabet), len(alphabet)) or (S != S.astype(np.int8)).any():
        raise ValueError("matrix must be len(alphabet) x len(alphabet) scores in [-128, 127]")
    if len(set(alphabet)) != len(alphabet):
        raise ValueError("alphabet holds a symbol twice")
    code = np.full(256, -1, dtype=np.int64)
    code[np.frombuffer(alphabet, dtype=np.uint8)] = np.arange(len(alphabet))
    ca = code[np.frombuffer(A, dtype=np.uint8)]
    if (ca < 0).any():
        raise ValueError("A holds a symbol outside the alphabet")
    return np.ascontiguousarray(S.astype(np.int8)[ca].reshape(len(A), len(alphabet)))


def _profile_in(profile, alphabet, mode):
    """(mode number, contiguous int8 profile, alphabet bytes) of a profile call, or its ValueError."""
    if mode not in _PROFILE_MODES:
        raise ValueError("mode must be 'local', 'global' or 'fit'")
    alphabet = _buf(alphabet)
    P = np.asarray(profile)
    if P.ndim != 2 or P.dtype == object or (P != P.astype(np.int8)).any():
        raise ValueError("profile must be a 2-D array of scores in [-128, 127]")
    if P.shape[1] != len(alphabet):
        raise ValueError("profile must have len(alphabet) columns")
    return _PROFILE_MODES[mode], np.ascontiguousarray(P, dtype=np.int8), alphabet


def _profile_align(single, profile, seqs, alphabet, mode, gap_open, gap_extend, traceback):
    """profile_align (``seqs`` one sequence, with ``single``) / profile_align_batch -> the list of result dicts."""
    mo, P, alphabet = _profile_in(profile, alphabet, mode)
    B, b_off, n = _concat([seqs] if single else seqs)
    if len(n) == 0:
        return []
    vals = dict(mode=mo, prof=_ptr(P), rows=P.shape[0], B=B, b_len=len(B), b_off=_ptr(b_off), n=_ptr(n),
                alphabet=alphabet, n_sym=len(alphabet), gap_open=gap_open, gap_extend=gap_extend)
    return _call(LB.KINDS["profile"], single, vals, np.full(len(n), P.shape[0]), n, traceback)


def profile_align(profile, seq, alphabet, mode="local", gap_open=3, gap_extend=1, traceback=True):
    """A position-specific score profile (a PSSM) against a sequence (build extension, msa_profile_align) ->
    dict(score, beg, end[, cigar]).

    ``profile``: rows x len(alphabet) scores in [-128, 127], ``profile[r][c]`` = profile position r against
    ``alphabet[c]``; ``alphabet``: the distinct symbols of ``seq``, at most 31 for ``mode="local"`` and 32 otherwise.
    ``mode``: "local" (sw_align's recurrence and cells: ``beg`` the start cell, ``end`` the end cell), "global"
    (nw_align's, unbanded: ``(0, 0)`` and ``(rows, len(seq))``) or "fit" (fit_align's, the whole profile in a substring
    of ``seq``: ``(0, beg_j)`` and ``(rows, end_j)``).  The CIGAR (start -> end) has I consuming a profile row and D a
    symbol of ``seq``.  ``traceback=False`` gives the score and ``end`` only (``beg`` is None).  A gap of L costs
    (gap_open - gap_extend) + gap_extend * L.  Building the profile from a multiple alignment is the caller's job;
    profile_from_matrix gives the one a single sequence has under a substitution matrix."""
    return _profile_align(True, profile, seq, alphabet, mode, gap_open, gap_extend, traceback)[0]


def profile_align_batch(profile, seqs, alphabet, mode="local", gap_open=3, gap_extend=1, traceback=True):
    """One profile against many sequences (msa_profile_align_batch) -> a list of profile_align()'s dicts: the search
    case, every pair using all rows of ``profile``, which each plan of the call holds once."""
    return _profile_align(False, profile, seqs, alphabet, mode, gap_open, gap_extend, traceback)
