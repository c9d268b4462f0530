"""ctypes binding of libmsa.so (include/msa.h).

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C cse305_parallel_sequence_alignment_amd/csrc``.  There is no CPU
fallback: if the library is missing, importing the compute API raises, and
on a machine without a gfx950 GPU every call returns MSA_ERR_NODEV, which
this module turns into ``MsaError``.

The alignment entries (msa_sw_align ... msa_profile_align_batch) are not listed
by hand: ``KINDS`` declares each alignment kind once -- how its entries are
named, the order of their arguments, its outputs and its result dict -- and
both ``lib()``'s argtypes and api.py's calls come from that declaration.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, Optional, Tuple

PKG = Path(__file__).resolve().parent
# MSA_LIB_PATH: a diagnostic build (e.g. -DMSA_STAMPS) loaded instead of the in-tree library
LIB_PATH = Path(os.environ.get("MSA_LIB_PATH", str(PKG / "libmsa.so")))

MSA_OK = 0
STATUS = {
    0: "ok", -1: "invalid argument", -2: "more than 8 distinct symbols", -3: "HIP runtime error",
    -4: "no gfx950 device", -5: "unsupported parameters", -6: "cross-workgroup wait timed out",
    -7: "out of memory", -8: "output buffer too small", -9: "traceback found no predecessor",
}

# msa_alg_e / msa_out_e
SW_LINEAR, SW_AFFINE, NW_BANDED, REF_GOTOH, PARTIAL, NW_ALIGN, NW_SCORED, NW_FIT = 0, 1, 2, 3, 4, 5, 6, 7
SW_SCORED = 8
NW_OVERLAP = 9
NW_EXTEND = 10
NW_EXTEND_BAND = 11
SCORE_NONE = -(1 << 31)  # MSA_SCORE_NONE: no such score (a clipped banded extension's global score)
XDROP_BAND_MAX = 640     # MSA_XDROP_BAND_MAX
CHAIN_LOOKBACK_MAX = 1024  # MSA_CHAIN_LOOKBACK_MAX
CELLS_NONE, CELLS_H, CELLS_DIR, CELLS_TAB = 0, 1, 2, 3
# msa_profile_align's modes
PROFILE_LOCAL, PROFILE_GLOBAL, PROFILE_FIT = 0, 1, 2


class MsaError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        super().__init__(f"{what}: msa status {status} ({STATUS.get(status, 'unknown')})")


def check(rc: int, what: str = "msa") -> None:
    if rc != MSA_OK:
        raise MsaError(rc, what)


class Node(C.Structure):
    _fields_ = [("i", C.c_uint64), ("j", C.c_uint64), ("t", C.c_int32), ("pad", C.c_int32)]


class PlanDesc(C.Structure):
    _fields_ = [
        ("alg", C.c_int32), ("cells", C.c_int32), ("match", C.c_int32), ("mismatch", C.c_int32),
        ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("start_type", C.c_int32), ("band", C.c_int32),
        ("track_end", C.c_int32), ("single", C.c_int32), ("n_pairs", C.c_int64),
        ("m", C.POINTER(C.c_int64)), ("n", C.POINTER(C.c_int64)),
        ("a_off", C.POINTER(C.c_int64)), ("b_off", C.POINTER(C.c_int64)),
    ]


class PairResult(C.Structure):
    _fields_ = [("score", C.c_int32), ("status", C.c_int32), ("end_i", C.c_int64), ("end_j", C.c_int64),
                ("fin", C.c_int32 * 3), ("pad", C.c_int32)]


# The alignment entries (msa_*_align*).  An argument is a named slot; these are the integers, every other slot is a
# pointer.  A Kind puts the slots of each of its entries in C order, once: lib() takes the argtypes from that order and
# api.py the call.
_INT_SLOTS = {"mode": C.c_int, "a_len": C.c_size_t, "b_len": C.c_size_t, "rows": C.c_size_t, "n_sym": C.c_size_t,
              "cap": C.c_size_t, "k": C.c_int64, "band": C.c_int64, "match": C.c_int32, "mismatch": C.c_int32,
              "gap_open": C.c_int32, "gap_extend": C.c_int32, "xdrop": C.c_int32,
              "seed_a0": C.c_int64, "seed_b0": C.c_int64, "seed_len0": C.c_int64}


@dataclass(frozen=True)
class Kind:
    """One alignment kind of include/msa.h: the names of its entries, their arguments and its result."""
    name: str                                    # msa_<name>_align
    result: Callable                             # (traceback, one pair's outputs in C order) -> its dict, cigar aside
    pairs: Tuple[str, ...] = ()                  # the int64 {i, j} outputs that follow the score
    split: bool = False                          # a single-pair entry takes each as two pointers, to i and to j
    score2: bool = False                         # a second int32 score follows them (extension's global score)
    withheld: Tuple[str, ...] = ()               # the outputs that are NULL when traceback=False
    head: Tuple[str, ...] = ("A", "a_len")       # what stands on the A side
    matrix: Tuple[str, ...] = ("alphabet", "n_sym", "sub")
    # the scoring slots of the entries without `_scored`, which run when match / mismatch (sw) or nothing (nw) is
    # given and max_symbols is 8; None: there are none, every call has an alphabet and a matrix (+1 / 0 by default)
    plain: Optional[Tuple[str, ...]] = None
    sentinel: bool = False                       # the highest code is kept free: one symbol fewer than max_symbols
    band: Optional[str] = None                   # None: no band; "": in every entry; else the suffix of those with one
    # the suffix, in place of the band's, of the entries that stop by X-drop: `xdrop` follows `band`, and an int64
    # `diagonals` per pair follows the scores; "": every entry stops by X-drop
    xdrop: Optional[str] = None
    # int64 inputs after the sequences, one per pair: arrays in a batch entry (after `n`), values in a single-pair
    # entry (slot name + "0")
    extra: Tuple[str, ...] = ()
    # both flanks of a seed: an int32 `flank_score` follows the {i, j} outputs, and it and `diagonals` hold two
    # entries per pair, {left, right}
    flanks: bool = False

    def outputs(self, xdrop=False):
        return (("score",) + self.pairs + (("global_score",) if self.score2 else ())
                + (("flank_score",) if self.flanks else ()) + (("diagonals",) if xdrop or self.xdrop == "" else ()))

    def entry(self, batch, scored=True, banded=False, wide=False, xdrop=False):
        """(C name, argument slots in C order) of one entry."""
        xdrop = xdrop or self.xdrop == ""
        banded = banded or xdrop
        name = (f"msa_{self.name}_align" + "_batch" * batch + "_scored" * (scored and self.plain is not None)
                + (self.xdrop if xdrop else self.band if banded else "") + "32" * wide)
        slots = self.head + ("B", "b_len")
        if batch:
            slots += ("k",) + (("a_off", "m") if self.head[0] == "A" else ()) + ("b_off", "n")
        slots += self.extra if batch else tuple(x + "0" for x in self.extra)
        slots += self.matrix if scored else self.plain
        slots += ("gap_open", "gap_extend") + (("band",) if banded or self.band == "" else ()) + ("xdrop",) * xdrop
        for o in self.outputs(xdrop):
            slots += (o + "_i", o + "_j") if o in self.pairs and self.split and not batch else (o,)
        return name, slots + ("cigar", "cap") + (("cigar_off",) if batch else ())

    def entries(self):
        """Every entry the header declares for this kind."""
        for batch in (False, True):
            for scored in (True,) if self.plain is None else (False, True):
                for banded in (False, True) if self.band else (False,):
                    for wide in (False, True) if scored and "sub" in self.matrix else (False,):
                        yield self.entry(batch, scored, banded, wide)
                        if banded and self.xdrop:
                            yield self.entry(batch, scored, banded, wide, xdrop=True)


def _ij(c):
    return int(c[0]), int(c[1])


def _sw_result(tb, score, end, beg):
    return dict(score=int(score), end=_ij(end), **(dict(beg=_ij(beg)) if tb else {}))


def _fit_result(tb, score, beg_end):
    return dict(score=int(score), beg=int(beg_end[0]) if tb else None, end=int(beg_end[1]))


def _overlap_result(tb, score, beg, end):
    return dict(score=int(score), a_beg=int(beg[0]) if tb else None, a_end=int(end[0]),
                b_beg=int(beg[1]) if tb else None, b_end=int(end[1]))


def _extend_result(tb, score, end, gscore, diagonals=None):
    # (MSA_SCORE_NONE: a banded extension clipped the pair, or X-drop stopped it, so its fill never reached (m, n))
    r = dict(score=int(score), a_end=int(end[0]), b_end=int(end[1]),
             global_score=None if int(gscore) == SCORE_NONE else int(gscore))
    if diagonals is not None:
        r["diagonals"] = int(diagonals)
    return r


def _seed_result(tb, score, beg, end, flank, diagonals):
    # (api.seed_align adds each flank's end cell and `dropped`, which need the seed's coordinates)
    left, right = (dict(score=int(flank[f]), diagonals=int(diagonals[f])) for f in (0, 1))
    return dict(score=int(score), a_beg=int(beg[0]), b_beg=int(beg[1]), a_end=int(end[0]), b_end=int(end[1]),
                seed_score=int(score) - int(flank[0]) - int(flank[1]), left=left, right=right)


def _profile_result(tb, score, beg, end):
    return dict(score=int(score), beg=_ij(beg) if tb else None, end=_ij(end))


KINDS = {kind.name: kind for kind in (
    Kind("sw", _sw_result, pairs=("end", "beg"), split=True, withheld=("beg",), plain=("match", "mismatch"),
         sentinel=True),
    Kind("nw", lambda tb, score: dict(score=int(score)), plain=(), band=""),
    Kind("fit", _fit_result, pairs=("beg_end",), split=True),
    Kind("overlap", _overlap_result, pairs=("beg", "end")),
    Kind("extend", _extend_result, pairs=("end",), score2=True, band="_banded", xdrop="_xdrop"),
    # one seed per pair and both of its flanks: a band and an xdrop in every entry
    Kind("seed", _seed_result, pairs=("beg", "end"), band="", xdrop="", extra=("seed_a", "seed_b", "seed_len"),
         flanks=True),
    # (mode, prof, rows) for A; the profile is its own scoring, so there is no matrix and no 32-symbol twin
    Kind("profile", _profile_result, pairs=("beg", "end"), withheld=("beg",), head=("mode", "prof", "rows"),
         matrix=("alphabet", "n_sym")),
)}


_lib = None


def lib() -> C.CDLL:
    """Load libmsa.so (raises if it was not built: the product has no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = _Bind(C.CDLL(str(LIB_PATH)))
    P, sz, i32, i64, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_uint64
    L.msa_status_string.restype = C.c_char_p
    L.msa_status_string.argtypes = [C.c_int]
    L.msa_version.restype = C.c_int
    L.msa_device_count.argtypes = [C.POINTER(C.c_int)]
    L.msa_set_device_budget.argtypes = [C.c_int64]
    L.msa_device_budget_info.argtypes = [C.POINTER(C.c_int64)]
    L.msa_device_memory_info.argtypes = [C.POINTER(C.c_int64)]
    L.msa_main_alignment.argtypes = [P, P, sz, sz, sz, C.c_double, C.c_double, P, sz, C.POINTER(sz),
                                     C.POINTER(C.c_double)]
    L.msa_subproblem.argtypes = [P, P, sz, sz, sz, sz, C.c_int, C.c_int, C.c_double, C.c_double, P, P, P, P, sz,
                                 C.POINTER(sz), P, C.POINTER(C.c_int)]
    L.msa_partial_partition.argtypes = [P, P, sz, sz, sz, C.c_double, C.c_double, C.c_int, C.c_int, P, sz,
                                        C.POINTER(sz)]
    L.msa_partial_tables.argtypes = [P, P, sz, sz, C.c_double, C.c_double, C.c_int, C.c_int, P, P, P, P, P, P]
    L.msa_partition_tables.argtypes = [P, P, P, P, P, P, sz, sz, sz, C.c_double, P, sz, C.POINTER(sz)]
    L.msa_non_parallel_tables.argtypes = [P, P, sz, sz, sz, sz, C.c_int, C.c_int, C.c_double, C.c_double, P, sz,
                                          C.POINTER(sz)]
    L.msa_subproblem_f64.argtypes = [P, P, sz, sz, sz, sz, C.c_int, C.c_double, C.c_double, C.c_int, P, P, P,
                                     C.POINTER(C.c_int)]
    L.msa_subproblem_row.argtypes = [C.c_int, P, P, sz, sz, sz, sz, C.c_int, C.c_double, C.c_double, sz, sz, P, P,
                                     P, P, P, P, P]
    L.msa_optimal_alignment.argtypes = [P, P, sz, sz, sz, C.c_double, C.c_double, P, sz, C.c_int, P, sz,
                                        C.POINTER(sz), P, sz, C.POINTER(sz)]
    L.msa_main_alignment_partitioned.argtypes = [P, P, sz, sz, sz, C.c_double, C.c_double, C.c_int, P, sz,
                                                 C.POINTER(sz)]
    L.msa_plan_create.argtypes = [C.POINTER(PlanDesc), C.POINTER(P)]
    L.msa_plan_create_scored.argtypes = [C.POINTER(PlanDesc), P, C.POINTER(P)]
    L.msa_plan_create_scored32.argtypes = [C.POINTER(PlanDesc), P, C.POINTER(P)]
    L.msa_plan_create_profile.argtypes = [C.POINTER(PlanDesc), P, i64, C.POINTER(P)]
    L.msa_plan_destroy.argtypes = [P]
    L.msa_plan_destroy.restype = None
    L.msa_plan_cells_size.argtypes = [P, C.POINTER(i64)]
    L.msa_plan_run.argtypes = [P, P, P, P, P, P, P]
    L.msa_plan_results.argtypes = [P, P, P]
    L.msa_plan_error.argtypes = [P, C.POINTER(C.c_int), P]
    L.msa_plan_run_info.argtypes = [P, P, P]
    L.msa_plan_launch_info.argtypes = [P, P]
    L.msa_plan_format_info.argtypes = [P, P]
    L.msa_plan_clear_error.argtypes = [P, P]
    L.msa_plan_scores.argtypes = [P, P, P]
    L.msa_plan_stripe_meta.argtypes = [P, P, i64, P]
    L.msa_plan_stripes.argtypes = [P]
    L.msa_plan_stripes.restype = i64
    L.msa_plan_pair_layout.argtypes = [P, i64, C.POINTER(i64)]
    L.msa_plan_checksum.argtypes = [P, P, i64, C.POINTER(u64), P]
    L.msa_plan_traceback.argtypes = [P, i64, P, P, i64, P, P]
    L.msa_plan_traceback_gotoh.argtypes = [P, i64, C.c_int, P, P, i64, P, P]
    L.msa_plan_traceback_nw.argtypes = [P, i64, P, P, i64, P, P]
    L.msa_plan_traceback_batch.argtypes = [P, P, P, P, P, P]
    L.msa_plan_last_kernel_ms.argtypes = [P, C.POINTER(C.c_float)]
    L.msa_plan_set_timing.argtypes = [P, i32]
    L.msa_encode_pair.argtypes = [P, sz, P, sz, P, P]
    L.msa_extend_band_clip.argtypes = [i64, i64, i64, C.POINTER(i64), C.POINTER(i64)]
    L.msa_xdrop_extend_run.argtypes = [P, P, i64, P, P, P, P, P, i32, i32, i32, i32, i32, i32, P, P, P, P]
    L.msa_xdrop_extend_walk.argtypes = [i64, i32, P, P, P, P, P, P, P]
    L.msa_xdrop_flank_run.argtypes = [P, P, i64, P, P, P, P, P, P, i32, i32, i32, i32, i32, i32, P, P, P, P]
    # seed chaining: no alignment kind (no sequences, no CIGAR), bound by hand
    chain = [i32, i32, i32, i64, i64, i32]  # match, gap_open, gap_extend, band, max_dist, lookback
    L.msa_chain_run.argtypes = [P, P, P, i64, P] + chain + [P, P, P, P]
    L.msa_chain_seeds.argtypes = [P, P, P, i64] + chain + [i32, P, P, P, P, P]
    L.msa_chain_seeds_batch.argtypes = [P, P, P, i64, P] + chain + [i32, P, P, P, P, P]
    # the alignment entries: every entry of every kind, from the kind's own argument order
    for kind in KINDS.values():
        for name, slots in kind.entries():
            getattr(L, name).argtypes = [_INT_SLOTS.get(s, P) for s in slots]
    _lib = L.lib
    return _lib


class _Bind:
    """Attribute proxy used while declaring signatures (all symbols must exist)."""

    def __init__(self, lib):
        self.lib = lib

    def __getattr__(self, name):
        return getattr(self.lib, name)


# Every symbol include/msa.h declares (checked by the CPU test suite).
EXPORTED = [
    "msa_status_string", "msa_version", "msa_device_count", "msa_set_device_budget", "msa_device_budget_info", "msa_device_memory_info", "msa_main_alignment", "msa_subproblem",
    "msa_non_parallel_tables", "msa_optimal_alignment", "msa_main_alignment_partitioned",
    "msa_subproblem_f64", "msa_subproblem_row",
    "msa_partial_partition", "msa_partial_tables", "msa_partition_tables", "msa_plan_create", "msa_plan_destroy", "msa_plan_cells_size",
    "msa_plan_run", "msa_plan_results", "msa_plan_error", "msa_plan_run_info", "msa_plan_clear_error", "msa_plan_scores",
    "msa_plan_stripe_meta", "msa_plan_stripes", "msa_plan_pair_layout", "msa_plan_launch_info",
    "msa_plan_format_info",
    "msa_plan_checksum", "msa_plan_traceback", "msa_plan_traceback_gotoh", "msa_plan_traceback_nw",
    "msa_plan_last_kernel_ms", "msa_plan_set_timing", "msa_encode_pair", "msa_sw_align", "msa_nw_align",
    "msa_plan_traceback_batch", "msa_sw_align_batch", "msa_nw_align_batch",
    "msa_plan_create_scored", "msa_nw_align_scored", "msa_nw_align_batch_scored",
    "msa_fit_align", "msa_fit_align_batch",
    "msa_plan_create_scored32", "msa_nw_align_scored32", "msa_nw_align_batch_scored32",
    "msa_fit_align32", "msa_fit_align_batch32",
    "msa_sw_align_scored", "msa_sw_align_batch_scored", "msa_sw_align_scored32", "msa_sw_align_batch_scored32",
    "msa_overlap_align", "msa_overlap_align_batch", "msa_overlap_align32", "msa_overlap_align_batch32",
    "msa_extend_align", "msa_extend_align_batch", "msa_extend_align32", "msa_extend_align_batch32",
    "msa_extend_align_banded", "msa_extend_align_batch_banded", "msa_extend_align_banded32",
    "msa_extend_align_batch_banded32", "msa_extend_band_clip",
    "msa_extend_align_xdrop", "msa_extend_align_batch_xdrop", "msa_extend_align_xdrop32",
    "msa_extend_align_batch_xdrop32", "msa_xdrop_extend_run", "msa_xdrop_extend_walk",
    "msa_plan_create_profile", "msa_profile_align", "msa_profile_align_batch",
    "msa_xdrop_flank_run", "msa_seed_align", "msa_seed_align_batch", "msa_seed_align32", "msa_seed_align_batch32",
    "msa_chain_run", "msa_chain_seeds", "msa_chain_seeds_batch",
]
