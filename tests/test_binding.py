"""The Python binding of the alignment entries: _lib.KINDS declares each kind once, and both the argtypes and api.py's
calls come from it.  CPU only: the signatures against include/msa.h, and every kind's call as far as the device."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT

# a declaration's parameter type -> what its argtypes element must be ("ptr": any pointer type)
C_TYPES = {"size_t": C.c_size_t, "int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}
NODEV = -4


def _declarations():
    """{name: [parameter type, ...]} of every alignment entry include/msa.h declares."""
    hdr = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "msa.h").read_text(), flags=re.S)
    decl = {}
    for name, params in re.findall(r"^\s*(?:[A-Za-z_][\w\s\*]*?)\b(msa_\w+_align\w*)\s*\(([^)]*)\)\s*;", hdr, re.M):
        types = []
        for p in params.split(","):
            ty = re.sub(r"\bconst\b", "", p).strip()
            ty = re.match(r"(.*?)\s*\w+$", ty, re.S).group(1).replace(" ", "")  # drop the parameter's name
            types.append("ptr" if ty.endswith("*") else ty)
        decl[name] = types
    return decl


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer)


def test_alignment_argtypes_match_the_header():
    """Every msa_*_align* entry is bound with as many argtypes as its declaration has parameters, a pointer where it
    declares a pointer and the integer (or floating) type of the same width and sign elsewhere."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    decl = _declarations()
    assert len(decl) >= 30
    assert {"msa_sw_align", "msa_extend_align_batch_banded32", "msa_profile_align_batch"} <= set(decl)
    L = LB.lib()
    for name, types in sorted(decl.items()):
        argtypes = getattr(L, name).argtypes
        assert argtypes is not None and len(argtypes) == len(types), name
        for pos, (ty, got) in enumerate(zip(types, argtypes)):
            if ty == "ptr":
                assert _is_pointer(got), (name, pos, got)
            else:
                assert got is C_TYPES[ty], (name, pos, ty, got)


A5 = b"ACGTA"
B7 = b"GATTACA"
DNA = np.where(np.eye(4, dtype=bool), 2, -1)
PROFILE = np.arange(20).reshape(5, 4) - 8

# (function, positional arguments, keywords, the C entry that must be reached): one valid call per kind, single and
# batch, and one per suffix combination
CALLS = [
    ("sw_align", (A5, B7), {}, "msa_sw_align"),
    ("sw_align_batch", ([A5, A5], [B7, B7]), {}, "msa_sw_align_batch"),
    ("nw_align", (A5, B7), {}, "msa_nw_align"),
    ("nw_align_batch", ([A5, A5], B7), {}, "msa_nw_align_batch"),
    ("fit_align", (A5, B7), {}, "msa_fit_align"),
    ("fit_align_batch", ([A5, A5], [B7, B7]), {}, "msa_fit_align_batch"),
    ("overlap_align", (A5, B7), {}, "msa_overlap_align"),
    ("overlap_align_batch", ([A5, A5], B7), {}, "msa_overlap_align_batch"),
    ("extend_align", (A5, B7), {}, "msa_extend_align"),
    ("extend_align_batch", ([A5, A5], [B7, B7]), {}, "msa_extend_align_batch"),
    ("profile_align", (PROFILE, B7, b"ACGT"), {}, "msa_profile_align"),
    ("profile_align_batch", (PROFILE, [B7, B7], b"ACGT"), {"mode": "fit"}, "msa_profile_align_batch"),
    ("sw_align", (A5, B7), {"alphabet": b"ACGT", "matrix": DNA}, "msa_sw_align_scored"),
    ("sw_align_batch", ([A5], B7), {"max_symbols": 32, "traceback": False}, "msa_sw_align_batch_scored32"),
    ("nw_align", (A5, B7), {"match": 2, "band": 3}, "msa_nw_align_scored"),
    ("nw_align_batch", ([A5], [B7]), {"max_symbols": 32}, "msa_nw_align_batch_scored32"),
    ("fit_align", (A5, B7), {"max_symbols": 32, "traceback": False}, "msa_fit_align32"),
    ("overlap_align_batch", ([A5], [B7]), {"max_symbols": 32, "traceback": False}, "msa_overlap_align_batch32"),
    ("extend_align", (A5, B7), {"max_symbols": 32}, "msa_extend_align32"),
    ("extend_align", (A5, B7), {"band": 3, "traceback": False}, "msa_extend_align_banded"),
    ("extend_align_batch", ([A5, A5], B7), {"band": 3}, "msa_extend_align_batch_banded"),
    ("extend_align", (A5, B7), {"band": 0, "max_symbols": 32}, "msa_extend_align_banded32"),
    ("extend_align_batch", ([A5], [B7]), {"band": 3, "max_symbols": 32}, "msa_extend_align_batch_banded32"),
]


@pytest.mark.parametrize("fn, args, kw, entry", CALLS, ids=[f"{c[3]}-{i}" for i, c in enumerate(CALLS)])
def test_valid_call_reaches_the_device_check(fn, args, kw, entry):
    """Without a GPU every entry returns its argument errors before it asks for a device, so a well-formed call -- one
    that got past every host-side check of the library -- ends in MSA_ERR_NODEV, reported under the C entry's name."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from cse305_parallel_sequence_alignment_amd import api, MsaError

    with pytest.raises(MsaError) as e:
        getattr(api, fn)(*args, **kw)
    assert e.value.status == NODEV
    assert str(e.value).startswith(entry + ":")
