"""Do two builds of libmsa.so hold the same gfx950 code?  Compares, function by function, the disassembled
(mnemonic, operands) streams (normalise: all but where the function sits), and kernel by kernel the code-object metadata rows (registers,
scratch, spills, LDS, arguments).  Exit status 1 if anything differs.

    python scripts/isa_diff.py old/libmsa.so new/libmsa.so
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from kmeta import kernels  # noqa: E402
from waitloops import disassemble, functions  # noqa: E402


def normalise(insts):
    """A function's (mnemonic, operands) stream without what only says where it sits in the file: the s_nop padding
    behind its last s_endpgm / s_setpc_b64 / s_branch, and the pc-relative literals of the s_add_u32, s_addc_u32
    behind an s_getpc_b64 (the address of a called function)."""
    out = [(mn, ops) for _, mn, ops in insts]
    ends = [i for i, (mn, _) in enumerate(out) if mn in ("s_endpgm", "s_setpc_b64", "s_branch")]
    if ends and all(mn == "s_nop" for mn, _ in out[ends[-1] + 1:]):
        del out[ends[-1] + 1:]
    for i in range(len(out) - 2):
        if [mn for mn, _ in out[i:i + 3]] == ["s_getpc_b64", "s_add_u32", "s_addc_u32"]:
            out[i + 1:i + 3] = [(mn, ops.rsplit(",", 1)[0] + ", <pcrel> ") for mn, ops in out[i + 1:i + 3]]
    return out


def streams(so: Path):
    return {name: normalise(insts) for name, insts in functions(disassemble(so)).items()}


def rows(so: Path):
    return {k.get("symbol", k.get("name")): k for k in kernels(so)}


def report(title, items):
    print(f"{title}: {len(items)}")
    for it in items:
        print(f"    {it}")
    return len(items)


def main(old: Path, new: Path) -> int:
    fo, fn, ko, kn = streams(old), streams(new), rows(old), rows(new)
    both = sorted(fo.keys() & fn.keys())
    print(f"functions in both: {len(both)}; kernels in both: {len(ko.keys() & kn.keys())}")
    bad = report("functions only in old", sorted(fo.keys() - fn.keys()))
    bad += report("functions only in new", sorted(fn.keys() - fo.keys()))
    bad += report("functions whose instruction stream differs",
                  [f"{len(fo[f])} -> {len(fn[f])} instructions  {f[:120]}" for f in both if fo[f] != fn[f]])
    bad += report("kernels only in one", sorted(ko.keys() ^ kn.keys()))
    bad += report("kernels whose metadata differs",
                  [f"{k[:100]}: " + ", ".join(f"{f} {ko[k].get(f)} -> {kn[k].get(f)}"
                                              for f in sorted(ko[k].keys() | kn[k].keys()) if ko[k].get(f) != kn[k].get(f))
                   for k in sorted(ko.keys() & kn.keys()) if ko[k] != kn[k]])
    print("IDENTICAL" if not bad else f"DIFFERENT ({bad} findings)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(Path(sys.argv[1]), Path(sys.argv[2])))
