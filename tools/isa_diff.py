#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel.

Input: two directories of .s files (hipcc --cuda-device-only -S; build.py
build_asm() writes build/asm and, with diag=True, build/asm_diag).  Functions
are pooled by symbol across the files of a directory, so a kernel that moved
to another translation unit still meets its counterpart.  Per symbol the
instruction lines are compared -- comments stripped, blank lines and
assembler directives dropped, the per-function label numbers .LBB<n>_
normalised to .LBB_ and the module-wide numbers of the long-branch labels
.Lpost_getpc<n> dropped -- and, for kernels, the resource record of the
metadata: .vgpr_count, .agpr_count, .sgpr_count, the spill counts,
.group_segment_fixed_size, .private_segment_fixed_size.

Prints the symbols that differ or exist on one side only; exit status 1 if
there are any.  Text and numbers only: no instruction is looked for.

usage: python tools/isa_diff.py DIR_A DIR_B [--verbose]
"""
import argparse
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_hazards import functions_from_asm  # noqa: E402

RECORD = (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
          ".group_segment_fixed_size", ".private_segment_fixed_size")


def normalise(body):
    out = []
    for line in body:
        line = line.split(";", 1)[0].strip()
        if not line or (line.startswith(".") and not line.startswith((".LBB", ".Lpost_getpc"))):
            continue
        out.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", line)))
    return out


def records(text):
    """{kernel symbol: {key: value}} from the amdhsa.kernels metadata."""
    out, cur = {}, None
    at = text.find("amdhsa.kernels:")
    for line in text[at:].splitlines()[1:] if at >= 0 else []:
        if not line.startswith("  "):
            break
        if line.startswith("  - "):
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"^    (\.\w+):\s*(\S+)\s*$", line)
        if m and cur is not None:
            if m.group(1) == ".name":
                out[m.group(2)] = cur
            elif m.group(1) in RECORD:
                cur[m.group(1)] = m.group(2)
    return out


def load(d):
    funcs, recs = {}, {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        text = open(path).read()
        name = os.path.basename(path)
        for sym, body in functions_from_asm(text).items():
            if sym in funcs:
                raise SystemExit(f"{d}: {sym} is in {funcs[sym][0]} and in {name}")
            funcs[sym] = (name, normalise(body))
        recs.update(records(text))
    return funcs, recs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--verbose", action="store_true", help="the first differing line of each symbol")
    a = ap.parse_args()
    fa, ra = load(a.dir_a)
    fb, rb = load(a.dir_b)
    bad = 0
    for sym in sorted(set(fa) | set(fb)):
        if sym not in fa or sym not in fb:
            side, f = (a.dir_a, fa) if sym in fa else (a.dir_b, fb)
            print(f"only in {side} ({f[sym][0]}): {sym}")
            bad += 1
            continue
        (na, ia), (nb, ib) = fa[sym], fb[sym]
        why = []
        if ia != ib:
            i = next((k for k, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            why.append(f"instructions ({len(ia)} / {len(ib)} lines, first difference at {i})")
            if a.verbose:
                why.append(f"\n    a: {ia[i] if i < len(ia) else '<end>'}\n    b: {ib[i] if i < len(ib) else '<end>'}")
        if ra.get(sym) != rb.get(sym):
            keys = [k for k in RECORD if (ra.get(sym) or {}).get(k) != (rb.get(sym) or {}).get(k)]
            why.append("record " + ", ".join(f"{k} {(ra.get(sym) or {}).get(k)} / {(rb.get(sym) or {}).get(k)}"
                                             for k in keys))
        if why:
            print(f"differs ({na} / {nb}): {sym}: " + "; ".join(why))
            bad += 1
    print(f"{len(fa)} symbols ({len(ra)} kernels) in {a.dir_a}, {len(fb)} ({len(rb)}) in {a.dir_b}: {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
