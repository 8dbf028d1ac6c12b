#!/usr/bin/env python3
"""Developer: are the functions of two device listings the same text?   isa_same.py parent.s new.s [name-filter-regex]
(listings: build.sh's FLAGS + -S --cuda-device-only).  A function is compared from its .type line to the end of its resource
comments, .amdhsa_* descriptor included; labels that number a function by its position in the file are normalised, runs of blanks too.  One line per
symbol: same | differs | only in <file>.  Exit status 1 if a symbol that both files have differs."""
import re
import subprocess
import sys

POSITIONAL = re.compile(r"\.?L?BB\d+_|\.Lfunc_(?:begin|end)\d+|\.Ltmp\d+|__hip_cuid_\w+")


def functions(path):
    out, name, done = {}, None, False
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, done = m.group(1), False
            out[name] = []
        elif name and done and re.match(r"\s*\.(text|section\s+\.text|section\s+\.AMDGPU\.gpr_maximums|type|amdgpu_metadata|ident)\b", line):
            name = None                       # the next function's (or the file's) own lines
        if name:
            out[name].append(" ".join(POSITIONAL.sub("@", line).split()))      # (comment columns move with a label's length)
            done = done or "-- End function" in line
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    keep = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
    names = list(dict.fromkeys(list(a) + list(b)))
    nice = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    bad = 0
    for sym, shown in zip(names, nice):
        if keep and not keep.search(shown):
            continue
        what = "same" if a.get(sym) == b.get(sym) else f"only in {sys.argv[2 if sym in b else 1]}" if (sym in a) != (sym in b) else "differs"
        bad += what == "differs"
        print(f"{what:8s} {shown}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
