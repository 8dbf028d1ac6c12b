#!/usr/bin/env python3
"""Developer: what every kernel of a hipcc -S listing does AFTER its last MFMA (its epilogue) — or, for a kernel without MFMAs,
in its whole body.   isa_tail.py listing.s [name-filter-regex]
(listing: build.sh's FLAGS + -S --cuda-device-only).  One line per kernel: instructions, vector-memory loads, vector-memory
stores, s_waitcnt that name vmcnt, of which vmcnt(0), and branches.  An epilogue that is a per-element chain load -> wait ->
store shows as about as many vmcnt(0) as stores: vmcnt counts the stores as well, so each such wait drains the store in front of
it besides the load it is there for."""
import re
import subprocess
import sys

VMEM = ("global_", "buffer_", "flat_", "scratch_")


def kernels(path):
    """name -> instruction lines, for the symbols that end in s_endpgm (device functions that were not inlined are skipped)"""
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            name = m.group(1)
            out[name] = []
            continue
        t = line.strip()
        if name is None or not t or t.startswith((".", ";", "//")) or re.match(r"^\.?\w+:", t):
            continue
        out[name].append(t)
        if t.startswith("s_endpgm"):
            name = None
    return {k: v for k, v in out.items() if v and v[-1].startswith("s_endpgm")}


def tail_counts(lines):
    last = max((i for i, t in enumerate(lines) if t.startswith("v_mfma")), default=-1)
    tail = lines[last + 1:]
    c = {"mfma": sum(t.startswith("v_mfma") for t in lines), "instr": len(tail), "loads": 0, "stores": 0, "vmcnt": 0, "vmcnt0": 0,
         "branches": 0}
    for t in tail:
        op = t.split()[0]
        if op.startswith(VMEM):
            if "_load" in op:
                c["loads"] += 1
            elif "_store" in op:
                c["stores"] += 1
        elif op == "s_waitcnt" and "vmcnt" in t:
            c["vmcnt"] += 1
            c["vmcnt0"] += bool(re.search(r"vmcnt\(0\)", t))
        elif op.startswith(("s_cbranch", "s_branch")):
            c["branches"] += 1
    return c


def main():
    ks = kernels(sys.argv[1])
    keep = re.compile(sys.argv[2]) if len(sys.argv) > 2 else None
    names = list(ks)
    nice = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    print(f"{'after the last MFMA: instr':>26s} {'loads':>6s} {'stores':>6s} {'vmcnt':>6s} {'vmcnt(0)':>8s} {'branch':>6s}  kernel (MFMAs)")
    for sym, shown in zip(names, nice):
        shown = re.sub(r"^void ", "", shown.split("(")[0])
        if keep and not keep.search(shown):
            continue
        c = tail_counts(ks[sym])
        print(f"{c['instr']:26d} {c['loads']:6d} {c['stores']:6d} {c['vmcnt']:6d} {c['vmcnt0']:8d} {c['branches']:6d}  {shown} ({c['mfma']})")


if __name__ == "__main__":
    main()
