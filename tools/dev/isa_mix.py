"""Static instruction mix of every loop of one kernel in a hipcc -S listing (developer tool).
usage: isa_mix.py listing.s mangled_kernel_name [resource_remarks.txt]
"dpp" counts the vector instructions that carry a DPP modifier (they are part of "valu" as well).  With the stderr of
hipcc -Rpass-analysis=kernel-resource-usage as the third argument, the kernel's register / scratch / LDS lines are printed too."""
import re
import sys
from collections import Counter

s = open(sys.argv[1]).read()
name = sys.argv[2]
a = s.index("\n" + name + ":")
b = s.index("s_endpgm", a)
body = s[a:b].splitlines()
labels = {}
for i, l in enumerate(body):
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        labels[m.group(1)] = i
loops = []
for i, l in enumerate(body):
    m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        loops.append((labels[m.group(1)], i))


def mix(lines):
    c = Counter()
    for l in lines:
        l = l.strip()
        if not l or l.startswith((".", ";", "//")) or l.endswith(":"):
            continue
        op = l.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith(("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_rcp_iflag")):
            c["trans"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if "_dpp" in op or "quad_perm:" in l or "row_shr:" in l or "row_bcast:" in l:
                c["dpp"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
        elif op.startswith(("global_", "buffer_", "flat_")):
            c["vmem"] += 1
        else:
            c["other"] += 1
    return dict(c)


print("whole kernel:", len(body), mix(body))
for st, en in loops:
    print(f"loop lines {st}..{en} ({en - st}):", mix(body[st:en]))
if len(sys.argv) > 3:
    on = False
    for l in open(sys.argv[3]):
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            on = m.group(1) == name
        m = re.search(r"remark:\s+((?:TotalSGPRs|VGPRs|AGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)[^:]*: \d+)", l)
        if on and m:
            print("resources:", m.group(1))
