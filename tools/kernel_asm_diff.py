#!/usr/bin/env python3
"""Compare two sets of `hipcc -S --cuda-device-only` assembly files kernel by kernel (development tool): A.s [A2.s ...] -- B.s [B2.s ...]
(or just A.s B.s).  A side's kernels are those of all its files: a source that was split is compared with the files it was split into.

Per kernel: the metadata (VGPR, SGPR, LDS, private segment, spills), the number of instructions and the histogram of mnemonics.  Prints one line
per kernel: `same` (instruction for instruction), `reordered` (equal metadata and histogram), or the figures of both sides."""
import collections
import re
import sys

KEYS = ["vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"]


def kernels_of(path):
    txt = open(path).read()
    out = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.symbol:\s+(\S+)\.kd", blk).group(1)
        out[name] = {"meta": [int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in KEYS]}
    for name, k in out.items():
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M).group(1)
        # (a local label carries the ordinal of its function in the file, .LBB<function>_<block>: dropped, so that a kernel that moved to another file compares equal)
        k["ins"] = [re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", ln.split(";")[0].strip()) for ln in body.split("\n") if re.match(r"\s+[a-z]\w+", ln)]
        k["hist"] = collections.Counter(i.split()[0] for i in k["ins"])
    return out


def kernels(paths):
    out = {}
    for path in paths:
        for name, k in kernels_of(path).items():
            if name in out:
                sys.exit(f"{name}: in more than one file of a side ({path})")
            out[name] = k
    return out


args = sys.argv[1:]
cut = args.index("--") if "--" in args else 1
a, b = kernels(args[:cut]), kernels([f for f in args[cut:] if f != "--"])
for name in sorted(set(a) | set(b)):
    short = re.sub(r"^_ZN2fy(2gr)?12_GLOBAL__N_1\d+", "", name)[:56]
    if name not in a or name not in b:
        print(f"{short:58s} only in {'A' if name in a else 'B'}")
        continue
    x, y = a[name], b[name]
    if x["meta"] == y["meta"] and x["ins"] == y["ins"]:
        print(f"{short:58s} same       {len(x['ins'])}")
    elif x["meta"] == y["meta"] and x["hist"] == y["hist"]:
        print(f"{short:58s} reordered  {len(x['ins'])}")
    else:
        print(f"{short:58s} DIFFERS    instructions {len(x['ins'])} -> {len(y['ins'])} ({100.0 * (len(y['ins']) - len(x['ins'])) / len(x['ins']):+.2f} %)  "
              f"[vgpr, sgpr, lds, private, vgpr spills, sgpr spills] {x['meta']} -> {y['meta']}")
