#!/usr/bin/env python3
"""Static tables of the conv3x3_wino builds (the LDS-patch Winograd kernel) from a device listing; a sibling of
tools/winog_isa_table.py, whose parser it uses:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -S --cuda-device-only csrc/conv_wino_kernels.hip -o wino.s
    python tools/wino_isa_table.py wino.s "wino<12, 12, true, 1, 1, 4, 3, 8, false, 0" "wino<12, 24, false, 2, 1, 8, 2, 6, false, 0"

For every pattern: the basic block that holds the M-tile's MFMAs (MFMAs, LDS reads by kind, s_waitcnt, v_add_u32
between the first and the last MFMA).  Then registers and scratch bytes of EVERY conv3x3_wino instantiation, one per
line.  Counts are static: code on both sides of a branch is counted once.
"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from winog_isa_table import kernels, table  # noqa: E402


def mtile_block(body):
    blocks = [[]]
    for ln in body:
        s = ln.strip()
        if s.startswith(".LBB") and s.split(";")[0].strip().endswith(":"):
            blocks.append([])
            continue
        if not s or s[0] in ";.":
            continue
        blocks[-1].append(s.split(";")[0].strip())
    return max(blocks, key=lambda b: sum(s.startswith("v_mfma") for s in b))


def main():
    funcs, meta, names = kernels(sys.argv[1])
    for pat in sys.argv[2:]:
        for mangled, body in funcs.items():
            if pat in names[mangled] and "conv3x3_wino<" in names[mangled] and mangled in meta:
                t = table(body)
                mb = mtile_block(body)
                reads = collections.Counter(s.split()[0] for s in mb if s.startswith("ds_read"))
                print(names[mangled].split("(")[0].replace("void asr::", ""))
                print("    MFMA %d  LDS reads %d %s  s_waitcnt %d  v_add_u32 between MFMAs %d  block %d instructions" %
                      (t["mfmas"], sum(reads.values()), dict(reads), sum(s.startswith("s_waitcnt") for s in mb),
                       t["adds_between"], len(mb)))
    print("registers / scratch of every conv3x3_wino instantiation")
    for mangled in sorted(funcs, key=lambda k: names[k]):
        if "conv3x3_wino<" in names[mangled] and mangled in meta:
            print("    %-70s %3d / %d" % (names[mangled].split("(")[0].replace("void asr::conv3x3_", ""), *meta[mangled]))


if __name__ == "__main__":
    main()
