#!/usr/bin/env python3
"""Static instruction table of conv3x3_winog builds from a device listing:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -S --cuda-device-only csrc/conv_wino_kernels.hip -o wino.s
    python tools/winog_isa_table.py wino.s "winog<24, 24, true, 2, 8, 2" "winog<12, 24, false, 2, 4, 2"

Per kernel: instructions in all; the basic block of the channel-block loop that holds its MFMAs (instructions, MFMAs,
v_add_u32 standing between two MFMAs, LDS reads by kind); v_mov_b64, zero clears (v_mov_b32 v, 0), v_cndmask and
packed adds of the whole kernel; registers and scratch bytes.  Counts are static: code on both sides of a branch is
counted once.
"""
import collections
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S):
        out[m.group(1)] = m.group(2).split("\n")
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        g = lambda k: int(re.search(r"\." + k + r" (\d+)", m.group(2)).group(1))
        meta[m.group(1)] = (g("amdhsa_next_free_vgpr"), g("amdhsa_private_segment_fixed_size"))
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return out, meta, dict(zip(names, dem))


def table(body):
    blocks = [[]]
    for ln in body:
        s = ln.strip()
        if re.match(r"^\.LBB\w+:", s):
            blocks.append([])
            continue
        if not s or s[0] in ";.":
            continue
        blocks[-1].append(s.split(";")[0].strip())
    ins = [s for b in blocks for s in b]
    ops = collections.Counter(s.split()[0] for s in ins)
    mb = max(blocks, key=lambda b: sum(s.startswith("v_mfma") for s in b))
    mf = [k for k, s in enumerate(mb) if s.startswith("v_mfma")]
    lds = collections.Counter(s.split()[0] for s in mb if s.startswith("ds_read"))
    return dict(total=len(ins), mfma_block=len(mb), mfmas=len(mf),
                adds_between=sum(1 for k, s in enumerate(mb) if mf[0] < k < mf[-1] and s.startswith("v_add_u32")),
                lds_reads=dict(lds), mov_b64=ops["v_mov_b64_e32"],
                clears=sum(bool(re.match(r"v_mov_b32_e32 v\d+, 0$", s)) for s in ins),
                cndmask=ops["v_cndmask_b32_e64"] + ops["v_cndmask_b32_e32"], pk_add=ops["v_pk_add_f32"])


def main():
    funcs, meta, names = kernels(sys.argv[1])
    for pat in sys.argv[2:]:
        for mangled, body in funcs.items():
            if pat in names[mangled] and mangled in meta:
                print(names[mangled].split("(")[0].replace("void asr::", ""))
                print("   ", table(body), "registers %d scratch %d" % meta[mangled])


if __name__ == "__main__":
    main()
