#!/usr/bin/env python3
"""Static tables of the conv3x3_wino4s builds (the wave-specialised F(4x4) kernel) from a device listing; a sibling of
tools/wino_isa_table.py, whose parser (tools/winog_isa_table.py) it uses:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -S --cuda-device-only csrc/conv_wino4_kernels.hip -o wino4.s
    python tools/wino4s_isa_table.py wino4.s "wino4s<48, 48, true, 48, 1, false>" "wino4s<24, 24, true, 24, 2, false>"

For every pattern: the basic blocks of the PRODUCER wave - laid out behind the consumers: everything from the first block
without an MFMA that issues a whole patch's 36 loads (the first item's) - that hold at least MIN_BLOCK instructions, in
layout order, with their instructions by class:
    mov     v_mov_b32 / v_mov_b64 (a patch copy shows as a block of 36 v_mov_b64)
    and     v_and_b32 (the border masks: 72 per item)
    bits    v_cndmask_b32, v_cmp_*, shifts, v_bfe, v_and_or: in an item's block the select pass that is recomputed per
            item (120 in the parent of round 31, none since); in the blocks that hold `setup` (once per M-tile) the
            tile decode and address arithmetic, 58 or 59
    pk      packed fp32 (v_pk_fma_f32, v_pk_add_f32, v_pk_mul_f32)
    valu    every other vector ALU instruction
    vmem    global / buffer loads
    lds     LDS writes (a ds_write2st64_b64 carries two positions)
    salu    scalar instructions without branches, waits and barriers
and how the block ends (branch targets), so that an item's path - border or interior - can be followed by hand: the
transform is the block with the 144 packed instructions, an item's loads the block with the 36 global loads.  Then
VGPRs / AGPRs / scratch bytes / LDS of EVERY conv3x3_wino4s instantiation, one per line, and for each of them the CONSUMER's
register classes:
    steps     steps (72 MFMAs each) in the basic blocks that hold at least one whole step
    accvgpr   v_accvgpr_* in those blocks (0 with the accumulators in VGPRs and the B operands loaded into AGPRs)
    loads>a   global / buffer loads with an AGPR destination per step (18 streamed, 0 with resident weights),
    loads>v   and those with a VGPR destination (the RAW builds' 18)
    epilogue  v_accvgpr_* / vector ALU instructions in the blocks that store outputs (the epilogues; what a consumer pays
              per M-tile is one of them: guarded, rows-full or general)
    all       v_accvgpr_* of the whole kernel
Counts are static.
"""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from winog_isa_table import kernels  # noqa: E402

MIN_BLOCK = 8
BITS = ("v_cndmask", "v_cmp", "v_lshrrev", "v_bfe", "v_and_or", "v_lshlrev")


def classify(op):
    if op.startswith("v_mov_b"):
        return "mov"
    if op.startswith("v_and_b32"):
        return "and"
    if op.startswith(BITS):
        return "bits"
    if op.startswith("v_pk_"):
        return "pk"
    if op.startswith(("global_load", "buffer_load")):
        return "vmem"
    if op.startswith("ds_write"):
        return "lds"
    if op.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_barrier", "s_nop", "s_endpgm")):
        return "ctl"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    return "other"


def blocks_of(body):
    blocks = [("entry", [])]
    for ln in body:
        s = ln.strip()
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            blocks.append((m.group(1), []))
            continue
        if not s or s[0] in ";.":
            continue
        blocks[-1][1].append(s.split(";")[0].strip())
    return blocks


def registers(text):
    """{mangled name: (VGPRs, AGPRs, scratch bytes, LDS bytes)} from the listing's per-function comments"""
    out = {}
    for m in re.finditer(r"\.Lfunc_end\d+:\n\s*\.size\s+(\S+),.*?; NumVgprs: (\d+)\n; NumAgprs: (\d+).*?; ScratchSize: (\d+).*?"
                         r"; LDSByteSize: (\d+)", text, re.S):
        out[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4, 5))
    return out


def consumer_classes(body):
    """(step blocks, v_accvgpr in them, loads into AGPRs / VGPRs per step block, v_accvgpr / VALU in the storing
    blocks, v_accvgpr in all) of one kernel"""
    blocks = [ins for _, ins in blocks_of(body)]
    acc = lambda ins: sum(s.startswith("v_accvgpr") for s in ins)
    steps = [ins for ins in blocks if sum(s.startswith("v_mfma") for s in ins) >= 72]
    loads = [s for ins in steps for s in ins if s.startswith(("global_load", "buffer_load"))]
    to_a = sum(s.split()[1].startswith("a") for s in loads)
    stores = [ins for ins in blocks if any(s.startswith(("buffer_store_dword", "global_store_dword")) for s in ins)]
    n = max(sum(s.startswith("v_mfma") for ins in steps for s in ins) // 72, 1)      # (a block may hold several steps)
    return (n,sum(acc(ins) for ins in steps), to_a // n, (len(loads) - to_a) // n, sum(acc(ins) for ins in stores),
            sum(classify(s.split()[0]) in ("mov", "and", "bits", "pk", "valu") for ins in stores for s in ins),
            sum(acc(ins) for ins in blocks))


def main():
    funcs, meta, names = kernels(sys.argv[1])
    regs = registers(open(sys.argv[1]).read())
    for pat in sys.argv[2:]:
        for mangled, body in funcs.items():
            if pat not in names[mangled] or "conv3x3_wino4s<" not in names[mangled] or mangled not in meta:
                continue
            print(names[mangled].split("(")[0].replace("void asr::", ""))
            blocks = blocks_of(body)
            first = next(k for k, (_, ins) in enumerate(blocks) if not any(s.startswith("v_mfma") for s in ins) and
                         sum(s.startswith("global_load_dwordx2") for s in ins) >= 36)
            for label, ins in blocks[first:]:
                if len(ins) < MIN_BLOCK:
                    continue
                c = collections.Counter(classify(s.split()[0]) for s in ins)
                ends = [s for s in ins if s.startswith(("s_cbranch", "s_branch"))]
                print("    %-10s %4d  " % (label, len(ins)) +
                      " ".join("%s %d" % (k, c[k]) for k in ("mov", "and", "bits", "pk", "valu", "vmem", "lds", "salu") if c[k]) +
                      ("  barriers %d" % sum(s.startswith("s_barrier") for s in ins) if any(s.startswith("s_barrier") for s in ins) else "") +
                      ("  -> " + ", ".join(e.split()[-1] for e in ends) if ends else ""))
    print("VGPRs / AGPRs / scratch / LDS of every conv3x3_wino4s instantiation")
    for mangled in sorted(funcs, key=lambda k: names[k]):
        if "conv3x3_wino4s<" in names[mangled] and mangled in regs:
            print("    %-48s %3d / %3d / %d / %d" % ((names[mangled].split("(")[0].replace("void asr::conv3x3_", ""),) + regs[mangled]))
    print("consumer register classes: steps / accvgpr in them / loads>a / loads>v per step / epilogue accvgpr / epilogue valu / accvgpr in all")
    for mangled in sorted(funcs, key=lambda k: names[k]):
        if "conv3x3_wino4s<" in names[mangled] and mangled in regs:
            print("    %-48s %d / %d / %d / %d / %d / %d / %d" % ((names[mangled].split("(")[0].replace("void asr::conv3x3_", ""),) +
                                                                 consumer_classes(funcs[mangled])))


if __name__ == "__main__":
    main()
