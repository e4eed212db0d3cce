"""The consumers of the non-RAW conv3x3_wino4s builds keep their accumulators in architectural VGPRs and their B operands
in AGPRs (inline assembly; csrc/conv_wino4_kernels.hip): the epilogue reads the accumulators where they are and the
weights are loaded where nothing else needs the space - all 216 of a lane at C_in = 24, once per workgroup.  A compiler
that answers the register pressure with copies between the two files, or a change that brings the weight loads back
into the resident builds' M-tile loop, leaves every result as it was; the device listing shows it.  Compiled for gfx950
as in tests/test_wino4_register_budgets.py (hipcc cross-compiles without a GPU), for the same four builds."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# <CIN, COUT, POOL, SLICE = COUT, PW = 1, RAW = false>
BUILDS = {
    "24->48": "_ZN3asr14conv3x3_wino4sILi24ELi48ELb0ELi48ELi1ELb0EEEvNS_9Wino4ArgsE",
    "48->48": "_ZN3asr14conv3x3_wino4sILi48ELi48ELb0ELi48ELi1ELb0EEEvNS_9Wino4ArgsE",
    "48->48 pooled": "_ZN3asr14conv3x3_wino4sILi48ELi48ELb1ELi48ELi1ELb0EEEvNS_9Wino4ArgsE",
    "24->24 pooled": "_ZN3asr14conv3x3_wino4sILi24ELi24ELb1ELi24ELi1ELb0EEEvNS_9Wino4ArgsE",
}
RESIDENT = ("24->48", "24->24 pooled")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wino4_listing") / "conv_wino4_kernels.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-S",
           "--cuda-device-only", "-Wno-comment", "-Wno-unused-result", "-Wno-unused-value",
           os.path.join(ROOT, "audio_sheet_retrieval_amd", "csrc", "conv_wino4_kernels.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as fp:
        return fp.read().split("\n")


def _kernel(lines, symbol):
    """(basic blocks as lists of instructions, registers in all, scratch bytes) of one kernel"""
    start = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    tail = lines[end:end + 80]
    num = lambda key: next(int(re.search(r"(\d+)", l.split(":")[1]).group(1)) for l in tail if key in l)
    blocks = [[]]
    for l in lines[start + 1:end]:
        s = l.strip()
        if re.match(r"^\.LBB\w+:", s):
            blocks.append([])
        elif s and s[0] not in ";.":
            blocks[-1].append(s.split(";")[0].strip())
    return blocks, num("; TotalNumVgprs:"), num("; ScratchSize:")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_accumulators_in_vgprs_and_weights_in_agprs(build, listing):
    blocks, total, scratch = _kernel(listing, BUILDS[build])
    count = lambda ins, prefix: sum(s.startswith(prefix) for s in ins)
    steps = [ins for ins in blocks if count(ins, "v_mfma") >= 72]
    stores = [ins for ins in blocks if count(ins, "buffer_store_dword")]
    print("%s: %d registers, %d B scratch; step blocks (MFMAs, v_accvgpr, loads): %s; %d storing blocks with %d v_accvgpr_read" % (
        build, total, scratch, [(count(i, "v_mfma"), count(i, "v_accvgpr"), count(i, "global_load") + count(i, "buffer_load")) for i in steps],
        len(stores), sum(count(i, "v_accvgpr_read") for i in stores)))
    assert scratch == 0, (build, scratch)
    assert total <= 512, (build, total)
    assert steps, "no basic block holds a whole 72-MFMA step"
    assert sum(count(i, "v_mfma") for i in blocks) == sum(count(i, "v_mfma") for i in steps), "MFMAs outside the step blocks"
    for ins in steps:
        assert count(ins, "v_accvgpr") == 0, (build, [s for s in ins if s.startswith("v_accvgpr")][:4])
        # the MFMA itself: C/D in VGPRs, B from an AGPR
        for s in ins:
            if s.startswith("v_mfma"):
                ops = [o.strip() for o in s.split(None, 1)[1].split(",")]
                assert ops[0].startswith("v[") and ops[2].startswith("a") and (ops[3] == "0" or ops[3].startswith("v[")), s
        if build in RESIDENT:
            assert count(ins, "global_load") + count(ins, "buffer_load") == 0, (build, [s for s in ins if "_load" in s][:4])
        else:
            loads = [s for s in ins if s.startswith(("global_load", "buffer_load"))]
            assert loads and all(s.split()[1].startswith("a[") for s in loads), (build, loads[:4])
    assert stores, "no epilogue found"
    for ins in stores:
        assert count(ins, "v_accvgpr_read") == 0, (build, [s for s in ins if s.startswith("v_accvgpr_read")][:4])
