"""The non-RAW builds of conv3x3_wino4s run one wave per SIMD: 256 architectural registers plus the accumulators, 512
in all.  Their epilogue exists two or three times (guarded; branch-free for rows-full M-tiles; un-pooled, branch-free
for the other M-tiles too; csrc/wino4_epilogue.h); no copy may push a build over the register file or into scratch.
Compiles the device listing of conv_wino4_kernels.hip for gfx950 (hipcc cross-compiles without a GPU) and reads the
figures of the four builds the headline and the tuner use: 24 -> 48, 48 -> 48, 48 -> 48 pooled, 24 -> 24 pooled."""
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


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wino4_listing") / "conv_wino4_kernels.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-S",
           "--cuda-device-only", "-Wno-comment", "-Wno-unused-result", "-Wno-unused-value",
           os.path.join(ROOT, "audio_sheet_retrieval_amd", "csrc", "conv_wino4_kernels.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as fp:
        return fp.read().split("\n")


def _figures(lines, symbol):
    """(registers in all, scratch bytes, buffer stores, global stores) of one kernel"""
    start = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    tail = lines[end:end + 80]
    num = lambda key: next(int(re.search(r"(\d+)", l.split(":")[1]).group(1)) for l in tail if key in l)
    body = [l.strip() for l in lines[start:end]]
    return (num("; TotalNumVgprs:"), num("; ScratchSize:"), sum(l.startswith("buffer_store_dword") for l in body),
            sum(l.startswith("global_store_dword ") for l in body))


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_inference_builds_fit_the_register_file_without_scratch(build, listing):
    total, scratch, buffer_stores, global_stores = _figures(listing, BUILDS[build])
    print("%s: %d registers, %d B scratch, %d buffer stores, %d global stores" % (build, total, scratch, buffer_stores, global_stores))
    assert scratch == 0, (build, scratch)
    assert total <= 512, (build, total)
    # every epilogue is in the build, one store per value each (4 tiles x 16 outputs, or 4 x 4 pooled): the guarded one,
    # the rows-full one and, un-pooled, the general branch-free form
    per_mtile = 16 if "pooled" in build else 64
    assert global_stores == per_mtile, (build, global_stores)
    assert buffer_stores == (per_mtile if "pooled" in build else 2 * per_mtile), (build, buffer_stores)
