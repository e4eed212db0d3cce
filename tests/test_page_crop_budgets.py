"""CPU: the kernels of the page crop (csrc/page_crop_kernels.hip) compile for gfx950 without scratch memory and within
128 VGPRs - the convention of tests/test_register_budgets.py and tests/test_page_flatten_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402

KERNELS = ("crop_counts_kernel", "crop_rects_kernel", "crop_copy_kernel")


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_crop_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "page_crop_kernels"))
    kernels = {k: v for k, v in fn.items() if any(name in k for name in KERNELS)}
    assert len(kernels) == len(KERNELS), sorted(fn)                  # the counts, the rects and the copy
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 128, (k, vgprs, scratch, inloop)
        print(k, vgprs, scratch, inloop)
