"""CPU: the kernel of the page resize (csrc/page_resize_kernels.hip) compiles for gfx950 without scratch memory and within
128 VGPRs - the convention of tests/test_register_budgets.py and tests/test_resample_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_page_resize_kernel_uses_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "page_resize_kernels"))
    kernels = {k: v for k, v in fn.items() if "resize_pages_kernel" in k}
    assert kernels, sorted(fn)
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 128, (k, vgprs, scratch, inloop)
