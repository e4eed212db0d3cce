"""CPU: the kernels of the page flattening (csrc/page_flatten_kernels.hip) compile for gfx950 without scratch memory and
within 128 VGPRs - the convention of tests/test_register_budgets.py and tests/test_page_deskew_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402

KERNEL = "flatten_pass_kernel"


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_flatten_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "page_flatten_kernels"))
    kernels = {k: v for k, v in fn.items() if KERNEL in k}
    assert len(kernels) == 2, sorted(fn)                             # the dilate and the erode
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 128, (k, vgprs, scratch, inloop)
