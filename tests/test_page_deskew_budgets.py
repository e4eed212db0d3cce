"""CPU: the kernels of the skew estimate and the shear (csrc/page_deskew_kernels.hip) compile for gfx950 without scratch
memory and within 128 VGPRs - the convention of tests/test_register_budgets.py and tests/test_page_resize_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402

KERNELS = ("skew_profiles_kernel", "skew_scores_kernel", "skew_select_kernel", "deskew_pages_kernel")


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_deskew_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "page_deskew_kernels"))
    for name in KERNELS:
        kernels = {k: v for k, v in fn.items() if name in k}
        assert kernels, (name, sorted(fn))
        for k, (vgprs, scratch, inloop) in kernels.items():
            assert scratch == 0 and inloop == 0 and vgprs <= 128, (k, vgprs, scratch, inloop)
