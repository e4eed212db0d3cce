"""CPU: the kernels of the resampler (csrc/resample_kernels.hip) compile for gfx950 without scratch memory and within
128 VGPRs (four 256-thread workgroups per CU and more) - the convention of tests/test_register_budgets.py and
tests/test_omr_detect_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_resampling_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "resample_kernels"))
    kernels = {k: v for k, v in fn.items() if "resample_" in k and "kernel" in k}
    for name in ("resample_batch_kernelILb0E", "resample_batch_kernelILb1E"):      # gathered taps / one phase (up == 1)
        assert any(name in k for k in kernels), (name, sorted(fn))
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 128, (k, vgprs, scratch, inloop)
