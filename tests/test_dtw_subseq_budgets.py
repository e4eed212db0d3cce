"""CPU: the kernels of the subsequence DTW (csrc/dtw_subseq_kernels.hip) compile for gfx950 without scratch memory and
within 128 VGPRs - sixteen waves of a 1024-lane workgroup on one CU - the convention of tests/test_register_budgets.py
and tests/test_resample_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_subsequence_dtw_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "dtw_subseq_kernels"))
    kernels = {k: v for k, v in fn.items() if "dtw_subseq_kernel" in k}
    # <pairs of query elements per lane, several waves, reference rows from global memory>
    for name in ("ILi16ELb0ELb0E", "ILi16ELb1ELb0E", "ILi16ELb1ELb1E", "ILi32ELb0ELb0E", "ILi32ELb1ELb0E",
                 "ILi32ELb1ELb1E"):
        assert any("dtw_subseq_kernel" + name in k for k in kernels), (name, sorted(fn))
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 128, (k, vgprs, scratch, inloop)
