"""CPU: the kernels of the streaming subsequence DTW (csrc/dtw_follow_kernels.hip) compile for gfx950 without scratch
memory and within 128 VGPRs - sixteen waves of a 1024-lane workgroup on one CU - the convention of
tests/test_dtw_subseq_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_follow_dtw_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "dtw_follow_kernels"))
    kernels = {k: v for k, v in fn.items() if "dtw_follow_kernel" in k}
    # <pairs of query elements per lane, several waves, reference rows from global memory>
    names = ("ILi16ELb0ELb0E", "ILi16ELb1ELb0E", "ILi16ELb1ELb1E", "ILi32ELb0ELb0E", "ILi32ELb1ELb0E", "ILi32ELb1ELb1E")
    for name in names:
        assert any("dtw_follow_kernel" + name in k for k in kernels), (name, sorted(fn))
    assert len(kernels) == len(names), sorted(kernels)
    for k, (vgprs, scratch, inloop) in kernels.items():
        print(k, vgprs, scratch, inloop)
        assert scratch == 0 and inloop == 0 and vgprs <= 128, (k, vgprs, scratch, inloop)
