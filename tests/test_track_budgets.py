"""CPU: the kernels of the running vote (csrc/track_kernels.hip) compile for gfx950 without scratch memory - the
convention of tests/test_register_budgets.py and tools/scratch_scan.sh."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_tracking_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "track_kernels"))
    kernels = {k: v for k, v in fn.items() if "track_" in k and "kernel" in k}
    for name in ("track_colsum_kernel", "track_level_kernel", "track_gate_kernel", "track_vote_kernelILb0E",
                 "track_vote_kernelILb1E"):
        assert any(name in k for k in kernels), (name, sorted(fn))
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 64, (k, vgprs, scratch, inloop)
