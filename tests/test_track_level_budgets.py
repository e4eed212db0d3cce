"""CPU: the kernels of the running music gate (csrc/track_level_kernels.hip) compile for gfx950 without scratch memory
and within the 64 VGPRs their siblings keep - the convention of tests/test_track_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402

KERNELS = ("track_level_suffix_kernel", "track_level_prefix_kernel", "track_level_state_kernel",
           "track_gate_running_kernel", "track_stream_gate_running_kernel")


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_level_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "track_level_kernels"))
    kernels = {k: v for k, v in fn.items() if "track_" in k and "kernel" in k}
    for name in KERNELS:
        assert any(name in k for k in kernels), (name, sorted(fn))
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 64, (k, vgprs, scratch, inloop)
