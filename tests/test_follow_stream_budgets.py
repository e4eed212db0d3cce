"""CPU: the kernels of score following for parallel streams (csrc/follow_stream_kernels.hip) compile for gfx950 without
scratch memory, without reloads inside their loops and within 128 VGPRs - the convention of
tests/test_dtw_follow_budgets.py and tests/test_track_stream_budgets.py.  They only move floats, so the bound is far
from what they use; a spill or a lost launch bound would still show here."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402

KERNELS = ["follow_stream_window_kernel", "follow_stream_tail_kernel", "follow_stream_log_kernel"]


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_stream_following_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "follow_stream_kernels"))
    kernels = {k: v for k, v in fn.items() if "follow_stream_" in k and "kernel" in k}
    assert len(kernels) == len(KERNELS), sorted(fn)
    for name in KERNELS:
        found = [v for k, v in kernels.items() if name in k]
        assert len(found) == 1, (name, sorted(fn))
        vgprs, scratch, inloop = found[0]
        assert scratch == 0 and inloop == 0, (name, vgprs, scratch, inloop)
        assert 0 < vgprs <= 128, (name, vgprs)
