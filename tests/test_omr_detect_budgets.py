"""CPU: the kernels of bar and note-head detection (csrc/omr_detect_kernels.hip) compile for gfx950 without scratch
memory - the convention of tests/test_register_budgets.py and tests/test_track_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_detection_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "omr_detect_kernels"))
    kernels = {k: v for k, v in fn.items() if "det_" in k and "kernel" in k}
    for name in ("det_minmax_kernel", "det_status_kernel", "det_peak_kernel", "det_rowcount_kernelILb0E",
                 "det_rowcount_kernelILb1E", "det_rowscan_kernel", "det_emit_kernelILb0E", "det_emit_kernelILb1E",
                 "det_edges_kernel", "det_hist_kernel", "det_otsu_kernel", "det_fg_label_kernel", "det_stats_kernel"):
        assert any(name in k for k in kernels), (name, sorted(fn))
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 64, (k, vgprs, scratch, inloop)
