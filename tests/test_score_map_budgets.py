"""CPU: the kernels of the score map (csrc/score_map_kernels.hip) compile for gfx950 without scratch memory and within 64
VGPRs - they hold a count, a flag word and a few indices per lane, so half of what tests/test_page_flatten_budgets.py
allows its tiles is the stated bound; the convention of tests/test_register_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402

KERNELS = ("score_map_counts_kernel", "score_map_lines_kernel", "score_map_table_kernel")


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_score_map_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "score_map_kernels"))
    kernels = {k: v for k, v in fn.items() if any(name in k for name in KERNELS)}
    assert len(kernels) == 3, sorted(fn)
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 64, (k, vgprs, scratch, inloop)
