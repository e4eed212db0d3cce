"""CPU: the kernels of the running vote for parallel streams (csrc/track_stream_kernels.hip) compile for gfx950 without
scratch memory and without reloads inside their loops - the convention of tests/test_track_budgets.py.  The VGPR counts
are the ones of the listing (docs/MEASUREMENT_LOG.md, round 25), pinned so that a later spill or a lost bound shows."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402

VGPRS = {"track_stream_colsum_kernel": 16, "track_stream_gate_kernel": 62, "track_stream_window_kernel": 8,
         "track_stream_tail_kernel": 17, "track_stream_vote_kernelILb0E": 42, "track_stream_vote_kernelILb1E": 30,
         "track_stream_ring_kernel": 21}


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_stream_tracking_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "track_stream_kernels"))
    kernels = {k: v for k, v in fn.items() if "track_stream_" in k and "kernel" in k}
    assert len(kernels) == len(VGPRS), sorted(fn)
    for name, pinned in VGPRS.items():
        found = [v for k, v in kernels.items() if name in k]
        assert len(found) == 1, (name, sorted(fn))
        vgprs, scratch, inloop = found[0]
        assert scratch == 0 and inloop == 0, (name, vgprs, scratch, inloop)
        assert vgprs == pinned, (name, vgprs, pinned)
