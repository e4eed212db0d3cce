"""CPU: the kernels of the streamed audio front-end (csrc/audio_stream_kernels.hip) compile for gfx950 without scratch
memory and within 128 VGPRs - the convention of tests/test_register_budgets.py and tests/test_resample_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_stream_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "audio_stream_kernels"))
    kernels = {k: v for k, v in fn.items() if "audio_stream_" in k and "kernel" in k}
    # gathered taps / one phase (up == 1, also the front-end's own rate) / the state's slide
    for name in ("audio_stream_frame_kernelILb0E", "audio_stream_frame_kernelILb1E", "audio_stream_carry_kernel"):
        assert any(name in k for k in kernels), (name, sorted(fn))
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and vgprs <= 128, (k, vgprs, scratch, inloop)
