"""CPU: the kernel of the FFT spectrogram route (csrc/spectrogram_fft_kernels.hip) compiles for gfx950 without scratch
memory and within 128 VGPRs - a lane keeps its 8 window values and 16 twiddles in registers across its frames, and four
256-thread workgroups per CU (24.5 KB of LDS each) is the occupancy the design counts on; the convention of
tests/test_register_budgets.py and tests/test_resample_budgets.py."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_fft_spectrogram_kernel_uses_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "spectrogram_fft_kernels"))
    kernels = {k: v for k, v in fn.items() if "spectrogram_fft_" in k and "kernel" in k}
    assert any("spectrogram_fft_batch_kernel" in k for k in kernels), sorted(fn)
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and 0 < vgprs <= 128, (k, vgprs, scratch, inloop)
