"""CPU: the kernels of the streamed FFT front-end (csrc/audio_stream_fft_kernels.hip) compile for gfx950 without scratch
memory and within 128 VGPRs - the convention of tests/test_register_budgets.py and tests/test_audio_stream_budgets.py -
and asr_audio_stream_push_fft_dev is declared with asr_audio_stream_push_dev's parameter list and exported (the means of
tests/test_abi.py)."""
import ctypes
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_register_budgets as budgets  # noqa: E402


@pytest.mark.skipif(shutil.which(budgets.HIPCC) is None and not os.path.exists(budgets.HIPCC), reason="hipcc not available")
def test_the_stream_fft_kernels_use_no_scratch(tmp_path):
    fn = budgets._functions(budgets._listing(tmp_path, "audio_stream_fft_kernels"))
    kernels = {k: v for k, v in fn.items() if "audio_stream_fft_" in k and "kernel" in k}
    # gathered taps / one phase (up == 1, also the front-end's own rate)
    for name in ("audio_stream_fft_frame_kernelILb0E", "audio_stream_fft_frame_kernelILb1E"):
        assert any(name in k for k in kernels), (name, sorted(fn))
    for k, (vgprs, scratch, inloop) in kernels.items():
        assert scratch == 0 and inloop == 0 and 0 < vgprs <= 128, (k, vgprs, scratch, inloop)


def _parameters(text, name):
    """the parameter list of the declaration of `name`, one normalised 'type name' string per parameter"""
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % re.escape(name), text)
    assert m, "%s is not declared" % name
    return [re.sub(r"\s*\*\s*", " *", " ".join(p.split())) for p in m.group(1).split(",")]


def test_the_fft_push_has_the_direct_push_parameters_and_is_exported(repo_root):
    from audio_sheet_retrieval_amd import _lib, build
    text = open(os.path.join(repo_root, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    direct = _parameters(text, "asr_audio_stream_push_dev")
    fft = _parameters(text, "asr_audio_stream_push_fft_dev")
    assert len(direct) == 33 and direct[0] == "asr_ctx *ctx" and direct[-1] == "int64_t out_floats"
    assert fft == direct
    assert "asr_audio_stream_push_fft_dev" in _lib.EXPORTS
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    assert hasattr(lib, "asr_audio_stream_push_fft_dev"), "libasr_hip.so does not export asr_audio_stream_push_fft_dev"
    bound = _lib.load_library()                                     # the prototypes resolve, and agree in length
    assert bound.asr_audio_stream_push_fft_dev.argtypes == bound.asr_audio_stream_push_dev.argtypes
    assert len(bound.asr_audio_stream_push_fft_dev.argtypes) == len(fft)
