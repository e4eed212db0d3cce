"""CPU: audio_frontend.spectrogram_fft_host, the numpy float32 restatement of the plan of asr_spectrogram_fft_batch_dev
(csrc/spectrogram_fft_kernels.hip), against a float64 spectrogram (tests/spectrogram_fft_ref.py), and the Python surface
of the FFT route that needs no device.

The bound on the four signals has two parts: 1e-4, the project's figure for this output
(tests/test_audio_frontend.py::test_device_spectrogram_matches_oracle), and the deviation of a float32 serial-order
direct DFT on the same signal - an FFT that is less accurate than the loop it replaces would be wrong."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrogram_fft_ref as R  # noqa: E402


def _proc(**kw):
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    return SpectrogramProcessor(None, **kw)


@pytest.mark.parametrize("i", range(4), ids=[s[0] for s in R.signals()])
def test_host_restatement_against_the_float64_spectrogram(i):
    from audio_sheet_retrieval_amd.audio_frontend import spectrogram_fft_host
    proc = _proc()
    name, x, scale = R.signals()[i]
    got = spectrogram_fft_host(x, R.window_for(proc, scale), proc.fb_start, proc.fb_len, proc.fb_w, proc.hop)
    ref = R.reference(i)
    assert got.dtype == np.float32 and got.shape == ref.shape == (92, proc.num_frames(x.size))
    dev = float(np.abs(got.astype(np.float64) - ref).max())
    direct = R.serial_dft_deviation(i)
    print("%s: fft %.3g, serial-order DFT %.3g" % (name, dev, direct))
    assert dev <= 1e-4, (name, dev)
    assert dev <= direct, (name, dev, direct)


@pytest.mark.parametrize("p", R.IMPULSE_AT)
def test_host_restatement_of_an_impulse(p):
    from audio_sheet_retrieval_amd.audio_frontend import spectrogram_fft_host
    proc = _proc()
    got = spectrogram_fft_host(R.impulse_recording(p), proc.window, proc.fb_start, proc.fb_len, proc.fb_w, proc.hop)
    want = R.impulse_expected(p, proc)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= R.IMPULSE_TOL, float(np.abs(got - want).max())


def test_host_restatement_of_short_and_empty_recordings():
    from audio_sheet_retrieval_amd.audio_frontend import spectrogram_fft_host
    proc = _proc()
    args = (proc.window, proc.fb_start, proc.fb_len, proc.fb_w, proc.hop)
    assert spectrogram_fft_host(np.zeros(0, np.float32), *args).shape == (92, 0)
    one = spectrogram_fft_host(np.ones(1, np.float32), *args)
    assert one.shape == (92, 1) and np.array_equal(one, np.zeros((92, 1), np.float32))      # window[0] == 0


def test_the_call_is_exported():
    from audio_sheet_retrieval_amd import _lib
    assert "asr_spectrogram_fft_batch_dev" in _lib.EXPORTS
    assert callable(_lib.Engine.spectrogram_fft_batch_dev)


def test_the_dft_keyword_is_checked_at_construction():
    assert _proc().dft == "direct" and _proc(dft="fft").dft == "fft"
    with pytest.raises(ValueError):
        _proc(dft="bogus")
    with pytest.raises(ValueError):
        _proc(frame_size=1024, dft="fft")
    assert _proc(frame_size=1024).frame_size == 1024              # the direct route keeps its frame sizes
    with pytest.raises(ValueError):
        _proc(dft="fft").stream()


def test_fast_dft_and_live_are_an_argument_error(capsys):
    from audio_sheet_retrieval_amd import umc_a2s_server
    with pytest.raises(SystemExit) as e:
        umc_a2s_server._arguments(["--model", "models/m.py", "--fast_dft", "--live"], "A2S")
    assert e.value.code == 2 and "--fast_dft" in capsys.readouterr().err
    assert umc_a2s_server._arguments(["--model", "models/m.py", "--fast_dft"], "S2A").fast_dft is True
    assert umc_a2s_server._arguments(["--model", "models/m.py"], "A2S").fast_dft is False
