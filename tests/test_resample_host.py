"""CPU: the resampler's definition (include/asr_hip.h, asr_resample_batch_dev) as audio_frontend states it on the host -
resample_plan's taps against scipy's firwin, resample_host against scipy's resample_poly (an independent implementation
of the same polyphase sum), the filter's own frequency response, tones through it, the 16-bit mode, and read_audio on
.wav files of several rates.  The device is compared with resample_host bit for bit in tests/test_gpu_resample.py."""
import math

import numpy as np
import pytest
from scipy import signal
from scipy.io import wavfile

from audio_sheet_retrieval_amd.audio_frontend import (SAMPLE_RATE, load_audio, read_audio, resample_host,
                                                      resample_plan)

#: rate -> (up, down, taps per phase)
RATES = {44100: (1, 2, 65), 48000: (147, 320, 70), 96000: (147, 640, 140), 32000: (441, 640, 47),
         16000: (441, 320, 33), 11025: (2, 1, 33), 8000: (441, 160, 33)}


def _firwin(rate):
    g = math.gcd(rate, SAMPLE_RATE)
    up, down = SAMPLE_RATE // g, rate // g
    q = max(up, down)
    return signal.firwin(2 * 16 * q + 1, 1.0 / q, window=("kaiser", 8.6)) * up, up, down, q


def _response(rate):
    """(largest passband deviation of |H| / up from 1, largest stopband gain) of the firwin taps: passband up to 0.8 of
    the lower Nyquist frequency, stopband from 1.2 of it; frequencies in units of the filter's own Nyquist frequency"""
    h, up, _, q = _firwin(rate)
    n_fft = 1 << int(np.ceil(np.log2(h.size * 16)))
    H = np.abs(np.fft.rfft(h, n_fft)) / up
    f = np.arange(H.size) / float(H.size - 1)
    return float(np.abs(H[f <= 0.8 / q] - 1.0).max()), float(H[f >= 1.2 / q].max())


@pytest.mark.parametrize("rate", sorted(RATES))
def test_taps_are_the_kaiser_windowed_sinc(rate):
    up, down, half, hp = resample_plan(rate)
    h, f_up, f_down, q = _firwin(rate)
    assert (up, down, hp.shape[1]) == RATES[rate] and (up, down) == (f_up, f_down)
    assert half == 16 * q and hp.shape == (up, -(-(2 * half + 1) // up)) and hp.dtype == np.float64
    flat = hp.T.ravel()                                   # hp[p][t] = h[p + t * up]
    diff = float(np.abs(flat[:h.size] - h).max())
    print("rate %d: taps differ from firwin * up by at most %.3g" % (rate, diff))
    assert diff <= 1e-12
    assert not flat[h.size:].any()
    assert abs(flat.sum() - up) <= 1e-9 * up


@pytest.mark.parametrize("rate", sorted(RATES))
def test_resample_host_is_scipys_polyphase_sum(rate):
    up, down, half, hp = resample_plan(rate)
    T = hp.shape[1]
    h = hp.T.ravel()[:2 * half + 1]
    rng = np.random.default_rng(rate)
    worst = 0.0
    for n in (0, 1, 5, T + 3, 1000, 5003):
        x = rng.standard_normal(n).astype(np.float32)
        got = resample_host(x, rate)
        assert got.dtype == np.float32 and got.shape == (-(-n * up // down),)
        if n == 0:
            continue
        ref = signal.resample_poly(x.astype(np.float64), up, down, window=h / up)
        assert ref.shape == got.shape
        err = np.abs(got.astype(np.float64) - ref)
        worst = max(worst, float(err.max()))
        assert np.all(err <= 2.0 ** -23 * np.abs(ref) + 1e-12), (n, float(err.max()))
    print("rate %d: resample_host differs from resample_poly by at most %.3g" % (rate, worst))


@pytest.mark.parametrize("rate", sorted(RATES))
def test_frequency_response_of_the_design(rate):
    ripple, stop = _response(rate)
    print("rate %d: passband deviation %.3g, stopband %.1f dB" % (rate, ripple, 20 * np.log10(stop)))
    assert ripple <= 1e-4
    assert 20 * np.log10(stop) <= -80.0


def test_tones_at_44100():
    ripple, stop = _response(44100)
    t_in = np.arange(44100) / 44100.0
    t_out = np.arange(22050) / 22050.0
    y = resample_host(np.sin(2 * np.pi * 1000.0 * t_in).astype(np.float32), 44100)
    assert y.shape == (22050,)
    err = float(np.abs(y[200:-200] - np.sin(2 * np.pi * 1000.0 * t_out)[200:-200]).max())
    print("1 kHz: deviation %.3g (passband %.3g)" % (err, ripple))
    assert err <= ripple + 1e-6
    y = resample_host(np.sin(2 * np.pi * 15000.0 * t_in).astype(np.float32), 44100)
    amp = float(np.abs(y[200:-200]).max())
    print("15 kHz: amplitude %.3g (stopband %.3g)" % (amp, stop))
    assert amp < stop


def square_wave(rate=44100, seconds=1.0, freq=100.0):
    t = np.arange(int(rate * seconds)) / float(rate)
    return np.where(np.sin(2 * np.pi * freq * t) >= 0, 32767.0, -32767.0).astype(np.float32)


def test_integer_mode_rounds_and_clips():
    x = square_wave()
    y = resample_host(x, 44100, integer=True)
    assert y.dtype == np.float32 and y.shape == (22050,)
    assert np.array_equal(y, np.rint(y)) and y.min() >= -32768 and y.max() <= 32767
    assert y.max() == 32767 and y.min() == -32768          # the filter overshoots at the edges: both limits are reached
    free = resample_host(x, 44100)
    assert free.max() > 32767.5 and free.min() < -32768.5                  # ... and the clip is what stops them
    assert np.abs(y - np.clip(free, -32768, 32767)).max() <= 0.5 + 2.0 ** -9   # float32 spacing at 32768: 2^-8


def test_read_audio(tmp_path):
    rng = np.random.default_rng(3)
    stereo = rng.integers(-32768, 32768, size=(4410, 2)).astype(np.int16)
    mono32 = rng.standard_normal(4800).astype(np.float32)
    own = rng.integers(-32768, 32768, size=2205).astype(np.int16)
    a, b, c = (str(tmp_path / n) for n in ("a.wav", "b.wav", "c.wav"))
    wavfile.write(a, 44100, stereo)
    wavfile.write(b, 48000, mono32)
    wavfile.write(c, 22050, own)

    samples, scale, rate, integer = read_audio(a)
    assert (scale, rate, integer) == (1.0 / 32767, 44100, True) and samples.dtype == np.float32
    assert np.array_equal(samples, np.mean(stereo, axis=-1).astype(np.int16).astype(np.float32))
    samples, scale, rate, integer = read_audio(b)
    assert (scale, rate, integer) == (1.0, 48000, False) and np.array_equal(samples, mono32)
    samples, scale, rate, integer = read_audio(c)
    assert (scale, rate, integer) == (1.0 / 32767, 22050, True) and np.array_equal(samples, own.astype(np.float32))
    # load_audio is what it was
    l_samples, l_scale = load_audio(c)
    assert np.array_equal(l_samples, samples) and l_scale == scale
    with pytest.raises(ValueError, match="sample rate 44100 Hz"):
        load_audio(a)
    with pytest.raises(ValueError, match="sample rate 48000 Hz"):
        load_audio(b)
    # a .npy file has no rate of its own
    d = str(tmp_path / "d.npy")
    np.save(d, mono32)
    samples, scale, rate, integer = read_audio(d)
    assert (scale, rate, integer) == (1.0, SAMPLE_RATE, False) and np.array_equal(samples, mono32)


@pytest.mark.parametrize("rate", [3999, 192001])
def test_rates_outside_the_range_are_rejected(tmp_path, rate):
    path = str(tmp_path / "x.wav")
    wavfile.write(path, rate, np.zeros(100, np.int16))
    samples, _, got, _ = read_audio(path)
    assert got == rate and samples.size == 100
    with pytest.raises(ValueError, match="sample rate"):
        resample_plan(got)
    with pytest.raises(ValueError, match="sample rate"):
        resample_host(samples, got)
    with pytest.raises(ValueError):
        resample_plan(44100.0)
