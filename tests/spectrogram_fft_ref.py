"""What tests/test_spectrogram_fft_host.py and tests/test_gpu_spectrogram_fft.py share: the four test signals, the float64
yardstick of the FFT route (built here, not taken from oracle/ - oracle.audio_frontend.spectrogram hands a float32 array
to np.fft.fft, which numpy >= 2 computes in complex64), a float32 serial-order restatement of the direct DFT, and the
impulse cases.  Every result is computed once per process and handed out read-only."""
import functools

import numpy as np

SR, FRAME, HOP = 22050, 2048, 22050 / 20.0
INT16_SCALE = 1.0 / 32767


def three_component_signal():
    """the signal of tests/test_audio_frontend.py::test_device_spectrogram_matches_oracle (2.3 s)"""
    rng = np.random.default_rng(0)
    t = np.arange(int(SR * 2.3)) / float(SR)
    return (0.3 * np.sin(2 * np.pi * 261.6 * t) + 0.2 * np.sin(2 * np.pi * 1318.5 * t) * (t > 1.0)
            + 0.05 * rng.standard_normal(t.size)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def signals():
    """((name, float32 samples, window_scale), ...)"""
    x = three_component_signal()
    pcm = np.rint(np.clip(3.0 * x.astype(np.float64), -1.0, 1.0) * 32767).astype(np.float32)     # int16 values
    rng = np.random.default_rng(1)
    step = rng.standard_normal(SR).astype(np.float32)
    step[9000:] *= np.float32(1e-3)
    loud = (rng.standard_normal(8000) * 1000.0).astype(np.float32)
    out = (("three_components", x, 1.0), ("clipped_int16", pcm, INT16_SCALE), ("noise_with_quiet_tail", step, 1.0),
           ("loud_noise", loud, 1.0))
    for _, s, _ in out:
        s.setflags(write=False)
    return out


def frames_of(samples, dtype):
    """(n_frames, 2048): frame i starts at int(i * hop); samples past the end of the recording read as zero"""
    x = np.asarray(samples).ravel()
    n = int(np.ceil(x.size / HOP))
    out = np.zeros((n, FRAME), dtype)
    for i in range(n):
        seg = x[int(i * HOP):int(i * HOP) + FRAME]
        out[i, :seg.size] = seg
    return out


def _filterbank(mag, proc, dtype):
    """(n_frames, 1024) magnitudes -> (n_filters, n_frames), weights in ascending bin order"""
    out = np.zeros((proc.num_bins, mag.shape[0]), dtype)
    off = 0
    for f in range(proc.num_bins):
        acc = np.zeros(mag.shape[0], dtype)
        for q in range(int(proc.fb_len[f])):
            acc = acc + mag[:, int(proc.fb_start[f]) + q] * dtype(proc.fb_w[off + q])
        off += int(proc.fb_len[f])
        out[f] = acc
    return out


def yardstick(samples, proc, window):
    """the float64 spectrogram: float64(sample) * float64(window_f32[t]), np.fft.rfft in float64, |.| of bins 0 .. 1023,
    the filterbank in float64 with the float32 weights, log10(1 + s) in float64 -> (n_filters, n_frames) float64"""
    fr = frames_of(samples, np.float64) * np.asarray(window, np.float32).astype(np.float64)[None, :]
    mag = np.abs(np.fft.rfft(fr, axis=1))[:, :FRAME // 2]
    assert mag.dtype == np.float64
    return np.log10(1.0 * _filterbank(mag, proc, np.float64) + 1.0)


def serial_dft_host(samples, proc, window):
    """float32 restatement of the direct DFT of csrc/spectrogram_frame.h: per bin one running sum over the 2048 samples
    in ascending order, float32 twiddles rounded from float64, one rounding per product and per sum (the kernel fuses
    them, which is a little better) -> (n_filters, n_frames) float32"""
    fr = frames_of(samples, np.float32) * np.asarray(window, np.float32)[None, :]
    max_bin = int((proc.fb_start + proc.fb_len).max())
    t = np.arange(FRAME, dtype=np.float64)
    tc, ts = np.cos(2 * np.pi * t / FRAME).astype(np.float32), np.sin(2 * np.pi * t / FRAME).astype(np.float32)
    k = np.arange(max_bin)
    re, im = np.zeros((fr.shape[0], max_bin), np.float32), np.zeros((fr.shape[0], max_bin), np.float32)
    for n in range(FRAME):
        idx = (k * n) & (FRAME - 1)
        re = re + fr[:, n, None] * tc[None, idx]
        im = im + (-fr[:, n, None]) * ts[None, idx]
    mag = np.zeros((fr.shape[0], FRAME // 2), np.float32)
    mag[:, :max_bin] = np.sqrt(re * re + im * im)
    s = _filterbank(mag, proc, np.float32)
    return np.log10(np.float32(1.0) * s + np.float32(1.0))


def window_for(proc, scale):
    return proc.window if scale == proc.window_scale else proc._window(scale)


@functools.lru_cache(maxsize=None)
def _references(i):
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    proc = SpectrogramProcessor(None)
    _, x, scale = signals()[i]
    w = window_for(proc, scale)
    ref = yardstick(x, proc, w)
    direct_dev = float(np.abs(serial_dft_host(x, proc, w).astype(np.float64) - ref).max())
    ref.setflags(write=False)
    return ref, direct_dev


def reference(i):
    """the yardstick of signal i, read-only"""
    return _references(i)[0]


def serial_dft_deviation(i):
    """largest deviation of the float32 serial-order DFT restatement from the yardstick on signal i"""
    return _references(i)[1]


# ---- impulses: a single 1.0 at sample p gives |X[k]| = window[p - start] for every bin of every frame that holds it, and
# the filters sum to 1, so all bands of that frame are log10(1 + window[p - start]); every other frame is log10(1) = 0.
# The recording has 5000 samples: 5 frames starting at 0, 1102, 2205, 3307, 4410, the last two zero padded.  p lies a
# quarter and three quarters into the frames 1 (even start), 2 and 3 (odd starts; 3 is zero padded), where the window's
# slope is 1.5e-3 per sample: a start that is off by one moves the result by 4e-4.
IMPULSE_LEN = 5000
IMPULSE_AT = tuple(int(i * HOP) + q for i in (1, 2, 3) for q in (FRAME // 4, 3 * FRAME // 4))
# float32: the impulse passes 5 butterflies and the post-pass with at most one rounded twiddle product each, the
# magnitude and the 92-band sums add a few more roundings - a relative error of some 1e-6 of a value <= 1 whose logarithm
# has slope <= 0.44; 1e-5 is ten times that and forty times below what an index error gives
IMPULSE_TOL = 1e-5


def impulse_recording(p):
    x = np.zeros(IMPULSE_LEN, np.float32)
    x[p] = 1.0
    return x


def impulse_expected(p, proc):
    n = int(np.ceil(IMPULSE_LEN / HOP))
    starts = [int(i * HOP) for i in range(n)]
    assert n == 5 and starts[1] % 2 == 0 and starts[2] % 2 == 1 and starts[-1] + FRAME > IMPULSE_LEN
    out = np.zeros((proc.num_bins, n), np.float64)
    hit = 0
    for i, s in enumerate(starts):
        if s <= p < s + FRAME:
            out[:, i] = np.log10(1.0 + float(proc.window[p - s]))
            hit += 1
    assert hit >= 2
    return out
