"""Audio front-end on the GPU: waveform -> the (92, frames) log-frequency spectrogram the
spectrogram tower takes, i.e. the madmom processor chain of the reference (tutorials/Embedding Tutorial.ipynb cell 28;
`processor.process(audio_file).T` at audio_sheet_server.py:632,678, audio2sheet_align.py:99):

    SignalProcessor(num_channels=1, sample_rate=22050) -> FramedSignalProcessor(frame_size=2048, fps=20, origin='future')
    -> FilteredSpectrogramProcessor(LogarithmicFilterbank, num_bands=16, fmin=30, fmax=6000)
    -> LogarithmicSpectrogramProcessor()

`process(samples)` takes mono samples at SAMPLE_RATE; `load_audio(path)` reads them from a .wav or .npy file.  Decoding
compressed formats stays with the caller.  Recordings at another rate: `read_audio(path)` reads them at their own rate
and `process*(..., sample_rate(s)=...)` resamples them on the device between the upload and the spectrogram
(asr_resample_batch_dev, csrc/resample_kernels.hip).  madmom resamples through ffmpeg, whose filter cannot be restated;
the resampler here is a definition of its own (include/asr_hip.h; `resample_plan`, `resample_host`).  Without a sample
rate everything behaves as before: a foreign rate is an error.  The filterbank is built on the host with madmom's published construction (third-party
semantic, unverified offline; it reproduces the reference's 92 bands); framing, windowed DFT magnitudes,
filterbank and logarithm run in one kernel per call (csrc/piece_vote_kernels.hip: spectrogram_kernel).
`SpectrogramProcessor(engine, dft="fft")` takes the magnitudes from a real-input FFT instead of the direct DFT
(asr_spectrogram_fft_batch_dev, csrc/spectrogram_fft_kernels.hip; `spectrogram_fft_host` restates its plan): the same
spectrogram within float32 rounding and some 55 times faster, but not bit-identical with the default route.  Its
stream is `processor.stream(..., dft="fft")` (asr_audio_stream_push_fft_dev, csrc/audio_stream_fft_kernels.hip):
bit-identical with that processor's `process`, and only given when asked for by name.
"""
from __future__ import print_function

import os

import numpy as np

SAMPLE_RATE = 22050
FRAME_SIZE = 2048
FPS = 20


def _log_frequencies(bands_per_octave, fmin, fmax, fref=440.0):
    left = np.floor(np.log2(float(fmin) / fref) * bands_per_octave)
    right = np.ceil(np.log2(float(fmax) / fref) * bands_per_octave)
    freqs = fref * 2.0 ** (np.arange(left, right) / float(bands_per_octave))
    freqs = freqs[np.searchsorted(freqs, fmin):]
    return freqs[:np.searchsorted(freqs, fmax, 'right')]


def _frequencies2bins(frequencies, bin_frequencies):
    idx = bin_frequencies.searchsorted(frequencies)
    idx = np.clip(idx, 1, len(bin_frequencies) - 1)
    left, right = bin_frequencies[idx - 1], bin_frequencies[idx]
    idx -= frequencies - left < right - frequencies
    return np.unique(idx)                                  # unique_filters=True


def logarithmic_filterbank(sample_rate=SAMPLE_RATE, frame_size=FRAME_SIZE, num_bands=16, fmin=30.0, fmax=6000.0):
    """madmom.audio.filters.LogarithmicFilterbank(norm_filters=True, unique_filters=True) as
    (starts int32[nf], lengths int32[nf], weights float32[sum lengths])."""
    bin_freqs = np.fft.fftfreq(frame_size, 1.0 / sample_rate)[:frame_size >> 1]
    bins = _frequencies2bins(_log_frequencies(num_bands, fmin, fmax), bin_freqs)
    starts, lens, weights = [], [], []
    for start, center, stop in zip(bins[:-2], bins[1:-1], bins[2:]):
        if stop - start < 2:
            center, stop = start, start + 1
        c = int(center - start)
        data = np.zeros(int(stop - start), dtype=np.float32)
        data[:c] = np.linspace(0, 1, c, endpoint=False)
        data[c:] = np.linspace(1, 0, int(stop - center), endpoint=False)
        data /= data.sum()
        starts.append(int(start))
        lens.append(len(data))
        weights.append(data)
    return np.asarray(starts, np.int32), np.asarray(lens, np.int32), np.concatenate(weights).astype(np.float32)


LOADABLE = (".wav", ".npy")


def _read(path, sample_rate, any_rate):
    """load_audio / read_audio -> (samples, window_scale, rate, integer)"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        samples = np.load(path)
        if samples.ndim != 1 or samples.dtype.kind != "f":
            raise ValueError("%s: expected mono float samples (1-d), got %s %r" % (path, samples.dtype, samples.shape))
        return np.ascontiguousarray(samples, dtype=np.float32), 1.0, sample_rate, False
    if ext != ".wav":
        raise ValueError("%s: no decoder for '%s' files is part of this implementation; convert the recording to "
                         "a %d Hz .wav (PCM 16-bit or float32) or .npy (mono float samples) file" %
                         (path, ext or "extension-less", sample_rate))
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if rate != sample_rate and not any_rate:
        raise ValueError("%s: sample rate %d Hz, expected %d Hz (resample the file first)" % (path, rate, sample_rate))
    if data.dtype == np.int16:
        scale = 1.0 / 32767
    elif data.dtype == np.float32:
        scale = 1.0
    else:
        raise ValueError("%s: %s samples; PCM 16-bit and float32 .wav files are read" % (path, data.dtype))
    if data.ndim == 2:
        # madmom's remix: the channel mean, in the sample type (integers truncate as astype does)
        data = np.mean(data, axis=-1).astype(data.dtype)
    return np.ascontiguousarray(data, dtype=np.float32), scale, int(rate), bool(data.dtype == np.int16)


def load_audio(path, sample_rate=SAMPLE_RATE):
    """-> (mono float32 samples, window_scale) of a .wav (PCM 16-bit or float32) or .npy (mono float samples) file -
    what madmom's SignalProcessor(num_channels=1, sample_rate=22050) hands on.  Channels are averaged.  16-bit PCM
    keeps its integer values and comes with window_scale = 1 / 32767 (madmom scales the STFT window by the integer
    range instead of the samples); float input has window_scale 1.  A file at another rate is an error: read_audio
    reads it, and the processor resamples it when it is told the rate."""
    return _read(path, sample_rate, False)[:2]


def read_audio(path):
    """load_audio for a file of any sample rate -> (mono float32 samples, window_scale, rate, integer).  integer: the
    samples are 16-bit PCM values, and resampling them yields 16-bit values again (rounded and clipped), as a decoder
    hands them to madmom.  A .npy file carries no rate: its samples are taken to be at SAMPLE_RATE."""
    return _read(path, SAMPLE_RATE, True)


RESAMPLE_TILE = 1024          # outputs per workgroup of resample_batch_kernel (csrc/asr_kernels.h)
RESAMPLE_RATES = (4000, 192000)
_plans = {}


def resample_plan(rate_in, rate_out=SAMPLE_RATE):
    """-> (up, down, half, taps_phase_major float64 (up, T)): the resampler rate_in -> rate_out as include/asr_hip.h
    defines it (asr_resample_batch_dev).  up / down = rate_out / rate_in in lowest terms; the filter is a windowed sinc
    of 2 * half + 1 taps, half = 16 * max(up, down), Kaiser window with beta 8.6, cut-off at the lower of the two
    Nyquist frequencies, gain up; row p of the table holds taps p, p + up, p + 2 up, ... (zeros past the end).  Rates
    are integers from 4000 to 192000 Hz."""
    for r in (rate_in, rate_out):
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not RESAMPLE_RATES[0] <= r <= RESAMPLE_RATES[1]:
            raise ValueError("sample rate %r: integer rates from %d to %d Hz are resampled" % ((r,) + RESAMPLE_RATES))
    key = (int(rate_in), int(rate_out))
    if key not in _plans:
        import math
        g = math.gcd(*key)
        up, down = key[1] // g, key[0] // g
        q = max(up, down)
        half = 16 * q
        n_taps = 2 * half + 1
        h = np.sinc((np.arange(n_taps) - half) / float(q)) * np.kaiser(n_taps, 8.6)
        h *= up / h.sum()
        T = -(-n_taps // up)
        table = np.zeros(T * up, np.float64)
        table[:n_taps] = h
        table = np.ascontiguousarray(table.reshape(T, up).T)
        table.setflags(write=False)
        if len(_plans) >= 8:                  # a table is up to 49 MB
            _plans.clear()
        _plans[key] = (up, down, half, table)
    return _plans[key]


def resample_host(samples, rate_in, integer=False, rate_out=SAMPLE_RATE):
    """the numpy restatement of asr_resample_batch_dev (include/asr_hip.h): mono samples at rate_in -> float32 samples
    at rate_out; integer=True rounds to even and clips to the 16-bit range.  The sum of an output runs over the taps in
    ascending order, float64 product then float64 sum, as on the device (bit-identical for finite samples)."""
    up, down, half, hp = resample_plan(rate_in, rate_out)
    T = hp.shape[1]
    x = np.ascontiguousarray(samples, dtype=np.float32).ravel().astype(np.float64)
    n = x.size
    n_out = -(-n * up // down)
    y = np.zeros(n_out, np.float64)
    block = 1 << 18
    for m0 in range(0, n_out, block):
        m = np.arange(m0, min(m0 + block, n_out), dtype=np.int64)
        c = m * down + half
        p, j0 = c % up, c // up
        acc = y[m0:m0 + m.size]
        if j0[0] - (T - 1) >= 0 and j0[-1] < n:       # every tap of every output of the block meets a sample
            for t in range(T):
                acc += (hp[0, t] if up == 1 else hp[p, t]) * x[j0 - t]
        else:
            for t in range(T):
                j = j0 - t
                ok = (j >= 0) & (j < n)
                acc[ok] = acc[ok] + hp[p[ok], t] * x[j[ok]]
    if integer:
        y = np.clip(np.rint(y), -32768, 32767)
    return y.astype(np.float32)


_FFT_TWIDDLES = []


def _fft_twiddles():
    """exp(-2 pi i t / 2048), t = 0 .. 2047, complex64 rounded from float64: the one table of the FFT route"""
    if not _FFT_TWIDDLES:
        _FFT_TWIDDLES.append(np.exp(-2j * np.pi * np.arange(2048) / 2048.0).astype(np.complex64))
    return _FFT_TWIDDLES[0]


def spectrogram_fft_host(samples, window, fb_start, fb_len, fb_w, hop, mul=1.0, add=1.0):
    """The numpy float32 restatement of the plan of asr_spectrogram_fft_batch_dev (csrc/spectrogram_fft_kernels.hip) for
    one recording -> (n_filters, n_frames) float32, n_frames = ceil(n / hop): the same packing of a frame's 2048 windowed
    samples into 1024 complex values, the same five radix-4 Stockham passes with the same twiddle table, the same
    post-pass, filterbank and logarithm.  It is where the index arithmetic of the kernel can be read and checked on a
    CPU; the device contracts multiply-adds and has its own log10f, so the two agree to rounding, not bit for bit."""
    x = np.ascontiguousarray(samples, dtype=np.float32).ravel()
    window = np.ascontiguousarray(window, dtype=np.float32)
    if window.size != 2048:
        raise ValueError("spectrogram_fft_host: a window of %d samples; the FFT route has frames of 2048" % window.size)
    fb_w = np.ascontiguousarray(fb_w, dtype=np.float32)
    n_frames = int(np.ceil(x.size / float(hop)))
    nf = len(fb_start)
    out = np.zeros((nf, n_frames), np.float32)
    if not n_frames:
        return out
    tw = _fft_twiddles()
    starts = (np.arange(n_frames, dtype=np.float64) * float(hop)).astype(np.int64)      # int(i * hop), origin 'future'
    idx = starts[:, None] + np.arange(2048, dtype=np.int64)[None, :]
    padded = np.concatenate([x, np.zeros(2048, np.float32)])          # past the end of the recording: zeros
    frames = padded[idx] * window[None, :]
    z = np.empty((n_frames, 1024), np.complex64)                    # packing: z[n] = x[2n] + i x[2n + 1]
    z.real, z.imag = frames[:, 0::2], frames[:, 1::2]
    mul_i = lambda a: (-a.imag + 1j * a.real).astype(np.complex64)  # i * a, exactly
    n, s = 1024, 1
    while n > 1:                                                    # pass of stride s, sub-length n: lane t = q + s p
        n1 = n // 4
        v = z.reshape(n_frames, 4, n1, s)                           # v[k] = in[t + 256 k]
        apc, amc, bpd, ibmd = v[:, 0] + v[:, 2], v[:, 0] - v[:, 2], v[:, 1] + v[:, 3], mul_i(v[:, 1] - v[:, 3])
        p = np.arange(n1) * (2 * s)                                 # w^(p k) = tw[2 s p k]
        y = np.empty((n_frames, n1, 4, s), np.complex64)            # out[q + s (4 p + k)]
        y[:, :, 0] = apc + bpd
        y[:, :, 1] = amc - ibmd
        y[:, :, 2] = apc - bpd
        y[:, :, 3] = amc + ibmd
        if n1 > 1:
            for k in (1, 2, 3):
                y[:, :, k] *= tw[k * p][None, :, None]
        z = y.reshape(n_frames, 1024)
        n, s = n1, 4 * s
    zc = np.conj(z[:, (1024 - np.arange(1024)) % 1024])             # post-pass: conj Z[1024 - k], Z[1024] = Z[0]
    t = (z - zc) * tw[None, :1024]
    x2 = (z + zc) - mul_i(t)                                        # twice X[k]
    mag = (np.float32(0.5) * np.sqrt(x2.real * x2.real + x2.imag * x2.imag)).astype(np.float32)
    mul, add = np.float32(mul), np.float32(add)
    off = 0
    for f in range(nf):
        acc = np.zeros(n_frames, np.float32)
        for q in range(int(fb_len[f])):
            acc = acc + mag[:, int(fb_start[f]) + q] * fb_w[off + q]
        off += int(fb_len[f])
        out[f] = np.log10(mul * acc + add)
    return out


class SpectrogramProcessor(object):
    """processor = SequentialProcessor([sig_proc, fsig_proc, spec_proc, log_spec_proc]) of the reference, on the GPU."""

    def __init__(self, engine, sample_rate=SAMPLE_RATE, frame_size=FRAME_SIZE, fps=FPS, window_scale=1.0, dft="direct"):
        """dft: "direct" - the direct DFT of csrc/spectrogram_frame.h, the route every bit-parity statement of this
        class is about (process, process_many, the stream); "fft" - the magnitudes from a real-input FFT
        (asr_spectrogram_fft_batch_dev; frames of 2048 samples only): within float32 rounding of the same spectrogram and
        closer to the float64 one, several times faster, but not bit-identical with "direct"; its stream is
        stream(dft="fft"), a plain stream() is refused."""
        if dft not in ("direct", "fft"):
            raise ValueError('dft=%r: "direct" or "fft"' % (dft,))
        if dft == "fft" and frame_size != 2048:
            raise ValueError('dft="fft" computes frames of 2048 samples, not %r' % (frame_size,))
        self.dft = dft
        self.engine = engine
        self.sample_rate, self.frame_size, self.fps = sample_rate, frame_size, fps
        self.hop = sample_rate / float(fps)
        # int16 input: madmom divides the window by the integer range (stft.py); pass window_scale = 1 / 32767
        self.window_scale = window_scale
        self.window = self._window(window_scale)
        self.fb_start, self.fb_len, self.fb_w = logarithmic_filterbank(sample_rate, frame_size)
        self.num_bins = len(self.fb_start)

    def _window(self, window_scale):
        return (np.hanning(self.frame_size) * window_scale).astype(np.float32)

    def num_frames(self, n_samples):
        return int(np.ceil(n_samples / float(self.hop)))

    def _batch_call(self):
        """the engine's batched spectrogram call of this processor's dft"""
        return self.engine.spectrogram_fft_batch_dev if self.dft == "fft" else self.engine.spectrogram_batch_dev

    def process_dev(self, samples, sample_rate=None, integer=False):
        """-> (DeviceBuffer holding the (num_bins, n_frames) float32 spectrogram, n_frames).  sample_rate: the rate of
        `samples` where it is not the processor's - they are resampled on the device first (integer: 16-bit PCM
        values, see read_audio)"""
        if sample_rate is not None and sample_rate != self.sample_rate:
            dev = self.process_many_dev([samples], None, [sample_rate], [integer])
            return dev.buf, dev.shapes[0][1]
        if self.dft == "fft":                                     # the FFT route has the batched call only
            dev = self.process_many_dev([samples])
            return dev.buf, dev.shapes[0][1]
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        n = self.num_frames(samples.size)
        eng = self.engine
        d_in = eng.alloc(max(4, samples.nbytes)).upload(samples)
        d_out = eng.alloc(max(4, n * self.num_bins * 4))
        try:
            eng.spectrogram_dev(d_in.ptr, samples.size, self.frame_size, self.hop, self.window, self.fb_start,
                                self.fb_len, self.fb_w, n, d_out.ptr, transposed=True)
        finally:
            d_in.free()
        return d_out, n

    def process(self, samples, sample_rate=None, integer=False):
        """the reference's `processor.process(audio).T`: (num_bins, n_frames) float32"""
        d_out, n = self.process_dev(samples, sample_rate, integer)
        out = d_out.download((self.num_bins, n), np.float32)
        d_out.free()
        return out

    def process_many_dev(self, recordings, window_scales=None, sample_rates=None, integer=None):
        """process_dev for a list of recordings of any lengths (an empty one gives no frames) in one launch
        (asr_spectrogram_batch_dev) -> piece_identification.DeviceArrays: the (num_bins, n_frames_i) spectrograms back
        to back in one device buffer, each bit-identical with process()'s.  window_scales: one per recording (what
        load_audio returned; default: the processor's) - recordings of equal scale share a launch.
        sample_rates: one per recording (what read_audio returned).  Recordings at the processor's rate are uploaded
        to their place in the buffer the spectrogram launch reads; the others are uploaded at their own rate and
        resampled into place on the device, one asr_resample_batch_dev call per (rate, integer) group - each result
        bit-identical with process() on resample_host()'s.  integer: one flag per recording (read_audio's; default
        False)."""
        from .piece_identification import DeviceArrays
        recs = [np.ascontiguousarray(r, dtype=np.float32).ravel() for r in recordings]
        scales = [self.window_scale] * len(recs) if window_scales is None else [float(w) for w in window_scales]
        if len(scales) != len(recs):
            raise ValueError("%d window scales for %d recordings" % (len(scales), len(recs)))
        if sample_rates is not None:
            return self._process_many_rates_dev(recs, scales, sample_rates, integer)
        if integer is not None:
            raise ValueError("integer flags without sample rates")
        counts = np.asarray([r.size for r in recs], np.int64)
        frames = np.asarray([self.num_frames(r.size) for r in recs], np.int64)
        s_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if recs else np.zeros(0, np.int64)
        o_off = np.concatenate([[0], np.cumsum(frames * self.num_bins)[:-1]]).astype(np.int64) if recs else \
            np.zeros(0, np.int64)
        eng = self.engine
        flat = np.concatenate(recs) if recs else np.zeros(0, np.float32)
        out_floats = int(frames.sum()) * self.num_bins
        d_in = eng.alloc(max(4, flat.nbytes)).upload(flat)
        d_out = eng.alloc(max(4, out_floats * 4))
        try:
            for scale in sorted(set(scales)):
                sel = np.asarray([i for i, w in enumerate(scales) if w == scale], np.int64)
                window = self.window if scale == self.window_scale else self._window(scale)
                self._batch_call()(d_in.ptr, flat.size, s_off[sel], counts[sel], frames[sel], o_off[sel],
                                   self.frame_size, self.hop, window, self.fb_start, self.fb_len, self.fb_w,
                                   d_out.ptr, out_floats, transposed=True)
        except Exception:
            d_out.free()
            raise
        finally:
            d_in.free()
        return DeviceArrays(d_out, [int(o) for o in o_off], [(self.num_bins, int(n)) for n in frames])

    def _process_many_rates_dev(self, recs, scales, sample_rates, integer):
        """process_many_dev with sample rates: upload, resample into place, one spectrogram launch per window scale"""
        from .piece_identification import DeviceArrays
        rates = list(sample_rates)
        flags = [False] * len(recs) if integer is None else [bool(f) for f in integer]
        if len(rates) != len(recs) or len(flags) != len(recs):
            raise ValueError("%d sample rates and %d integer flags for %d recordings" % (len(rates), len(flags), len(recs)))
        foreign = [i for i, r in enumerate(rates) if r != self.sample_rate]
        plans = {r: resample_plan(r, self.sample_rate) for r in set(rates[i] for i in foreign)}
        counts = np.asarray([r.size for r in recs], np.int64)          # at the processor's rate
        for i in foreign:
            up, down = plans[rates[i]][:2]
            counts[i] = -(-recs[i].size * up // down)
        frames = np.asarray([self.num_frames(int(c)) for c in counts], np.int64)
        zero = np.zeros(0, np.int64)
        s_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if recs else zero
        o_off = np.concatenate([[0], np.cumsum(frames * self.num_bins)[:-1]]).astype(np.int64) if recs else zero
        n_off = np.zeros(len(recs), np.int64)                          # of the foreign ones in the native-rate buffer
        native_floats = 0
        for i in foreign:
            n_off[i] = native_floats
            native_floats += recs[i].size
        eng = self.engine
        in_floats = int(counts.sum())
        out_floats = int(frames.sum()) * self.num_bins
        d_in = eng.alloc(max(4, in_floats * 4))
        d_native = eng.alloc(max(4, native_floats * 4)) if foreign else None
        d_out = eng.alloc(max(4, out_floats * 4))
        try:
            own = [i for i in range(len(recs)) if rates[i] == self.sample_rate and recs[i].size]
            k = 0
            while k < len(own):                                       # neighbours in the buffer travel together
                e = k + 1
                while e < len(own) and own[e] == own[e - 1] + 1:
                    e += 1
                eng.raw_upload(d_in.offset(4 * int(s_off[own[k]])), np.concatenate([recs[i] for i in own[k:e]]))
                k = e
            if native_floats:
                d_native.upload(np.concatenate([recs[i] for i in foreign]))
            for rate, flag in sorted(set((rates[i], flags[i]) for i in foreign)):
                sel = np.asarray([i for i in foreign if rates[i] == rate and flags[i] == flag], np.int64)
                up, down, half, taps = plans[rate]
                eng.resample_batch_dev(d_native.ptr, native_floats, n_off[sel], [recs[i].size for i in sel], s_off[sel],
                                       counts[sel], up, down, taps, half, flag, d_in.ptr, in_floats)
            for scale in sorted(set(scales)):
                sel = np.asarray([i for i, w in enumerate(scales) if w == scale], np.int64)
                window = self.window if scale == self.window_scale else self._window(scale)
                self._batch_call()(d_in.ptr, in_floats, s_off[sel], counts[sel], frames[sel], o_off[sel],
                                   self.frame_size, self.hop, window, self.fb_start, self.fb_len, self.fb_w,
                                   d_out.ptr, out_floats, transposed=True)
        except Exception:
            d_out.free()
            raise
        finally:
            d_in.free()
            if d_native is not None:
                d_native.free()
        return DeviceArrays(d_out, [int(o) for o in o_off], [(self.num_bins, int(n)) for n in frames])

    def process_many(self, recordings, window_scales=None, sample_rates=None, integer=None):
        """process() for a list of recordings in one launch -> list of (num_bins, n_frames_i) float32 arrays"""
        dev = self.process_many_dev(recordings, window_scales, sample_rates, integer)
        try:
            total = sum(r * c for r, c in dev.shapes)
            flat = dev.buf.download((total,), np.float32) if total else np.zeros(0, np.float32)
        finally:
            dev.buf.free()
        return [flat[o:o + r * c].reshape(r, c).copy() for o, (r, c) in zip(dev.offsets, dev.shapes)]

    def stream(self, n_streams=1, sample_rate=None, integer=False, window_scale=None, dft=None):
        """AudioStream(self, ...): spectrogram columns from audio that arrives block by block.  dft: None - the direct
        stream of a "direct" processor; "fft" - the FFT stream of an "fft" processor, named explicitly (AudioStream)"""
        return AudioStream(self, n_streams, sample_rate, integer, window_scale, dft)


# ---- streamed audio: blocks of samples in, the spectrogram columns they complete out ----------------------------------------
# The integer plan of asr_audio_stream_push_dev (include/asr_hip.h carries the definition).  The resampler's output m reads
# the inputs j0(m) - (T - 1) .. j0(m), j0(m) = (m * down + half) // up, T = taps_per_phase; taps_per_phase == 0 stands for
# the front-end's own rate (up == down == 1, y = x, no filter).
def _stream_final_outputs(n, up, down, half, taps_per_phase):
    """M(n): how many resampler outputs n input samples make final, j0(m) < n"""
    if not taps_per_phase:
        return n
    num = n * up - half
    return 0 if num <= 0 else min(-(-num // down), -(-n * up // down))


def _stream_complete_frames(m, frame_size, hop):
    """number of frames i with int(i * hop) + frame_size <= m: an estimate, then the definition"""
    if m < frame_size:
        return 0
    k = int(float(m - frame_size) / hop)
    while int(float(k) * hop) + frame_size <= m:
        k += 1
    while k > 0 and int(float(k - 1) * hop) + frame_size > m:
        k -= 1
    return k


def _stream_keep_from(next_frame, n, hop, up, down, half, taps_per_phase):
    s = int(float(next_frame) * hop)
    j = (s * down + half) // up - (taps_per_phase - 1) if taps_per_phase else s
    return max(0, min(j, n))


def audio_stream_plan(n_before, n_new, final, frame_size, hop, up=1, down=1, half=0, taps_per_phase=0):
    """-> (first_frame, n_frames, keep_from) of one push of n_new input samples to a stream that has had n_before: the
    first frame the push emits, how many it emits, and the first input sample the state holds afterwards - what
    asr_audio_stream_push_dev recomputes and checks.  final: the push flushes the stream (the frames past the last sample,
    zero padded, up to num_frames of the whole recording).  hop is a float64 and a frame starts at int(i * hop), as on the
    device; everything else is integer arithmetic."""
    n_before, n_new, hop = int(n_before), int(n_new), float(hop)
    n1 = n_before + n_new
    args = (up, down, half, taps_per_phase)
    f0 = _stream_complete_frames(_stream_final_outputs(n_before, *args), frame_size, hop)
    if final:
        length = -(-n1 * up // down) if taps_per_phase else n1
        f1 = max(f0, int(np.ceil(length / hop)))
    else:
        f1 = _stream_complete_frames(_stream_final_outputs(n1, *args), frame_size, hop)
    return f0, f1 - f0, _stream_keep_from(f1, n1, hop, *args)


def audio_stream_state_len(frame_size, up=1, down=1, taps_per_phase=0):
    """floats of state a stream needs: n - keep_from never exceeds it, whatever the cut into blocks.
    Proof.  After n samples let i be the first frame not emitted and s = int(i * hop) its start.  Not emitted means
    s + frame_size > M(n), so output s + frame_size - 1 is not final: j0(s + frame_size - 1) >= n.  The state starts at
    keep_from = max(0, j0(s) - (T - 1)) (the clamp to n only empties it), hence
        n - keep_from <= j0(s + frame_size - 1) - j0(s) + T - 1
                       = floor((a + (frame_size - 1) * down) / up) - floor(a / up) + T - 1,    a = s * down + half
                      <= ceil((frame_size - 1) * down / up) + T - 1.
    At the front-end's own rate j0(m) = m and no tap reaches back: n <= s + frame_size - 1, keep_from = s, frame_size - 1.
    A flushed stream's next frame starts at or past the end of the recording, which only moves keep_from up.  The bound
    does not depend on hop or on the block lengths (2047 floats at 22.05 kHz, 4158 at 44.1 kHz, 4526 at 48 kHz, 18103
    at 192 kHz for frames of 2048)."""
    if not taps_per_phase:
        return frame_size - 1
    return -(-(frame_size - 1) * down // up) + taps_per_phase - 1


class resample_stream_host(object):
    """resample_host for samples that arrive block by block - the numpy restatement of the resampling half of
    asr_audio_stream_push_dev.  push(block) returns the outputs the block makes final (every input they read has arrived),
    flush() the remaining ones up to ceil(n * up / down), computed with zeros past the end as resample_host does; the
    concatenation equals resample_host on the whole recording bit for bit, whatever the cut.  The object carries the
    input tail the next output still reads."""

    def __init__(self, rate_in, integer=False, rate_out=SAMPLE_RATE):
        self.up, self.down, self.half, self.taps = resample_plan(rate_in, rate_out)
        self.integer = bool(integer)
        self.n_in = 0                                       # input samples so far
        self.n_out = 0                                      # outputs returned so far
        self._tail = np.zeros(0, np.float64)                # inputs self._from .. n_in - 1
        self._from = 0
        self.flushed = False

    def _outputs(self, m0, m1, x, x_from):
        """outputs m0 .. m1 - 1 from inputs x = x[x_from .. n_in): ascending taps, float64 product then float64 sum"""
        up, down, half, hp = self.up, self.down, self.half, self.taps
        T = hp.shape[1]
        m = np.arange(m0, m1, dtype=np.int64)
        c = m * down + half
        p, j0 = c % up, c // up
        acc = np.zeros(m.size, np.float64)
        for t in range(T):
            j = j0 - t
            ok = (j >= 0) & (j < self.n_in)
            acc[ok] = acc[ok] + hp[p[ok], t] * x[j[ok] - x_from]
        if self.integer:
            acc = np.clip(np.rint(acc), -32768, 32767)
        return acc.astype(np.float32)

    def _advance(self, block, m1):
        x = np.concatenate((self._tail, np.ascontiguousarray(block, dtype=np.float32).ravel().astype(np.float64)))
        self.n_in = self._from + x.size
        if m1 is None:
            m1 = _stream_final_outputs(self.n_in, self.up, self.down, self.half, self.taps.shape[1])
        y = self._outputs(self.n_out, m1, x, self._from)
        keep = max(self._from, min(self.n_in, (m1 * self.down + self.half) // self.up - (self.taps.shape[1] - 1)))
        self._tail, self._from, self.n_out = x[keep - self._from:], keep, m1
        return y

    def push(self, block):
        if self.flushed:
            raise ValueError("the stream has been flushed")
        return self._advance(block, None)

    def flush(self):
        if self.flushed:
            raise ValueError("the stream has been flushed")
        self.flushed = True
        return self._advance(np.zeros(0, np.float32), -(-(self._from + self._tail.size) * self.up // self.down))


class AudioStream(object):
    """Spectrogram columns from audio that arrives block by block, for n_streams parallel streams of one sample rate:
    push(blocks) takes one 1-d array of new samples per stream (empty allowed) and returns per stream the
    (num_bins, n_i) float32 columns those samples complete; flush() emits the zero-padded last frames and closes the
    streams.  Whatever the cut into blocks, the concatenated columns of a stream are bit-identical with
    processor.process(recording, sample_rate, integer) on the whole recording.  sample_rate: the rate of the samples
    (None: the processor's); integer: they are 16-bit PCM values (read_audio's flag); window_scale: what read_audio
    returned (None: the processor's).  All streams share rate, integer flag and window scale: one push is one
    asr_audio_stream_push_dev call (csrc/audio_stream_kernels.hip).  The samples the next frames still read stay on the
    device (audio_stream_state_len floats per stream); state and upload buffers are allocated once and reused.
    dft: which transform computes the frames, named explicitly.  None - the direct DFT, for a dft="direct" processor (a
    "fft" processor is refused: it has to ask for its stream by name).  "fft" - the real-input FFT
    (asr_audio_stream_push_fft_dev, csrc/audio_stream_fft_kernels.hip), for a dft="fft" processor only: the same plan,
    state and methods, and the concatenated columns of a stream are bit-identical with
    processor.process(recording, sample_rate, integer) of that same "fft" processor, whatever the cut into blocks and
    whatever the other streams carry.  "direct" - the direct DFT, for a "direct" processor only."""

    def __init__(self, processor, n_streams=1, sample_rate=None, integer=False, window_scale=None, dft=None):
        if n_streams < 1:
            raise ValueError("n_streams must be >= 1")
        if dft not in (None, "direct", "fft"):
            raise ValueError('dft=%r: None, "direct" or "fft"' % (dft,))
        if dft is None and processor.dft != "direct":
            raise ValueError('AudioStream: the streamed front-end is bit-identical with the dft="direct" route and '
                             'computes the direct DFT; this processor was built with dft=%r (its FFT stream has to be '
                             'asked for by name: dft="fft")' % (processor.dft,))
        if dft is not None and dft != processor.dft:
            raise ValueError('AudioStream: dft=%r for a processor built with dft=%r: a stream reproduces the bits of its '
                             'own processor' % (dft, processor.dft))
        self.dft = processor.dft
        self.processor, self.engine, self.n_streams = processor, processor.engine, int(n_streams)
        self.sample_rate = processor.sample_rate if sample_rate is None else sample_rate
        self.integer = bool(integer)
        if self.sample_rate == processor.sample_rate:
            self.up, self.down, self.half, self.taps, self.taps_per_phase = 1, 1, 0, None, 0
        else:
            self.up, self.down, self.half, self.taps = resample_plan(self.sample_rate, processor.sample_rate)
            self.taps_per_phase = self.taps.shape[1]
        scale = processor.window_scale if window_scale is None else float(window_scale)
        self.window = processor.window if scale == processor.window_scale else processor._window(scale)
        self.state_cap = audio_stream_state_len(processor.frame_size, self.up, self.down, self.taps_per_phase)
        self.state_floats = self.n_streams * self.state_cap
        self.state_offsets = np.arange(self.n_streams, dtype=np.int64) * self.state_cap
        self.n_samples = [0] * self.n_streams               # input samples per stream so far
        self.n_frames = [0] * self.n_streams                # frames emitted per stream so far
        self.flushed = [False] * self.n_streams
        self._d_state = self.engine.alloc(max(4, self.state_floats * 4))
        self._d_blocks = self._d_out = None

    def _plan(self, s, n_new, final):
        p = self.processor
        return audio_stream_plan(self.n_samples[s], n_new, final, p.frame_size, p.hop, self.up, self.down, self.half,
                                 self.taps_per_phase)

    def _buffer(self, name, nbytes):
        """the upload / output buffer `name`, grown when a larger push arrives"""
        buf = getattr(self, name)
        if buf is None or buf.nbytes < nbytes:
            if buf is not None:
                buf.free()
            buf = self.engine.alloc(max(4, int(nbytes)))
            setattr(self, name, buf)
        return buf

    def _push(self, blocks, final, out_buf=None):
        """one call -> (buffer, offsets, shapes); out_buf None: a buffer of the caller's (push_dev)"""
        if self._d_state is None:
            raise ValueError("the AudioStream is closed")
        if len(blocks) != self.n_streams:
            raise ValueError("%d blocks for %d streams" % (len(blocks), self.n_streams))
        blocks = [np.ascontiguousarray(b, dtype=np.float32) for b in blocks]
        for s, b in enumerate(blocks):
            if b.ndim != 1:
                raise ValueError("stream %d: expected a 1-d block of samples, got shape %r" % (s, b.shape))
            if self.flushed[s] and (b.size or final[s]):
                raise ValueError("stream %d has been flushed; reset() it before pushing again" % s)
        counts = np.asarray([b.size for b in blocks], np.int64)
        b_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        plans = [self._plan(s, int(counts[s]), final[s]) for s in range(self.n_streams)]
        first = np.asarray([p[0] for p in plans], np.int64)
        n_new = np.asarray([p[1] for p in plans], np.int64)
        nb = self.processor.num_bins
        o_off = np.concatenate([[0], np.cumsum(n_new * nb)[:-1]]).astype(np.int64)
        total_in, out_floats = int(counts.sum()), int(n_new.sum()) * nb
        d_blocks = self._buffer("_d_blocks", total_in * 4)
        if total_in:
            d_blocks.upload(np.concatenate(blocks))
        d_out = self.engine.alloc(max(4, out_floats * 4)) if out_buf is None else self._buffer(out_buf, out_floats * 4)
        p = self.processor
        call = self.engine.audio_stream_push_fft_dev if self.dft == "fft" else self.engine.audio_stream_push_dev
        try:
            call(
                d_blocks.ptr, total_in, b_off, counts, self.n_samples, [1 if f else 0 for f in final], first, n_new, o_off,
                self.up, self.down, self.taps, self.half, self.integer, self._d_state.ptr, self.state_floats,
                self.state_offsets, self.state_cap, p.frame_size, p.hop, self.window, p.fb_start, p.fb_len, p.fb_w,
                d_out.ptr, out_floats, transposed=True)
        except Exception:
            if out_buf is None:
                d_out.free()
            raise
        for s in range(self.n_streams):
            self.n_samples[s] += int(counts[s])
            self.n_frames[s] += int(n_new[s])
            self.flushed[s] = self.flushed[s] or bool(final[s])
        return d_out, [int(o) for o in o_off], [(nb, int(n)) for n in n_new]

    def _download(self, res):
        d_out, offsets, shapes = res
        total = sum(r * c for r, c in shapes)
        flat = d_out.download((total,), np.float32) if total else np.zeros(0, np.float32)
        return [flat[o:o + r * c].reshape(r, c).copy() for o, (r, c) in zip(offsets, shapes)]

    def push_dev(self, blocks):
        """push() that leaves the columns on the device -> piece_identification.DeviceArrays (free its buffer)"""
        from .piece_identification import DeviceArrays
        return DeviceArrays(*self._push(blocks, [False] * self.n_streams))

    def push(self, blocks):
        """one 1-d array of new samples per stream -> list of (num_bins, n_i) float32 arrays, the columns they complete"""
        return self._download(self._push(blocks, [False] * self.n_streams, "_d_out"))

    def _which(self, streams):
        which = range(self.n_streams) if streams is None else [int(s) for s in streams]
        for s in which:
            if not 0 <= s < self.n_streams:
                raise ValueError("stream %d of %d" % (s, self.n_streams))
        return which

    def flush(self, streams=None):
        """the recordings of `streams` (default: all that are open) end here -> list (one entry per stream of the object;
        an empty array for the others) of their remaining columns, the last frames zero padded as process() pads them.
        A flushed stream takes no more samples until reset()."""
        return self._download(self._flush(streams, "_d_out"))

    def flush_dev(self, streams=None):
        """flush() that leaves the columns on the device -> piece_identification.DeviceArrays (free its buffer)"""
        from .piece_identification import DeviceArrays
        return DeviceArrays(*self._flush(streams))

    def _flush(self, streams, out_buf=None):
        if streams is None:
            which = [s for s in range(self.n_streams) if not self.flushed[s]]
        else:
            which = self._which(streams)
        final = [s in which for s in range(self.n_streams)]
        empty = np.zeros(0, np.float32)
        return self._push([empty] * self.n_streams, final, out_buf)

    def reset(self, streams=None):
        """`streams` (default: all) start over: the next push is the first of a new recording"""
        for s in self._which(streams):
            self.n_samples[s], self.n_frames[s], self.flushed[s] = 0, 0, False

    def close(self):
        for name in ("_d_state", "_d_blocks", "_d_out"):
            buf = getattr(self, name)
            if buf is not None:
                buf.free()
            setattr(self, name, None)
