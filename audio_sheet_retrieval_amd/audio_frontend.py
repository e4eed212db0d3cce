"""Audio front-end on the GPU: waveform -> the (92, frames) log-frequency spectrogram the
spectrogram tower takes, i.e. the madmom processor chain of the reference (tutorials/Embedding Tutorial.ipynb cell 28;
`processor.process(audio_file).T` at audio_sheet_server.py:632,678, audio2sheet_align.py:99):

    SignalProcessor(num_channels=1, sample_rate=22050) -> FramedSignalProcessor(frame_size=2048, fps=20, origin='future')
    -> FilteredSpectrogramProcessor(LogarithmicFilterbank, num_bands=16, fmin=30, fmax=6000)
    -> LogarithmicSpectrogramProcessor()

`process(samples)` takes mono samples at SAMPLE_RATE; `load_audio(path)` reads them from a .wav or .npy file.  Decoding
compressed formats and resampling (ffmpeg inside madmom) stay with the caller.  The filterbank is built on the host with madmom's published construction (third-party
semantic, unverified offline; it reproduces the reference's 92 bands); framing, windowed DFT magnitudes,
filterbank and logarithm run in one kernel per call (csrc/piece_vote_kernels.hip: spectrogram_kernel).
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


def load_audio(path, sample_rate=SAMPLE_RATE):
    """-> (mono float32 samples, window_scale) of a .wav (PCM 16-bit or float32) or .npy (mono float samples) file -
    what madmom's SignalProcessor(num_channels=1, sample_rate=22050) hands on.  Channels are averaged.  16-bit PCM
    keeps its integer values and comes with window_scale = 1 / 32767 (madmom scales the STFT window by the integer
    range instead of the samples); float input has window_scale 1.  A file at another rate is an error: resampling is
    the caller's."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        samples = np.load(path)
        if samples.ndim != 1 or samples.dtype.kind != "f":
            raise ValueError("%s: expected mono float samples (1-d), got %s %r" % (path, samples.dtype, samples.shape))
        return np.ascontiguousarray(samples, dtype=np.float32), 1.0
    if ext != ".wav":
        raise ValueError("%s: no decoder for '%s' files is part of this implementation; convert the recording to "
                         "a %d Hz .wav (PCM 16-bit or float32) or .npy (mono float samples) file" %
                         (path, ext or "extension-less", sample_rate))
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if rate != sample_rate:
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
    return np.ascontiguousarray(data, dtype=np.float32), scale


class SpectrogramProcessor(object):
    """processor = SequentialProcessor([sig_proc, fsig_proc, spec_proc, log_spec_proc]) of the reference, on the GPU."""

    def __init__(self, engine, sample_rate=SAMPLE_RATE, frame_size=FRAME_SIZE, fps=FPS, window_scale=1.0):
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

    def process_dev(self, samples):
        """-> (DeviceBuffer holding the (num_bins, n_frames) float32 spectrogram, n_frames)"""
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

    def process(self, samples):
        """the reference's `processor.process(audio).T`: (num_bins, n_frames) float32"""
        d_out, n = self.process_dev(samples)
        out = d_out.download((self.num_bins, n), np.float32)
        d_out.free()
        return out

    def process_many_dev(self, recordings, window_scales=None):
        """process_dev for a list of recordings of any lengths (an empty one gives no frames) in one launch
        (asr_spectrogram_batch_dev) -> piece_identification.DeviceArrays: the (num_bins, n_frames_i) spectrograms back
        to back in one device buffer, each bit-identical with process()'s.  window_scales: one per recording (what
        load_audio returned; default: the processor's) - recordings of equal scale share a launch."""
        from .piece_identification import DeviceArrays
        recs = [np.ascontiguousarray(r, dtype=np.float32).ravel() for r in recordings]
        scales = [self.window_scale] * len(recs) if window_scales is None else [float(w) for w in window_scales]
        if len(scales) != len(recs):
            raise ValueError("%d window scales for %d recordings" % (len(scales), len(recs)))
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
                eng.spectrogram_batch_dev(d_in.ptr, flat.size, s_off[sel], counts[sel], frames[sel], o_off[sel],
                                          self.frame_size, self.hop, window, self.fb_start, self.fb_len, self.fb_w,
                                          d_out.ptr, out_floats, transposed=True)
        except Exception:
            d_out.free()
            raise
        finally:
            d_in.free()
        return DeviceArrays(d_out, [int(o) for o in o_off], [(self.num_bins, int(n)) for n in frames])

    def process_many(self, recordings, window_scales=None):
        """process() for a list of recordings in one launch -> list of (num_bins, n_frames_i) float32 arrays"""
        dev = self.process_many_dev(recordings, window_scales)
        try:
            total = sum(r * c for r, c in dev.shapes)
            flat = dev.buf.download((total,), np.float32) if total else np.zeros(0, np.float32)
        finally:
            dev.buf.free()
        return [flat[o:o + r * c].reshape(r, c).copy() for o, (r, c) in zip(dev.offsets, dev.shapes)]
