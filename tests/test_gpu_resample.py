"""GPU: recordings at any sample rate (asr_resample_batch_dev, csrc/resample_kernels.hip) - the device against the numpy
restatement audio_frontend.resample_host bit for bit (tests/test_resample_host.py holds that one against scipy and the
filter's design), composed with the spectrogram launch, the argument checks, and load_specs(resample=True)."""
import os

import numpy as np
import pytest
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

MODEL = "mutopia_ccal_cont"
SR = 22050
RATES = (44100, 48000, 96000, 32000, 16000, 11025, 8000)
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def eng():
    from audio_sheet_retrieval_amd import _lib
    engine = _lib.Engine(MODEL, device=0)
    yield engine
    engine.close()


def _square(rate, n):
    t = np.arange(n) / float(rate)
    return np.where(np.sin(2 * np.pi * 100.0 * t) >= 0, 32767.0, -32767.0).astype(np.float32)


def _n_in_for(n_out, up, down):
    """the shortest input that gives n_out outputs, ceil(n * up / down) >= n_out: exactly n_out when the rate goes
    down; one more at 11025 Hz, where every count is even"""
    n = n_out * down // up
    while -(-n * up // down) < n_out:
        n += 1
    return n


def _run(eng, recs, rate, integer, gap=3):
    """one resample_batch_dev call on `recs`, each output `gap` floats after the one before -> (outputs per recording,
    every other float of the output buffer)"""
    from audio_sheet_retrieval_amd.audio_frontend import resample_plan
    up, down, half, taps = resample_plan(rate)
    in_counts = np.asarray([r.size for r in recs], np.int64)
    out_counts = -(-in_counts * up // down)
    in_off = np.concatenate([[0], np.cumsum(in_counts)[:-1]]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(out_counts + gap)[:-1]]).astype(np.int64) + gap
    in_floats = int(in_counts.sum())
    out_floats = int(out_off[-1] + out_counts[-1]) + gap
    d_in = eng.alloc(max(4, in_floats * 4)).upload(np.concatenate(recs))
    d_out = eng.alloc(out_floats * 4).upload(np.full(out_floats, SENTINEL, np.float32))
    try:
        eng.resample_batch_dev(d_in.ptr, in_floats, in_off, in_counts, out_off, out_counts, up, down, taps, half, integer,
                               d_out.ptr, out_floats)
        flat = d_out.download((out_floats,), np.float32)
    finally:
        d_in.free()
        d_out.free()
    rest = np.ones(out_floats, bool)
    outs = []
    for o, c in zip(out_off, out_counts):
        outs.append(flat[o:o + c])
        rest[o:o + c] = False
    return outs, flat[rest]


@pytest.mark.parametrize("rate", RATES)
def test_device_equals_host_bit_for_bit(eng, rate):
    from audio_sheet_retrieval_amd.audio_frontend import RESAMPLE_TILE, resample_host, resample_plan
    up, down, _, taps = resample_plan(rate)
    T = taps.shape[1]
    rng = np.random.default_rng(rate)
    lengths = (0, 1, 7, 0, T + 3, _n_in_for(2 * RESAMPLE_TILE + 17, up, down))
    recs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    outs, rest = _run(eng, recs, rate, False)
    assert outs[-1].size == 2 * RESAMPLE_TILE + (18 if rate == 11025 else 17)      # two tiles and a piece of a third
    for r, got in zip(recs, outs):
        want = resample_host(r, rate)
        assert got.shape == want.shape and np.array_equal(got, want), (rate, r.size)
    assert rest.size and np.all(rest == SENTINEL)
    assert float(np.abs(outs[-1]).max()) > 0.1


@pytest.mark.parametrize("rate", [44100, 8000])
def test_integer_mode_equals_host_and_clips(eng, rate):
    from audio_sheet_retrieval_amd.audio_frontend import RESAMPLE_TILE, resample_host, resample_plan
    up, down, _, taps = resample_plan(rate)
    rng = np.random.default_rng(rate + 1)
    long_n = _n_in_for(2 * RESAMPLE_TILE + 17, up, down)
    recs = [np.zeros(0, np.float32), rng.integers(-32768, 32768, size=7).astype(np.float32), np.zeros(0, np.float32),
            rng.integers(-32768, 32768, size=taps.shape[1] + 3).astype(np.float32), _square(rate, long_n)]
    outs, rest = _run(eng, recs, rate, True)
    for r, got in zip(recs, outs):
        want = resample_host(r, rate, integer=True)
        assert got.shape == want.shape and np.array_equal(got, want), (rate, r.size)
        assert np.array_equal(got, np.rint(got))
    assert np.all(rest == SENTINEL)
    assert outs[-1].max() == 32767 and outs[-1].min() == -32768       # the overshoot of the square wave is clipped
    assert resample_host(recs[-1], rate).max() > 32767.5


def test_composition_with_the_spectrogram(eng):
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor, resample_host
    rng = np.random.default_rng(11)
    rates = [44100, SR, 48000, 16000]
    integer = [True, False, False, True]
    scales = [1.0 / 32767, 1.0, 1.0, 1.0 / 32767]
    recs = []
    for rate, flag in zip(rates, integer):
        n = int(rate * 0.4) + 13
        t = np.arange(n) / float(rate)
        x = np.sin(2 * np.pi * 440.0 * t) + 0.1 * rng.standard_normal(n)
        recs.append(np.rint(20000.0 * x).clip(-32768, 32767).astype(np.float32) if flag else x.astype(np.float32))
    proc = SpectrogramProcessor(eng)
    got = proc.process_many(recs, scales, sample_rates=rates, integer=integer)
    host = [r if rate == SR else resample_host(r, rate, integer=f) for r, rate, f in zip(recs, rates, integer)]
    want = proc.process_many(host, scales)
    assert len(got) == len(want) == 4
    for g, w, h in zip(got, want, host):
        assert g.shape == w.shape == (92, proc.num_frames(h.size)) and np.array_equal(g, w)
        assert float(np.abs(g).max()) > 0.1
    # a single recording: process(samples, sample_rate)
    assert np.array_equal(proc.process(recs[2], sample_rate=48000), want[2])
    assert np.array_equal(SpectrogramProcessor(eng, window_scale=scales[0]).process(recs[0], 44100, integer=True), want[0])
    # without sample rates: the path as it was, which process() per recording pins
    plain = proc.process_many(host, scales)
    for h, s, p in zip(host, scales, plain):
        assert np.array_equal(p, SpectrogramProcessor(eng, window_scale=s).process(h))
    # all rates the processor's own: nothing is resampled
    same = proc.process_many(host, scales, sample_rates=[SR] * 4)
    assert all(np.array_equal(a, b) for a, b in zip(same, want))
    assert proc.process_many([], None, sample_rates=[]) == []
    with pytest.raises(ValueError, match="sample rate"):
        proc.process_many(recs[:1], None, sample_rates=[3999])


def test_invalid_arguments_launch_nothing(eng):
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.audio_frontend import resample_plan
    up, down, half, taps = resample_plan(44100)
    x = np.random.default_rng(5).standard_normal(1000).astype(np.float32)
    d_in = eng.alloc(x.nbytes).upload(x)
    d_out = eng.alloc(500 * 4).upload(np.full(500, SENTINEL, np.float32))

    def call(in_floats=1000, in_off=0, in_cnt=1000, out_off=0, out_cnt=500, up=up, down=down, taps=taps, half=half,
             out_floats=500):
        eng.resample_batch_dev(d_in.ptr, in_floats, [in_off], [in_cnt], [out_off], [out_cnt], up, down, taps, half, 0,
                               d_out.ptr, out_floats)

    try:
        for kwargs, message in ((dict(out_cnt=499), "outputs stated"), (dict(in_cnt=998), "outputs stated"),
                                (dict(in_off=1001), "outside its buffers"), (dict(in_off=1), "outside its buffers"),
                                (dict(out_off=1), "outside its buffers"), (dict(up=0), "at least 1"),
                                (dict(down=0), "at least 1"),
                                (dict(taps=np.ascontiguousarray(taps[:, :-1])), "taps per phase")):
            with pytest.raises(_lib.AsrError, match=message) as info:
                call(**kwargs)
            assert info.value.code == _lib.ASR_ERR_INVALID, kwargs
        assert np.all(d_out.download((500,), np.float32) == SENTINEL)
        call()                                                   # the same call with nothing wrong writes every float
        assert not np.any(d_out.download((500,), np.float32) == SENTINEL)
        # nothing to do is not an error
        eng.resample_batch_dev(d_in.ptr, 1000, [], [], [], [], up, down, taps, half, 0, d_out.ptr, 500)
        eng.resample_batch_dev(d_in.ptr, 1000, [5], [0], [7], [0], up, down, taps, half, 0, d_out.ptr, 500)
    finally:
        d_in.free()
        d_out.free()


def test_load_specs_resamples(eng, tmp_path):
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor, resample_host
    from audio_sheet_retrieval_amd.sheet_utils.umc import load_specs
    rng = np.random.default_rng(8)
    pcm = rng.integers(-20000, 20000, size=(44100 // 2 + 5, 2)).astype(np.int16)
    flt = (0.3 * rng.standard_normal(48000 // 2 + 9)).astype(np.float32)
    own = (0.3 * rng.standard_normal(SR // 2 + 1)).astype(np.float32)
    paths = []
    for name, write in (("a", lambda d: wavfile.write(os.path.join(d, "score_ppq.wav"), 44100, pcm)),
                        ("b", lambda d: wavfile.write(os.path.join(d, "score_ppq.wav"), 48000, flt)),
                        ("c", lambda d: np.save(os.path.join(d, "score_ppq.npy"), own))):
        d = str(tmp_path / name)
        os.makedirs(d)
        write(d)
        paths.append(d)
    proc = SpectrogramProcessor(eng)
    mono = np.mean(pcm, axis=-1).astype(np.int16).astype(np.float32)
    host = [resample_host(mono, 44100, integer=True), resample_host(flt, 48000), own]
    want = proc.process_many(host, [1.0 / 32767, 1.0, 1.0])
    got = load_specs(paths, "score_ppq", proc, resample=True)
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want))
    dev = load_specs(paths, "score_ppq", proc, return_device=True, resample=True)
    try:
        assert dev.shapes == [w.shape for w in want]
        total = sum(r * c for r, c in dev.shapes)
        flat = dev.buf.download((total,), np.float32)
        for o, (r, c), w in zip(dev.offsets, dev.shapes, want):
            assert np.array_equal(flat[o:o + r * c].reshape(r, c), w)
    finally:
        dev.buf.free()
    with pytest.raises(ValueError, match="sample rate 44100 Hz"):
        load_specs(paths, "score_ppq", proc)
