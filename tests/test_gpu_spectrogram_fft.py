"""GPU: the FFT route of the batched audio front-end (asr_spectrogram_fft_batch_dev, SpectrogramProcessor(dft="fft"),
--fast_dft) - accuracy against a float64 spectrogram (tests/spectrogram_fft_ref.py) and against the direct route,
bit-exact independence of a recording's result from the rest of the call, the impulse response, the argument checks,
the Python routes and the driver option.

The deviations measured on an MI355X are in docs/MEASUREMENT_LOG.md (Round 24)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrogram_fft_ref as R  # noqa: E402
from test_gpu_umc import MODEL, SPLIT, CONFIG, TAG, _omr_flags, _umc_dir, exp_root  # noqa: E402,F401

SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def eng():
    from audio_sheet_retrieval_amd import _lib
    e = _lib.Engine(MODEL)
    yield e
    e.close()


def _proc(eng, **kw):
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    return SpectrogramProcessor(eng, **kw)


# ---- 1. accuracy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(4), ids=[s[0] for s in R.signals()])
def test_accuracy_against_the_float64_spectrogram(eng, i):
    name, x, scale = R.signals()[i]
    ref = R.reference(i)
    fft = _proc(eng, window_scale=scale, dft="fft").process(x)
    direct = _proc(eng, window_scale=scale).process(x)
    assert fft.shape == direct.shape == ref.shape and fft.dtype == np.float32
    dev_fft = float(np.abs(fft.astype(np.float64) - ref).max())
    dev_direct = float(np.abs(direct.astype(np.float64) - ref).max())
    print("%s: deviation from the float64 spectrogram: fft %.3g, direct %.3g" % (name, dev_fft, dev_direct))
    assert dev_fft <= 1e-4, (name, dev_fft)
    assert dev_fft <= dev_direct, (name, dev_fft, dev_direct)


# ---- 2. batch invariance, bit for bit --------------------------------------------------------------------------------
# The kernel takes one frame per workgroup (no grouping of frames: a group of 1), so every total is "no multiple of the
# group"; the 60 frames of this call are neither a multiple of the 2048 workgroups of a launch nor of anything else.
LENGTHS = (0, 1, 1101, 1102, 1103, 2047, 2048, 2049, 3307, 50715)


def _recordings():
    rng = np.random.default_rng(7)
    recs = [rng.standard_normal(n).astype(np.float32) * np.float32(0.3) for n in LENGTHS]
    recs[8] = recs[8] * np.float32(1e-3 / 0.3)            # amplitude 1e-3 directly before ...
    recs[9] = recs[9] * np.float32(1.0 / 0.3)             # ... one of amplitude 1.0
    return recs


def _call(eng, proc, recs, transposed, gap=0, fill=None):
    """asr_spectrogram_fft_batch_dev on recs packed back to back -> list of arrays in the layout asked for (and the whole
    output buffer where a fill value is given); gap: floats left free after every recording's output"""
    counts = np.asarray([r.size for r in recs], np.int64)
    frames = np.asarray([proc.num_frames(r.size) for r in recs], np.int64)
    s_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    o_off = np.concatenate([[0], np.cumsum(frames * proc.num_bins + gap)[:-1]]).astype(np.int64)
    out_floats = int((frames * proc.num_bins + gap).sum())
    flat = np.concatenate(recs)
    d_in = eng.alloc(max(4, flat.nbytes)).upload(flat)
    d_out = eng.alloc(max(4, out_floats * 4))
    try:
        if fill is not None:
            d_out.upload(np.full(out_floats, fill, np.float32))
        eng.spectrogram_fft_batch_dev(d_in.ptr, flat.size, s_off, counts, frames, o_off, proc.frame_size, proc.hop,
                                      proc.window, proc.fb_start, proc.fb_len, proc.fb_w, d_out.ptr, out_floats,
                                      transposed=transposed)
        whole = d_out.download((out_floats,), np.float32)
    finally:
        d_in.free()
        d_out.free()
    shape = (lambda n: (proc.num_bins, int(n))) if transposed else (lambda n: (int(n), proc.num_bins))
    outs = [whole[o:o + int(n) * proc.num_bins].reshape(shape(n)) for o, n in zip(o_off, frames)]
    return (outs, whole, o_off, frames) if fill is not None else outs


def test_a_recording_does_not_see_the_rest_of_the_call(eng):
    proc = _proc(eng, dft="fft")
    recs = _recordings()
    s_off = np.concatenate([[0], np.cumsum([r.size for r in recs])[:-1]])
    assert any(int(o) % 2 for o in s_off) and sum(proc.num_frames(r.size) for r in recs) == 60
    together = _call(eng, proc, recs, True)
    assert [t.shape for t in together] == [(92, proc.num_frames(n)) for n in LENGTHS]
    for r, t in zip(recs, together):
        assert np.array_equal(_call(eng, proc, [r], True)[0], t), r.size
    backwards = _call(eng, proc, recs[::-1], True)[::-1]
    for t, b in zip(together, backwards):
        assert np.array_equal(t, b)
    rows = _call(eng, proc, recs, False)
    for t, r in zip(together, rows):
        assert np.array_equal(t, r.T)
    assert all(np.array_equal(a, b) for a, b in zip(together, _call(eng, proc, recs, True)))      # repeated calls agree
    # the quiet recording's zero-padded last frames stay quiet: its loud neighbour would lift every band
    quiet, ref = together[8], R.yardstick(recs[8], proc, proc.window)
    assert np.abs(quiet - ref).max() <= 1e-4 and 10 * quiet[:, -1].max() < together[9][:, 0].max()


# ---- 3. impulse --------------------------------------------------------------------------------------------------------
def test_impulses(eng):
    proc = _proc(eng, dft="fft")
    got = proc.process_many([R.impulse_recording(p) for p in R.IMPULSE_AT])
    for p, g in zip(R.IMPULSE_AT, got):
        want = R.impulse_expected(p, proc)
        assert g.shape == want.shape
        assert np.abs(g - want).max() <= R.IMPULSE_TOL, (p, float(np.abs(g - want).max()))


# ---- 4. arguments ------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_anything_is_written(eng):
    from audio_sheet_retrieval_amd import _lib
    proc = _proc(eng, dft="fft")
    rng = np.random.default_rng(3)
    x = rng.standard_normal(3000).astype(np.float32)
    n, nb = proc.num_frames(x.size), proc.num_bins
    out_floats = n * nb + 50
    d_in = eng.alloc(x.nbytes).upload(x)
    d_out = eng.alloc(out_floats * 4).upload(np.full(out_floats, SENTINEL, np.float32))

    def call(samples_floats=x.size, offsets=(0,), counts=(x.size,), frames=(n,), o_off=(0,), frame_size=2048,
             window=proc.window, fb_start=proc.fb_start, fb_len=proc.fb_len, out_floats=out_floats):
        eng.spectrogram_fft_batch_dev(d_in.ptr, samples_floats, offsets, counts, frames, o_off, frame_size, proc.hop,
                                      window, fb_start, fb_len, proc.fb_w, d_out.ptr, out_floats)

    reach = proc.fb_len.copy()
    reach[-1] = 1025 - proc.fb_start[-1]                                    # the last filter reaches bin 1024
    bad = [dict(frame_size=1024, window=proc.window[:1024]), dict(fb_len=reach), dict(offsets=(1,)),
           dict(counts=(x.size + 1,)), dict(samples_floats=x.size - 1), dict(o_off=(51,)), dict(frames=(n + 1,)),
           dict(out_floats=n * nb - 1), dict(offsets=(-1,)), dict(frames=(-1,))]
    try:
        for kw in bad:
            with pytest.raises(_lib.AsrError) as info:
                call(**kw)
            assert info.value.code == _lib.ASR_ERR_INVALID and "spectrogram_fft_batch" in str(info.value), kw
            assert np.all(d_out.download((out_floats,), np.float32) == SENTINEL), kw
        call(offsets=(), counts=(), frames=(), o_off=())                     # n_recordings == 0
        call(counts=(0,), frames=(0,))                                       # a recording without samples
        assert np.all(d_out.download((out_floats,), np.float32) == SENTINEL)
        call(o_off=(50,))                                                    # a valid call writes its own floats only
        whole = d_out.download((out_floats,), np.float32)
        assert np.all(whole[:50] == SENTINEL) and not np.any(whole[50:] == SENTINEL)
        assert np.array_equal(whole[50:].reshape(nb, n), proc.process(x))
    finally:
        d_in.free()
        d_out.free()


def test_gaps_between_the_outputs_are_left_alone(eng):
    proc = _proc(eng, dft="fft")
    recs = _recordings()[2:9]
    outs, whole, o_off, frames = _call(eng, proc, recs, True, gap=37, fill=SENTINEL)
    covered = np.zeros(whole.size, bool)
    for o, n in zip(o_off, frames):
        covered[o:o + int(n) * proc.num_bins] = True
    assert covered.sum() == whole.size - 37 * len(recs)
    assert np.all(whole[~covered] == SENTINEL) and not np.any(whole[covered] == SENTINEL)
    for a, b in zip(outs, _call(eng, proc, recs, True)):
        assert np.array_equal(a, b)


# ---- 5. routes ---------------------------------------------------------------------------------------------------------
def test_process_many_equals_process(eng):
    proc = _proc(eng, dft="fft")
    (_, x, _), (_, pcm, scale) = R.signals()[0], R.signals()[1]
    recs, scales = [x[:30000], pcm[:20001], x[5:4000]], [1.0, scale, 1.0]
    many = proc.process_many(recs, window_scales=scales)
    for r, s, m in zip(recs, scales, many):
        assert np.array_equal(m, _proc(eng, window_scale=s, dft="fft").process(r))
    # and through the device-side handle
    dev = proc.process_many_dev(recs, window_scales=scales)
    flat = dev.buf.download((sum(r * c for r, c in dev.shapes),), np.float32)
    dev.buf.free()
    assert np.array_equal(flat, np.concatenate([m.ravel() for m in many]))


def test_process_many_with_sample_rates_equals_process_of_the_resampled(eng):
    from audio_sheet_retrieval_amd.audio_frontend import resample_host
    proc = _proc(eng, window_scale=R.INT16_SCALE, dft="fft")
    pcm = R.signals()[1][1]
    recs = [pcm[:30001], pcm[7:9000]]
    many = proc.process_many(recs, sample_rates=[44100, 22050], integer=[True, True])
    assert np.array_equal(many[0], proc.process(resample_host(recs[0], 44100, integer=True)))
    assert np.array_equal(many[1], proc.process(recs[1]))
    assert np.array_equal(many[0], proc.process(recs[0], sample_rate=44100, integer=True))


def test_the_stream_is_refused_and_the_default_is_unchanged(eng):
    with pytest.raises(ValueError):
        _proc(eng, dft="fft").stream()
    x = R.signals()[0][1]
    default, direct = _proc(eng), _proc(eng, dft="direct")
    assert default.dft == "direct"
    n = default.num_frames(x.size)
    d_in = eng.alloc(x.nbytes).upload(x)
    d_out = eng.alloc(n * 92 * 4)
    try:                                                          # today's process(): asr_spectrogram_dev
        eng.spectrogram_dev(d_in.ptr, x.size, 2048, default.hop, default.window, default.fb_start, default.fb_len,
                            default.fb_w, n, d_out.ptr, transposed=True)
        today = d_out.download((92, n), np.float32)
    finally:
        d_in.free()
        d_out.free()
    assert np.array_equal(default.process(x), today) and np.array_equal(direct.process_many([x])[0], today)
    fft = _proc(eng, dft="fft").process(x)
    assert not np.array_equal(fft, today) and np.abs(fft - today).max() <= 1e-4


# ---- 6. driver ---------------------------------------------------------------------------------------------------------
def test_the_driver_takes_fast_dft(exp_root, tmp_path, capsys):  # noqa: F811
    import yaml
    from audio_sheet_retrieval_amd import umc_a2s_server
    data_dir = _umc_dir(tmp_path)
    common = ["--model", "models/%s.py" % MODEL, "--data_dir", data_dir, "--train_split", SPLIT, "--config", CONFIG,
              "--n_candidates", "9", "--full_eval", "--dump_results"] + _omr_flags(exp_root)
    res_file = exp_root / MODEL / ("umc_retrieval_%s_umc_test_A2S.yaml" % TAG)
    results = []
    for extra in (["--init_sheet_db"], ["--fast_dft"]):           # the second run loads the data base of the first
        ranks = umc_a2s_server.main(common + extra)
        with open(res_file) as fp:
            dumped = yaml.safe_load(fp)
        os.remove(res_file)
        assert dumped == ranks and len(ranks) == 4 and all(isinstance(r, int) and r >= 1 for r in ranks)
        results.append(ranks)
    capsys.readouterr()
    with capsys.disabled():                                       # recorded, not asserted: the weights are synthetic
        print("ranks without / with --fast_dft: %r / %r (%s)" % (results[0], results[1],
                                                                "equal" if results[0] == results[1] else "different"))
    with pytest.raises(SystemExit) as e:
        umc_a2s_server.main(common + ["--fast_dft", "--live"])
    assert e.value.code == 2 and "--fast_dft" in capsys.readouterr().err
