"""GPU: spectrogram columns from streamed audio blocks by the FFT (asr_audio_stream_push_fft_dev,
csrc/audio_stream_fft_kernels.hip, AudioStream(dft="fft"), live_track_scores(dft="fft"), umc_a2s_server --live_dft fft).
The yardstick is the whole-recording route of the same processor, SpectrogramProcessor(dft="fft").process(recording,
sample_rate) = asr_resample_batch_dev + asr_spectrogram_fft_batch_dev, and every comparison is exact (np.array_equal):
whatever the cut into blocks and whatever the other streams, the concatenated columns are the same bits.  That is also
the proof that the two translation units compile the shared frame body (csrc/spectrogram_fft_frame.h) to the same
arithmetic.

Shapes of tests/test_gpu_audio_stream.py: recordings of 0.62 s have 13 frames, 11 of them complete before the flush."""
import os
import sys

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_gpu_audio_stream import MODEL, SENTINEL, _recording, _same_track, _stream_whole  # noqa: E402
from test_gpu_umc import KEPT, TAG, _omr_flags, _umc_dir, exp_root  # noqa: E402,F401

RATES = (22050, 44100, 48000, 16000, 8000)


@pytest.fixture(scope="module")
def engine():
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine(MODEL)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def proc(engine):
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    return SpectrogramProcessor(engine, dft="fft")


@pytest.fixture(scope="module")
def whole(proc):
    """rate -> (recording, proc.process of it), computed once"""
    out = {}
    for rate in RATES:
        rec = _recording(rate, 0.62, rate)
        out[rate] = (rec, proc.process(rec, sample_rate=rate))
    return out


# ---- 1. bit equality with the whole-recording FFT route ---------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_any_cut_gives_the_bits_of_the_whole_recording(proc, whole, rate):
    """22050: no taps; 44100: up == 1; 48000: gathered phases; 16000, 8000: upsampling.  A difference at 22050 would be in
    the FFT body, not in the resampler"""
    rec, want = whole[rate]
    assert want.shape == (92, 13)
    stream = proc.stream(sample_rate=rate, dft="fft")
    try:
        assert stream.dft == "fft"
        taps = max(stream.taps_per_phase, 33)
        # an empty block, one sample, fewer samples than a phase has taps, whole frames, and a block longer than the rest
        first = [0, 1, taps - 16, 0, 1, rec.size // 3, 7, rec.size // 4, 0, 10 * rec.size]
        got, before = _stream_whole(stream, rec, first)
        assert before == 11 and stream.n_frames == [13] and stream.flushed == [True]
        assert got.shape == want.shape and np.array_equal(got, want)
        with pytest.raises(ValueError):
            stream.push([rec[:1]])
        stream.reset()                                                  # a second, different cut on the same object
        assert stream.n_samples == [0] and stream.n_frames == [0] and stream.flushed == [False]
        second = [rec.size // 2 + 3] + [997] * (rec.size // 997 + 1)
        again, before = _stream_whole(stream, rec, second)
        assert before == 11 and np.array_equal(again, want)
    finally:
        stream.close()


# ---- 2. the twiddle table is there for a context whose first FFT call is a stream push ----------------------------------
def test_the_first_call_of_a_fresh_engine_is_a_stream_push():
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    eng = _lib.Engine(MODEL)
    try:
        fresh = SpectrogramProcessor(eng, dft="fft")
        rec = _recording(44100, 0.62, 44100)
        stream = fresh.stream(sample_rate=44100, dft="fft")
        try:
            got, before = _stream_whole(stream, rec, [rec.size // 2, 10 * rec.size])
        finally:
            stream.close()
        want = fresh.process(rec, sample_rate=44100)                    # the batched call comes second
        assert before == 11 and want.shape == (92, 13) and np.array_equal(got, want)
    finally:
        eng.close()


# ---- 3. more frames than CUs in one call ---------------------------------------------------------------------------------
def test_more_frames_than_compute_units_in_one_call(proc, whole):
    rec, want = whole[48000]
    n = 24                                                              # 24 x 11 frames in one call: above 256
    stream = proc.stream(n_streams=n, sample_rate=48000, dft="fft")
    try:
        cols = stream.push([rec] * n)
        assert stream.n_frames == [11] * n
        last = stream.flush()
        for a, b in zip(cols, last):
            assert np.array_equal(np.hstack([a, b]), want)
    finally:
        stream.close()


# ---- 4. several streams of one object ------------------------------------------------------------------------------------
def test_streams_do_not_see_each_other(proc):
    rate = 44100
    recs = [_recording(rate, sec, 50 + k) for k, sec in enumerate((0.62, 0.41, 0.3))]
    want = proc.process_many(recs, None, [rate] * 3)
    step = [4410, 3000, 5000]

    def run(which):
        """the streams `which` of the schedule below in one object -> their columns"""
        stream = proc.stream(n_streams=len(which), sample_rate=rate, dft="fft")
        try:
            parts = [[] for _ in which]
            pos = [0] * len(which)
            for it in range(12):
                blocks = []
                for k, s in enumerate(which):
                    idle = s == 1 and 1 <= it <= 3                      # stream 1: empty blocks for three pushes
                    blocks.append(recs[s][pos[k]:pos[k] + (0 if idle or stream.flushed[k] else step[s])])
                    pos[k] += blocks[-1].size
                for k, c in enumerate(stream.push(blocks)):
                    parts[k].append(c)
                # a stream whose recording has ended is flushed while the others go on
                ended = [k for k, s in enumerate(which) if pos[k] >= recs[s].size and not stream.flushed[k]]
                if ended:
                    for k, c in enumerate(stream.flush(ended)):
                        parts[k].append(c)
            assert all(stream.flushed)
            return [np.hstack(p) for p in parts]
        finally:
            stream.close()

    together = run([0, 1, 2])
    for s in range(3):
        alone = run([s])[0]
        assert np.array_equal(together[s], alone), s
        assert np.array_equal(together[s], want[s]), s


# ---- 5. 16-bit sources ---------------------------------------------------------------------------------------------------
def test_integer_mode_rounds_and_clips(engine):
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor, resample_host
    rate = 44100
    n = int(0.62 * rate)
    rec = np.where((np.arange(n) // 37) % 2 == 0, 32767.0, -32767.0).astype(np.float32)    # the filter overshoots
    y = resample_host(rec, rate, integer=True)
    assert y.max() == 32767.0 and y.min() == -32768.0                   # the clip is reached on both sides
    scaled = SpectrogramProcessor(engine, window_scale=1.0 / 32767, dft="fft")
    want = scaled.process(rec, rate, integer=True)
    assert not np.array_equal(want, scaled.process(rec, rate, integer=False))
    stream = scaled.stream(sample_rate=rate, integer=True, dft="fft")
    try:
        got, _ = _stream_whole(stream, rec, [5000, 1, 0, 8000, 3, 10 * n])
        assert np.array_equal(got, want)
    finally:
        stream.close()


# ---- 6. the sample that completes a frame emits it ---------------------------------------------------------------------
def test_a_frame_appears_with_its_last_sample(proc, whole):
    rec, want = whole[22050]
    stream = proc.stream(dft="fft")
    try:
        pos = 0
        for i in (0, 1, 5):
            end = int(i * proc.hop) + 2048
            got = stream.push([rec[pos:end - 1]])[0]
            assert stream.n_frames == [i]                               # one sample short: frame i is not out
            assert np.array_equal(got, want[:, i - got.shape[1]:i])
            got = stream.push([rec[end - 1:end]])[0]                    # the sample that completes it
            assert got.shape == (92, 1) and np.array_equal(got[:, 0], want[:, i]) and stream.n_frames == [i + 1]
            pos = end
    finally:
        stream.close()


# ---- 7, 8. the call itself -------------------------------------------------------------------------------------------------
class _Raw(object):
    """Engine.audio_stream_push_fft_dev on buffers with room around every range, filled with a sentinel"""

    def __init__(self, engine, proc, n_streams, rate, gap=37):
        from audio_sheet_retrieval_amd import audio_frontend as af
        self.eng, self.p, self.n, self.gap = engine, proc, n_streams, gap
        self.up, self.down, self.half, self.taps = af.resample_plan(rate)
        self.T = self.taps.shape[1]
        self.cap = af.audio_stream_state_len(proc.frame_size, self.up, self.down, self.T)
        self.state_offsets = gap + np.arange(n_streams, dtype=np.int64) * (self.cap + gap)
        self.state_floats = int(self.state_offsets[-1]) + self.cap + gap
        self.d_state = engine.alloc(self.state_floats * 4).upload(np.full(self.state_floats, SENTINEL))
        self.before = [0] * n_streams

    def state(self):
        return self.d_state.download((self.state_floats,), np.float32)

    def call(self, blocks, final, transposed=True, **wrong):
        """-> (columns per stream as (92, n), the whole output buffer, the mask of the floats the streams own); wrong:
        arguments replaced to provoke a refusal - the call then raises, after the checks of what it left behind"""
        from audio_sheet_retrieval_amd import audio_frontend as af
        p, gap = self.p, self.gap
        counts = np.asarray([b.size for b in blocks], np.int64)
        plans = [af.audio_stream_plan(self.before[s], counts[s], final[s], p.frame_size, p.hop, self.up, self.down,
                                      self.half, self.T) for s in range(self.n)]
        first, new = [q[0] for q in plans], np.asarray([q[1] for q in plans], np.int64)
        b_off = gap + np.concatenate([[0], np.cumsum(counts + gap)[:-1]]).astype(np.int64)
        o_off = gap + np.concatenate([[0], np.cumsum(new * p.num_bins + gap)[:-1]]).astype(np.int64)
        flat = np.full(int(b_off[-1] + counts[-1] + gap), SENTINEL)
        for b, o in zip(blocks, b_off):
            flat[o:o + b.size] = b
        out_floats = int(o_off[-1] + new[-1] * p.num_bins + gap)
        a = dict(n_new_frames=new, state_offsets=self.state_offsets, frame_size=p.frame_size, window=p.window,
                 fb_len=p.fb_len, fb_w=p.fb_w)
        a.update(wrong)
        d_blocks = self.eng.alloc(flat.nbytes).upload(flat)
        d_out = self.eng.alloc(out_floats * 4).upload(np.full(out_floats, SENTINEL))
        try:
            state_before = self.state()
            try:
                self.eng.audio_stream_push_fft_dev(
                    d_blocks.ptr, flat.size, b_off, counts, self.before, [1 if f else 0 for f in final], first,
                    a["n_new_frames"], o_off, self.up, self.down, self.taps, self.half, False, self.d_state.ptr,
                    self.state_floats, a["state_offsets"], self.cap, a["frame_size"], p.hop, a["window"], p.fb_start,
                    a["fb_len"], a["fb_w"], d_out.ptr, out_floats, transposed=transposed)
            except Exception:
                # a refused call has touched neither the state nor the output
                assert np.array_equal(self.state(), state_before)
                assert np.all(d_out.download((out_floats,), np.float32) == SENTINEL)
                raise
            out = d_out.download((out_floats,), np.float32)
        finally:
            d_blocks.free()
            d_out.free()
        held = np.zeros(out_floats, bool)
        cols = []
        for s in range(self.n):
            o, m = int(o_off[s]), int(new[s]) * p.num_bins
            held[o:o + m] = True
            own = out[o:o + m]
            cols.append((own.reshape(p.num_bins, int(new[s])) if transposed else own.reshape(int(new[s]), p.num_bins).T).copy())
            self.before[s] += int(counts[s])
        return cols, out, held

    def close(self):
        self.d_state.free()


def test_layout_and_gaps(engine, proc):
    rate = 44100
    recs = [_recording(rate, 0.3, 70), _recording(rate, 0.41, 71)]
    want = proc.process_many(recs, None, [rate] * 2)
    got = {}
    for transposed in (True, False):
        raw = _Raw(engine, proc, 2, rate)
        try:
            parts = [[], []]
            for blocks, final in (([r[:9000] for r in recs], [False, False]), ([r[9000:] for r in recs], [True, True])):
                cols, out, held = raw.call(blocks, final, transposed=transposed)
                assert held.any() and not held.all()
                assert np.all(out[~held] == SENTINEL)                   # every float outside the streams' ranges
                assert not np.any(out[held] == SENTINEL)
                for s in range(2):
                    parts[s].append(cols[s])
            state = raw.state()
            owned = np.zeros(raw.state_floats, bool)
            for o in raw.state_offsets:
                owned[o:o + raw.cap] = True
            assert np.all(state[~owned] == SENTINEL)
            got[transposed] = [np.hstack(q) for q in parts]
        finally:
            raw.close()
    for s in range(2):
        assert got[True][s].shape == want[s].shape and want[s].shape[1] > 2
        assert np.array_equal(got[True][s], want[s]) and np.array_equal(got[False][s], want[s]), s


def test_refused_calls_launch_nothing(engine, proc, whole):
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    rate = 44100
    recs = [_recording(rate, 0.3, 70), _recording(rate, 0.3, 71)]
    raw = _Raw(engine, proc, 2, rate)
    try:
        raw.call([r[:6000] for r in recs], [False, False])              # a state worth keeping: one frame is out
        nxt = [r[6000:9000] for r in recs]
        fb_len = proc.fb_len.copy()
        fb_len[-1] = 1025 - proc.fb_start[-1]                           # the last filter reaches bin 1024
        fb_w = np.concatenate([proc.fb_w, np.zeros(1024, np.float32)])
        wrong = [
            dict(frame_size=1024, window=proc.window[:1024]),
            dict(fb_len=fb_len, fb_w=fb_w),
            dict(n_new_frames=np.asarray([1, 2], np.int64)),            # stream 0 completes two frames, not one
            dict(state_offsets=np.asarray([raw.state_offsets[0], raw.state_offsets[0] + raw.cap - 1], np.int64)),
        ]
        for w in wrong:
            with pytest.raises(_lib.AsrError) as err:
                raw.call(nxt, [False, False], **w)
            assert err.value.code == _lib.ASR_ERR_INVALID and "audio_stream_push_fft" in str(err.value), w
        # ... and the stream goes on as if nothing had been tried
        a = raw.call(nxt, [False, False])[0]
        b = raw.call([r[9000:] for r in recs], [True, True])[0]
        want = proc.process_many(recs, None, [rate] * 2)
        for s in range(2):
            assert np.array_equal(np.hstack([want[s][:, :1], a[s], b[s]]), want[s])
    finally:
        raw.close()
    # the transform of a stream is its processor's, named explicitly for the FFT
    direct = SpectrogramProcessor(engine)
    for p, kw in ((direct, dict(dft="fft")), (proc, dict(dft="direct")), (proc, dict())):
        with pytest.raises(ValueError):
            p.stream(**kw)
    rec, fft_bits = whole[22050]
    stream = direct.stream()                                            # today's stream, today's bits
    try:
        assert stream.dft == "direct"
        got, _ = _stream_whole(stream, rec, [rec.size // 2, 10 * rec.size])
    finally:
        stream.close()
    assert np.array_equal(got, direct.process(rec)) and not np.array_equal(got, fft_bits)


# ---- 9. samples in, ranking out ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tracking(engine, proc):
    """(data base, recordings, rates, track_scores on the finished FFT spectrograms), computed once"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        engine.set_params([z["p%02d" % i] for i in range(len(param_shapes(MODEL)))])
    rng = np.random.default_rng(8)
    n_pieces = 11
    codes = rng.standard_normal((700, 32)).astype(np.float32)
    ids = np.sort(rng.integers(0, n_pieces, size=700))
    db = pid.EmbeddingDB(engine, codes, ids, {i: "piece_%02d" % i for i in range(n_pieces)})
    rates = [44100, 22050, 44100]
    recs = [_recording(r, sec, 90 + k) for k, (r, sec) in enumerate(zip(rates, (3.0, 3.1, 2.4)))]
    want = pid.track_scores(engine, db, proc.process_many(recs, None, rates), 3, 5, 10, return_idx=True)
    yield db, recs, rates, want
    db.close()


@pytest.mark.parametrize("batched", [False, True])
def test_live_tracking_equals_tracking_the_finished_spectrograms(engine, proc, tracking, batched):
    from audio_sheet_retrieval_amd import piece_identification as pid
    db, recs, rates, want = tracking
    assert all(len(w.frames) > 5 for w in want)                         # the gate opens: the vote is exercised
    got = pid.live_track_scores(engine, db, proc, recs, rates, [r // 10 for r in rates], None, 3, 5, 10,
                                batched=batched, dft="fft")
    assert len(got) == 3
    for g, w in zip(got, want):
        _same_track(g, w)


# ---- 10. the driver --------------------------------------------------------------------------------------------------------
def test_driver_live_dft_fft_dumps_the_tracking(exp_root, tmp_path, capsys):  # noqa: F811
    from audio_sheet_retrieval_amd import umc_a2s_server
    data_dir = _umc_dir(tmp_path)
    common = ["--model", "models/%s.py" % MODEL, "--data_dir", data_dir, "--train_split", "splits/all_split.yaml",
              "--config", "exp_configs/mutopia_full_aug.yaml", "--n_candidates", "5"] + _omr_flags(exp_root)
    res = umc_a2s_server.main(common + ["--init_sheet_db", "--live", "--live_dft", "fft", "--block_ms", "100",
                                        "--resample", "--dump_results"])
    text = capsys.readouterr().out
    with open(exp_root / MODEL / ("umc_tracking_%s_umc_test_A2S.yaml" % TAG)) as fp:
        dumped = yaml.safe_load(fp)
    names = [n for n in KEPT if n != "p7_no_score_ppq"]
    assert dumped == res and sorted(dumped) == ["first_lead", "lead_share"]
    assert len(dumped["first_lead"]) == len(dumped["lead_share"]) == len(names) == text.count("of the voiced frames")
    with pytest.raises(SystemExit) as e:
        umc_a2s_server.main(common + ["--live_dft", "fft"])
    assert e.value.code == 2 and "--live_dft" in capsys.readouterr().err
