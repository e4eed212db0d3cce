"""GPU: spectrogram columns from streamed audio blocks (asr_audio_stream_push_dev, csrc/audio_stream_kernels.hip,
audio_frontend.AudioStream, piece_identification.live_track_scores, umc_a2s_server --live).  The yardstick is the
whole-recording route, processor.process(recording, sample_rate) = asr_resample_batch_dev + asr_spectrogram_batch_dev,
and every comparison is exact: whatever the cut into blocks, the concatenated columns are the same bits.

Product processor: frames of 2048 at 20 fps, 92 bands.  Recordings of 0.62 s have 13 frames, 11 of them complete
before the flush."""
import os
import sys

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL = "mutopia_ccal_cont"
SENTINEL = np.float32(-1234.5)


@pytest.fixture(scope="module")
def engine():
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine(MODEL)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def processor(engine):
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    return SpectrogramProcessor(engine)


def _recording(rate, seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    t = np.arange(n) / float(rate)
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in
            zip(rng.uniform(0.1, 0.4, 4), rng.uniform(80, 3000, 4), rng.uniform(0, 6, 4)))
    return (x / np.abs(x).max() * 0.8 + 0.01 * rng.standard_normal(n)).astype(np.float32)


def _stream_whole(stream, rec, sizes):
    """push `rec` in blocks of `sizes` (the last one takes what is left), flush -> (columns, frames before the flush)"""
    parts, pos = [], 0
    for n in sizes:
        block = rec[pos:pos + n]
        pos += block.size
        got = stream.push([block])
        assert len(got) == 1 and got[0].dtype == np.float32 and got[0].shape[0] == stream.processor.num_bins
        parts.append(got[0])
    assert pos == rec.size and stream.n_samples == [rec.size]
    before = sum(p.shape[1] for p in parts)
    parts.append(stream.flush()[0])
    return np.hstack(parts), before


# ---- 1. bit equality with the whole-recording route ---------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(processor):
    """rate -> (recording, processor.process of it), computed once"""
    out = {}
    for rate in (22050, 44100, 48000, 16000, 8000):
        rec = _recording(rate, 0.62, rate)
        out[rate] = (rec, processor.process(rec, sample_rate=rate))
    return out


@pytest.mark.parametrize("rate", [22050, 44100, 48000, 16000, 8000])
def test_any_cut_gives_the_bits_of_the_whole_recording(processor, whole, rate):
    rec, want = whole[rate]
    assert want.shape == (92, 13)
    stream = processor.stream(sample_rate=rate)
    try:
        taps = max(stream.taps_per_phase, 33)
        # an empty block, one sample, fewer samples than a phase has taps, whole frames, and a block longer than the rest
        first = [0, 1, taps - 16, 0, 1, rec.size // 3, 7, rec.size // 4, 0, 10 * rec.size]
        got, before = _stream_whole(stream, rec, first)
        assert before == 11 and stream.n_frames == [13] and stream.flushed == [True]
        assert got.shape == want.shape and np.array_equal(got, want)
        with pytest.raises(ValueError):
            stream.push([rec[:1]])
        # a second, different cut on the same object
        stream.reset()
        assert stream.n_samples == [0] and stream.n_frames == [0] and stream.flushed == [False]
        second = [rec.size // 2 + 3] + [997] * (rec.size // 997 + 1)
        again, before = _stream_whole(stream, rec, second)
        assert before == 11 and np.array_equal(again, want)
    finally:
        stream.close()


@pytest.mark.parametrize("parts", ["1", "2", "8", None])
def test_splitting_a_frame_over_workgroups_changes_no_bit(processor, whole, monkeypatch, parts):
    """a call with fewer frames than CUs splits a frame's filters over several workgroups (three for these frames);
    ASR_STREAM_PARTS forces the number.  None: the rule itself, with more frames than CUs in one push (no split)"""
    rec, want = whole[48000]
    if parts is not None:
        monkeypatch.setenv("ASR_STREAM_PARTS", parts)
        stream = processor.stream(sample_rate=48000)
        try:
            got, _ = _stream_whole(stream, rec, [rec.size // 2, 5, 10 * rec.size])
            assert np.array_equal(got, want)
        finally:
            stream.close()
        return
    n = 24                                                                  # 24 x 11 frames in one call: above 256
    stream = processor.stream(n_streams=n, sample_rate=48000)
    try:
        cols = stream.push([rec] * n)
        assert stream.n_frames == [11] * n
        last = stream.flush()
        for a, b in zip(cols, last):
            assert np.array_equal(np.hstack([a, b]), want)
    finally:
        stream.close()


# ---- 2. the sample that completes a frame emits it ------------------------------------------------------------------
def test_a_frame_appears_with_its_last_sample(processor, whole):
    rec, want = whole[22050]
    stream = processor.stream()
    try:
        pos = 0
        for i in (0, 1, 5):
            end = int(i * processor.hop) + 2048
            got = stream.push([rec[pos:end - 1]])[0]
            assert stream.n_frames == [i]                                   # one sample short: frame i is not out
            assert np.array_equal(got, want[:, i - got.shape[1]:i])
            got = stream.push([rec[end - 1:end]])[0]                        # the sample that completes it
            assert got.shape == (92, 1) and np.array_equal(got[:, 0], want[:, i]) and stream.n_frames == [i + 1]
            pos = end
    finally:
        stream.close()


# ---- 3. several streams of one object -------------------------------------------------------------------------------
class _Raw(object):
    """the call itself on buffers with room around every range, filled with a sentinel"""

    def __init__(self, engine, processor, n_streams, rate, integer=False, gap=37):
        from audio_sheet_retrieval_amd import audio_frontend as af
        self.eng, self.p, self.n, self.gap, self.integer = engine, processor, n_streams, gap, integer
        if rate == processor.sample_rate:
            self.up, self.down, self.half, self.taps, self.T = 1, 1, 0, None, 0
        else:
            self.up, self.down, self.half, self.taps = af.resample_plan(rate)
            self.T = self.taps.shape[1]
        self.cap = af.audio_stream_state_len(processor.frame_size, self.up, self.down, self.T)
        self.state_offsets = gap + np.arange(n_streams, dtype=np.int64) * (self.cap + gap)
        self.state_floats = int(self.state_offsets[-1]) + self.cap + gap
        self.d_state = engine.alloc(self.state_floats * 4).upload(np.full(self.state_floats, SENTINEL))
        self.before = [0] * n_streams
        self.bufs = [self.d_state]

    def state(self):
        return self.d_state.download((self.state_floats,), np.float32)

    def state_gaps(self):
        s = self.state()
        held = np.zeros(self.state_floats, bool)
        for o in self.state_offsets:
            held[o:o + self.cap] = True
        return s[~held]

    def call(self, blocks, final, **wrong):
        """-> columns per stream; wrong: arguments replaced to provoke a refusal (the call then raises)"""
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
        d_blocks = self.eng.alloc(flat.nbytes).upload(flat)
        d_out = self.eng.alloc(out_floats * 4).upload(np.full(out_floats, SENTINEL))
        a = dict(blocks_floats=flat.size, block_offsets=b_off, block_counts=counts, n_new_frames=new,
                 state_offsets=self.state_offsets, state_cap=self.cap, state_floats=self.state_floats, up=self.up,
                 down=self.down, taps=self.taps, half=self.half)
        a.update(wrong)
        try:
            state_before = self.state()
            try:
                self.eng.audio_stream_push_dev(
                    d_blocks.ptr, a["blocks_floats"], a["block_offsets"], a["block_counts"], self.before,
                    [1 if f else 0 for f in final], first, a["n_new_frames"], o_off, a["up"], a["down"], a["taps"],
                    a["half"], self.integer, self.d_state.ptr, a["state_floats"], a["state_offsets"], a["state_cap"],
                    p.frame_size, p.hop, p.window, p.fb_start, p.fb_len, p.fb_w, d_out.ptr, out_floats)
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
            cols.append(out[o:o + m].reshape(p.num_bins, int(new[s])).copy())
            self.before[s] += int(counts[s])
        assert np.all(out[~held] == SENTINEL) and np.all(self.state_gaps() == SENTINEL)
        return cols

    def close(self):
        for b in self.bufs:
            b.free()


def test_streams_of_one_object_do_not_touch_each_other(engine, processor):
    rate = 44100
    recs = [_recording(rate, sec, 50 + k) for k, sec in enumerate((0.62, 0.41, 0.3))]
    want = processor.process_many(recs, None, [rate] * 3)
    raw = _Raw(engine, processor, 3, rate)
    try:
        parts = [[], [], []]
        pos, done = [0, 0, 0], [False, False, False]
        step = [4410, 3000, 5000]
        for it in range(12):
            blocks, final = [], []
            for s in range(3):
                idle = s == 1 and 1 <= it <= 3                               # stream 1: empty blocks for three pushes
                n = 0 if (idle or done[s]) else step[s]
                blocks.append(recs[s][pos[s]:pos[s] + n])
                pos[s] += blocks[-1].size
                # stream 2 is flushed early (with its last block) while the others go on
                final.append(not done[s] and pos[s] >= recs[s].size and not idle)
            cols = raw.call(blocks, final)
            for s in range(3):
                parts[s].append(cols[s])
                done[s] = done[s] or final[s]
        assert done == [True, True, True] and pos == [r.size for r in recs]
        for s in range(3):
            assert np.array_equal(np.hstack(parts[s]), want[s]), s
    finally:
        raw.close()


# ---- 4. 16-bit sources -------------------------------------------------------------------------------------------------
def test_integer_mode_rounds_and_clips(engine, processor):
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor, resample_host
    rate = 44100
    n = int(0.62 * rate)
    rec = np.where((np.arange(n) // 37) % 2 == 0, 32767.0, -32767.0).astype(np.float32)    # the filter overshoots
    y = resample_host(rec, rate, integer=True)
    assert y.max() == 32767.0 and y.min() == -32768.0                       # the clip is reached on both sides
    scaled = SpectrogramProcessor(engine, window_scale=1.0 / 32767)
    want = scaled.process(rec, rate, integer=True)
    assert not np.array_equal(want, scaled.process(rec, rate, integer=False))
    stream = processor.stream(sample_rate=rate, integer=True, window_scale=1.0 / 32767)
    try:
        got, _ = _stream_whole(stream, rec, [5000, 1, 0, 8000, 3, 10 * n])
        assert np.array_equal(got, want)
    finally:
        stream.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing(engine, processor):
    from audio_sheet_retrieval_amd import _lib
    rate = 44100
    recs = [_recording(rate, 0.3, 70), _recording(rate, 0.3, 71)]
    raw = _Raw(engine, processor, 2, rate)
    try:
        raw.call([r[:6000] for r in recs], [False, False])                  # a state worth keeping: one frame is out
        nxt = [r[6000:9000] for r in recs]
        wrong = [
            dict(n_new_frames=np.asarray([1, 2], np.int64)),                # stream 0 completes two frames, not one
            dict(state_offsets=np.asarray([raw.state_offsets[0], raw.state_offsets[0] + raw.cap - 1], np.int64)),
            dict(state_cap=raw.cap - 1),
            dict(blocks_floats=raw.gap + 3000 + raw.gap + 2999),            # stream 1's block ends past the buffer
            dict(up=1, down=32, half=32, taps=np.zeros((1, 65))),           # 2047 * 32 + 65 inputs per frame: 262 KB
        ]
        for w in wrong:
            with pytest.raises(_lib.AsrError) as err:
                raw.call(nxt, [False, False], **w)
            assert err.value.code == _lib.ASR_ERR_INVALID, w
        # ... and the stream goes on as if nothing had been tried
        a = raw.call(nxt, [False, False])
        b = raw.call([r[9000:] for r in recs], [True, True])
        want = processor.process_many(recs, None, [rate] * 2)
        for s in range(2):
            assert np.array_equal(np.hstack([want[s][:, :1], a[s], b[s]]), want[s])
    finally:
        raw.close()
    # no streams, and streams that get nothing: valid, nothing written
    engine.audio_stream_push_dev(0, 0, [], [], [], [], [], [], [], 1, 1, None, 0, False, 0, 0, [], 2047,
                                 processor.frame_size, processor.hop, processor.window, processor.fb_start,
                                 processor.fb_len, processor.fb_w, 0, 0)
    stream = processor.stream(n_streams=2)
    try:
        assert [c.shape for c in stream.push([np.zeros(0, np.float32)] * 2)] == [(92, 0)] * 2
    finally:
        stream.close()


# ---- 6. samples in, ranking out ------------------------------------------------------------------------------------------
def _same_track(a, b):
    assert a.m_prob.tobytes() == b.m_prob.tobytes() and not np.isnan(a.m_prob).any()
    for name in ("voiced", "frames", "pieces", "counts", "n_out", "history", "idx"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and np.array_equal(x, y), name


def test_live_tracking_equals_tracking_the_finished_spectrograms(engine, processor):
    from audio_sheet_retrieval_amd import piece_identification as pid
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        engine.set_params([z["p%02d" % i] for i in range(len(param_shapes(MODEL)))])
    rng = np.random.default_rng(8)
    n_pieces = 11
    codes = rng.standard_normal((700, 32)).astype(np.float32)
    ids = np.sort(rng.integers(0, n_pieces, size=700))
    db = pid.EmbeddingDB(engine, codes, ids, {i: "piece_%02d" % i for i in range(n_pieces)})
    try:
        rates = [44100, 22050, 44100]
        recs = [_recording(r, sec, 90 + k) for k, (r, sec) in enumerate(zip(rates, (3.0, 3.1, 2.4)))]
        specs = processor.process_many(recs, None, rates)
        want = pid.track_scores(engine, db, specs, 3, 5, 10, return_idx=True)
        assert all(len(w.frames) > 5 for w in want)                         # the gate opens: the vote is exercised
        got = pid.live_track_scores(engine, db, processor, recs, rates, [r // 10 for r in rates], None, 3, 5, 10)
        assert len(got) == 3
        for g, w in zip(got, want):
            _same_track(g, w)
    finally:
        db.close()


# ---- 7. the driver -----------------------------------------------------------------------------------------------------
sys.path.insert(0, HERE)
from test_gpu_umc import KEPT, TAG, _engine, _omr_flags, _umc_dir, exp_root  # noqa: E402,F401


def test_driver_live_dumps_the_tracking_of_every_recording(exp_root, tmp_path, capsys):  # noqa: F811
    from audio_sheet_retrieval_amd import umc_a2s_server
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor, read_audio
    from audio_sheet_retrieval_amd.audio_sheet_server import TRACK_TOP_K
    from audio_sheet_retrieval_amd.piece_identification import EmbeddingDB, live_track_scores
    from audio_sheet_retrieval_amd.sheet_utils import umc
    data_dir = _umc_dir(tmp_path)
    res = umc_a2s_server.main(["--model", "models/%s.py" % MODEL, "--data_dir", data_dir, "--train_split",
                               "splits/all_split.yaml", "--config", "exp_configs/mutopia_full_aug.yaml", "--n_candidates",
                               "5", "--init_sheet_db", "--live", "--block_ms", "100", "--resample", "--dump_results"] +
                              _omr_flags(exp_root))
    text = capsys.readouterr().out
    with open(exp_root / MODEL / ("umc_tracking_%s_umc_test_A2S.yaml" % TAG)) as fp:
        dumped = yaml.safe_load(fp)
    names = [n for n in KEPT if n != "p7_no_score_ppq"]
    assert dumped == res and sorted(dumped) == ["first_lead", "lead_share"]
    assert len(dumped["first_lead"]) == len(dumped["lead_share"]) == len(names) == text.count("of the voiced frames")
    # live_track_scores called directly on the same recordings and the saved data base
    eng = _engine()
    db = EmbeddingDB.load(eng, "umc_sheet_db_file.pkl")
    try:
        audio = [read_audio(umc.get_performance_audio_path(os.path.join(data_dir, n), "score_ppq")) for n in names]
        rates = [a[2] for a in audio]
        direct = live_track_scores(eng, db, SpectrogramProcessor(eng), [a[0] for a in audio], rates,
                                   [int(round(r * 0.1)) for r in rates], None, top_k=TRACK_TOP_K, n_candidates=5,
                                   running_frames=100, integer=[a[3] for a in audio], window_scales=[a[1] for a in audio])
        ids = {name: i for i, name in db.id_to_name.items()}
        for k, (name, r) in enumerate(zip(names, direct)):
            leads = (r.n_out > 0) & (r.pieces[:, 0] == ids[name]) if len(r.frames) else np.zeros(0, bool)
            assert dumped["first_lead"][k] == (int(r.frames[np.argmax(leads)]) if leads.any() else -1)
            assert dumped["lead_share"][k] == (float(leads.mean()) if leads.size else 0.0)
    finally:
        db.close()
        eng.close()
