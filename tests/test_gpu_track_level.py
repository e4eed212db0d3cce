"""GPU: the music gate at the level of what has been heard so far (asr_track_gate_running_dev,
asr_track_stream_gate_running_dev, csrc/track_level_kernels.hip, piece_identification.RunningLevel through track_scores,
PieceTrackerBank, live_track_scores and umc_a2s_server --live --bank --level running).  Every comparison is exact: the
whole-recording call against track_gate_host(level=RunningLevel(...)), the stream call against the whole-recording
call on the concatenated columns, the bank against track_scores and track_score_host.  NaNs (a silent prefix's 0 / 0)
are compared by position, as tests/test_gpu_track_stream.py does."""
import os
import sys

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_track_stream import (MODEL, N_CAND, RUNNING, SENTINEL, TOP_K, _bytes, _cuts, _offsets, _recording,  # noqa: E402,F401
                                   _run_bank, _same, _same_track, case, engine, trained)
from test_gpu_umc import KEPT, TAG, _omr_flags, _umc_dir, exp_root  # noqa: E402,F401
from test_track_level_host import CASES, level_signal, running_level  # noqa: E402


def _same_floats(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and _bytes(a) == _bytes(b)


def _recordings(bins, w, T):
    """the test signal, one column, fewer columns than the window, a silent prefix"""
    quiet = level_signal(bins, w + 9, seed=3)
    quiet[:, :w // 2] = 0.0
    return [level_signal(bins, T), level_signal(bins, 1, seed=1), level_signal(bins, w - 1, seed=2), quiet]


# ---- 1. whole recordings -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_floor", [False, True])
@pytest.mark.parametrize("bins,w,T,L", CASES)
def test_whole_recording_call_equals_the_host_restatement(engine, bins, w, T, L, with_floor):
    from audio_sheet_retrieval_amd.piece_identification import track_gate_host
    specs = _recordings(bins, w, T)
    floor = float(np.median(specs[0].sum(axis=0))) if with_floor else None
    rule = running_level(L, floor)
    flat = np.concatenate([s.ravel() for s in specs])
    d_src = engine.alloc(flat.nbytes).upload(flat)
    try:
        m, v, lvl = engine.track_gate_running_dev(d_src.ptr, flat.size, _offsets([s.size for s in specs]),
                                                  [s.shape for s in specs], w, rule.memory_arg, rule.floor_arg)
    finally:
        d_src.free()
    assert m.dtype == lvl.dtype == np.float32 and v.dtype == bool
    assert m.shape == v.shape == lvl.shape == (sum(s.shape[1] for s in specs),)
    at = 0
    for r, s in enumerate(specs):
        n = s.shape[1]
        rm, rv = track_gate_host(s, w, rule)
        zeros = np.zeros((bins, 1), np.float32)                      # (a second column keeps numpy adding row after row)
        rl = rule.levels(np.hstack((s, zeros)).sum(axis=0)[:n])
        assert _same_floats(m[at:at + n], rm), r
        assert np.array_equal(v[at:at + n], rv), r
        assert lvl[at:at + n].tobytes() == rl.tobytes(), r
        at += n
    assert v[:T].any() and not v[:T].all()                           # the gate opens and closes
    assert np.isnan(m[-(w + 9)]) or with_floor                       # the silent prefix: 0 / 0 (0 / floor with one)


# ---- 2. streams ----------------------------------------------------------------------------------------------------
def _whole(engine, specs, w, rule):
    flat = np.concatenate([s.ravel() for s in specs])
    d_src = engine.alloc(flat.nbytes).upload(flat)
    try:
        m, v, lvl = engine.track_gate_running_dev(d_src.ptr, flat.size, _offsets([s.size for s in specs]),
                                                  [s.shape for s in specs], w, rule.memory_arg, rule.floor_arg)
    finally:
        d_src.free()
    first = np.concatenate([[0], np.cumsum([s.shape[1] for s in specs])])
    return [(m[a:b], v[a:b], lvl[a:b]) for a, b in zip(first[:-1], first[1:])]


def _run_streams(engine, specs, w, rule, takes, restart=None):
    """pushes the streams through one call per round, `takes[round][stream]` columns each; tails and level states start
    as NaN.  restart = (round, stream, recording): from that round on the stream is a new one that brings `recording`.
    -> per stream (m_prob, voiced, level, windows), the rounds concatenated"""
    bins, t, n = specs[0].shape[0], w - 1, len(specs)
    per = rule.state_floats()
    gap = 3
    tail_off = np.arange(n, dtype=np.int64) * (bins * t)
    level_off = np.arange(n, dtype=np.int64) * (per + gap)           # unused floats between the level states
    tail_floats, level_floats = n * bins * t, n * (per + gap)
    state0 = np.full(level_floats, np.nan, np.float32)
    for s in range(n):
        state0[s * (per + gap) + per:(s + 1) * (per + gap)] = SENTINEL
    cap = max(sum(tk) for tk in takes)
    d_tail = engine.alloc(tail_floats * 4).upload(np.full(tail_floats, np.nan, np.float32))
    d_level = engine.alloc(state0.nbytes).upload(state0)
    d_cols = engine.alloc(max(4, cap * bins * 4))
    d_win = engine.alloc((cap + 1) * bins * w * 4)
    specs, done, before = list(specs), [0] * n, [0] * n
    out = [([], [], [], []) for _ in range(n)]
    try:
        for rnd, take in enumerate(takes):
            if restart is not None and restart[0] == rnd:
                specs[restart[1]], done[restart[1]], before[restart[1]] = restart[2], 0, 0
            blocks = [np.ascontiguousarray(specs[s][:, done[s]:done[s] + take[s]]) for s in range(n)]
            assert [b.shape[1] for b in blocks] == list(take)
            total = sum(take)
            if total:
                d_cols.upload(np.concatenate([b.ravel() for b in blocks]))
            d_win.upload(np.full((cap + 1) * bins * w, SENTINEL, np.float32))
            state_before = d_level.download((level_floats,), np.float32)
            m, v, nv, lvl = engine.track_stream_gate_running_dev(
                d_cols.ptr, max(1, cap * bins), _offsets([b.size for b in blocks]), take, before, rule.memory_arg,
                rule.floor_arg, bins, w, d_tail.ptr, tail_floats, tail_off, d_level.ptr, level_floats, level_off,
                d_win.ptr, total)
            assert m.shape == v.shape == lvl.shape == (total,) and nv.shape == (n,)
            win = d_win.download((cap + 1, bins, w), np.float32)
            assert (win[int(nv.sum()):] == SENTINEL).all()           # nothing past the last window
            state = d_level.download((level_floats,), np.float32)
            f0, w0 = 0, 0
            for s in range(n):
                f1, w1 = f0 + take[s], w0 + int(nv[s])
                assert int(v[f0:f1].sum()) == nv[s]
                for k, x in enumerate((m[f0:f1], v[f0:f1], lvl[f0:f1], win[w0:w1].copy())):
                    out[s][k].append(x)
                lo = s * (per + gap)
                assert (state[lo + per:lo + per + gap] == SENTINEL).all()
                if not take[s]:                                      # untouched, NaN filling included
                    assert state[lo:lo + per].tobytes() == state_before[lo:lo + per].tobytes(), (rnd, s)
                done[s] += take[s]
                before[s] += take[s]
                f0, w0 = f1, w1
    finally:
        for b in (d_tail, d_level, d_cols, d_win):
            b.free()
    return [tuple(np.concatenate(o[k]) for k in range(4)) for o in out]


def _takes(lengths, sizes_per_stream):
    """rounds of block lengths: stream s takes sizes_per_stream[s] in turn until its recording is used up"""
    cuts = [_cuts(T, sizes) for T, sizes in zip(lengths, sizes_per_stream)]
    return [[c[r] if r < len(c) else 0 for c in cuts] for r in range(max(len(c) for c in cuts))]


def _check_streams(got, want, specs, w):
    bins = specs[0].shape[0]
    for s, ((gm, gv, gl, gw), (wm, wv, wl)) in enumerate(zip(got, want)):
        assert _same_floats(gm, wm), s
        assert np.array_equal(gv, wv), s
        assert gl.tobytes() == wl.tobytes(), s
        padded = np.hstack([np.zeros((bins, w - 1), np.float32), specs[s]])
        frames = np.flatnonzero(wv)
        windows = np.stack([padded[:, i:i + w] for i in frames]) if len(frames) else np.zeros((0, bins, w), np.float32)
        assert gw.shape == windows.shape and gw.tobytes() == windows.tobytes(), s


STREAM_CASES = [(5, 8, 300, 0), (5, 8, 300, 8), (5, 8, 300, 13), (3, 9, 120, 40), (92, 42, 200, 60)]


@pytest.mark.parametrize("cut", ["columns", "pattern", "big"])
@pytest.mark.parametrize("bins,w,T,L", STREAM_CASES)
def test_stream_call_equals_the_whole_recording_call_on_the_concatenation(engine, bins, w, T, L, cut):
    rule = running_level(L, None if L == 13 else 0.25 * bins)        # both with and without a floor
    lengths = [T, T - 37, T // 2] if cut != "columns" else [3 * T // 4, T // 2, T // 3]
    specs = [level_signal(bins, n, seed=10 + k) for k, n in enumerate(lengths)]
    specs[1][:, :5] = 0.0                                            # a silent prefix
    want = _whole(engine, specs, w, rule)
    assert sum(int(wv.sum()) for _, wv, _ in want) >= 10               # windows are written
    K = L or w
    pattern = [0, 1, K - 2, K - 1, K, K + 1, 2 * K + 3]              # a 0: a round in which the stream brings nothing
    if cut == "columns":
        takes = _takes(lengths, [[1] * T] * 3)
    elif cut == "pattern":                                          # three phases of the same pattern
        takes = _takes(lengths, [(pattern[k:] + pattern[:k]) * 40 for k in (0, 2, 5)])
    else:                                                            # more than 256 new frames in one call
        takes = _takes(lengths, [[3, 270, 2], [2, 150, 1], [1, T // 2 - 1]])
        assert max(sum(tk) for tk in takes) > 256
    got = _run_streams(engine, specs, w, rule, takes)
    _check_streams(got, want, specs, w)


@pytest.mark.parametrize("L", [0, 13])
def test_a_stream_that_starts_over_equals_a_fresh_recording(engine, L):
    bins, w = 5, 8
    rule = running_level(L)
    specs = [level_signal(bins, 90, seed=20), level_signal(bins, 90, seed=21)]
    specs[0][:, :30] *= 50.0                                         # a loud start the new recording must not remember
    fresh = level_signal(bins, 60, seed=22)
    takes = [[30, 30], [30, 30], [30, 30]]
    got = _run_streams(engine, specs, w, rule, takes, restart=(1, 0, fresh))
    old, new, other = _whole(engine, [specs[0][:, :30], fresh, specs[1]], w, rule)
    loud = _whole(engine, [np.hstack((specs[0][:, :30], fresh))], w, rule)[0]
    assert not _same_floats(loud[0][30:], new[0])                    # remembering would show
    for k in range(3):
        a = np.concatenate((old[k], new[k]))
        assert (_same_floats(got[0][k], a) if k != 1 else np.array_equal(got[0][k], a)), k
        assert (_same_floats(got[1][k], other[k]) if k != 1 else np.array_equal(got[1][k], other[k])), k


# ---- 3. invalid arguments ------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing_and_touch_no_state(engine):
    from audio_sheet_retrieval_amd import _lib
    lib = engine.lib
    q = lambda x: None if x is None else x.ctypes.data
    i32, i64 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.int64))
    rng = np.random.default_rng(3)
    nan, inf = float("nan"), float("inf")
    # two streams, 5 bins, width 8, memory 9: level states of 8 floats
    cols, tail, state = (rng.random(n).astype(np.float32) for n in (25, 70, 16))
    d_cols, d_tail, d_state = (engine.alloc(x.nbytes).upload(x) for x in (cols, tail, state))
    d_win = engine.alloc(5 * 40 * 4)
    outs = [np.full(5, 7, np.float32), np.full(5, 7, np.uint8), np.full(2, 7, np.int32), np.full(5, 7, np.float32)]
    good = dict(cols_floats=25, n=2, col_off=i64(0, 15), n_new=i32(3, 2), before=i64(10, 10), memory=9, floor=-inf,
                bins=5, width=8, tail_floats=70, tail_off=i64(0, 35), level_floats=16, level_off=i64(0, 8), win_cap=5)
    bad = [dict(memory=-1), dict(memory=1), dict(memory=7), dict(memory=(1 << 20) + 1), dict(floor=nan), dict(floor=inf),
           dict(level_off=i64(0, 9)), dict(level_off=i64(-1, 8)), dict(level_off=i64(0, 7)), dict(level_floats=15),
           dict(memory=0, level_off=i64(3, 3)), dict(memory=0, level_off=i64(0, 16)),
           dict(width=7), dict(width=129), dict(bins=0), dict(n=0), dict(n_new=i32(3, -1)), dict(col_off=i64(0, 16)),
           dict(tail_off=i64(0, 34)), dict(tail_off=i64(0, 36)), dict(win_cap=4), dict(before=i64(10, -1))]
    try:
        kept = None
        for change in [{}] + bad:
            a = dict(good, **change)
            before = [o.copy() for o in outs]
            rc = lib.asr_track_stream_gate_running_dev(
                engine.ctx, d_cols.ptr, a["cols_floats"], a["n"], q(a["col_off"]), q(a["n_new"]), q(a["before"]),
                a["memory"], a["floor"], a["bins"], a["width"], d_tail.ptr, a["tail_floats"], q(a["tail_off"]), d_state.ptr,
                a["level_floats"], q(a["level_off"]), d_win.ptr, a["win_cap"], *[q(o) for o in outs])
            assert rc == (_lib.ASR_ERR_INVALID if change else _lib.ASR_OK), change
            now = (d_tail.download((70,), np.float32).tobytes(), d_state.download((16,), np.float32).tobytes())
            if change:
                assert b"asr_track_stream_gate_running_dev" in lib.asr_last_error(engine.ctx), change
                assert now == kept, change
                assert all(o.tobytes() == b.tobytes() for o, b in zip(outs, before)), change
            else:
                assert now[0] != tail.tobytes() and now[1] != state.tobytes()        # the good call moved both states
                # frames 10, 11, 12 -> slots 2, 3, 4 of the first ring; frames 10, 11 -> slots 2, 3 of the second
                got, sums = np.frombuffer(now[1], np.float32), cols[:15].reshape(5, 3).sum(axis=0)
                assert np.array_equal(np.flatnonzero(got != state), [2, 3, 4, 10, 11])
                assert np.allclose(got[2:5], sums, rtol=1e-6)
            kept = now
        # the whole-recording call
        m, v = np.empty(5, np.float32), np.empty(5, np.uint8)
        for memory, floor in [(-1, -inf), (7, -inf), ((1 << 20) + 1, -inf), (0, nan), (9, inf)]:
            rc = lib.asr_track_gate_running_dev(engine.ctx, d_cols.ptr, 25, 1, q(i64(0)), q(i32(5)), q(i32(5)), 8, memory,
                                                floor, q(m), q(v), None)
            assert rc == _lib.ASR_ERR_INVALID and b"track_gate_running" in lib.asr_last_error(engine.ctx), (memory, floor)
        assert lib.asr_track_gate_running_dev(engine.ctx, d_cols.ptr, 25, 1, q(i64(0)), q(i32(5)), q(i32(5)), 8, 9, -inf,
                                              q(m), q(v), None) == _lib.ASR_OK
    finally:
        for b in (d_cols, d_tail, d_state, d_win):
            b.free()


# ---- 4. the bank, samples in, ranking out --------------------------------------------------------------------------
@pytest.mark.parametrize("memory", [None, 60])
def test_bank_equals_track_scores_and_the_host_loop(engine, case, memory):
    from audio_sheet_retrieval_amd import piece_identification as pid
    db, specs, _ = case
    rule = pid.RunningLevel(memory=memory)
    want = pid.track_scores(engine, db, specs, TOP_K, N_CAND, RUNNING, return_idx=True, level=rule)
    fixed = pid.track_scores(engine, db, specs, TOP_K, N_CAND, RUNNING)
    assert all(w.m_prob.tobytes() != f.m_prob.tobytes() for w, f in zip(want, fixed))  # not the recording's own level
    for w, s in zip(want, specs):
        assert len(w.frames)
        _same(w, pid.track_score_host(engine, db, s, TOP_K, N_CAND, RUNNING, level=rule))
    _same(want[1], pid.track_score(engine, db, specs[1], TOP_K, N_CAND, RUNNING, return_idx=True, level=rule))
    bank = pid.PieceTrackerBank(engine, db, rule, TOP_K, N_CAND, RUNNING, n_streams=3)
    try:
        for sizes in ([5] * 80, [1, 41, 42, 43, 59, 61, 130]):
            for g, w in zip(_run_bank(engine, bank, specs, [_cuts(s.shape[1], sizes) for s in specs]), want):
                _same(g, w)
            bank.reset()
        bank.reset([1])
    finally:
        bank.close()
    with pytest.raises(ValueError, match="closed"):
        bank.push([s[:, :1] for s in specs])


def test_live_tracking_without_a_known_level_equals_the_finished_spectrograms(engine, case):
    from audio_sheet_retrieval_amd import piece_identification as pid
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    db = case[0]
    processor = SpectrogramProcessor(engine)
    rates = [44100, 22050, 44100]
    recs = [_recording(r, sec, 90 + k) for k, (r, sec) in enumerate(zip(rates, (3.0, 3.1, 2.4)))]
    rule = pid.RunningLevel()
    want = pid.track_scores(engine, db, processor.process_many(recs, None, rates), 3, 5, 10, return_idx=True, level=rule)
    assert all(len(w.frames) > 5 for w in want)
    got = pid.live_track_scores(engine, db, processor, recs, rates, [r // 10 for r in rates], rule, 3, 5, 10, batched=True)
    assert len(got) == 3
    for g, w in zip(got, want):
        _same_track(g, w)


# ---- 5. the driver -------------------------------------------------------------------------------------------------
def test_driver_live_bank_at_a_running_level_names_the_rule(exp_root, tmp_path, capsys):  # noqa: F811
    from audio_sheet_retrieval_amd import umc_a2s_server
    data_dir = _umc_dir(tmp_path)
    res = umc_a2s_server.main(["--model", "models/%s.py" % MODEL, "--data_dir", data_dir, "--train_split",
                               "splits/all_split.yaml", "--config", "exp_configs/mutopia_full_aug.yaml", "--n_candidates",
                               "5", "--init_sheet_db", "--live", "--bank", "--level", "running", "--level_memory", "1200",
                               "--block_ms", "100", "--resample", "--dump_results"] + _omr_flags(exp_root))
    text = capsys.readouterr().out
    dump = exp_root / MODEL / ("umc_tracking_%s_umc_test_A2S.yaml" % TAG)
    with open(dump) as fp:
        dumped = yaml.safe_load(fp)
    names = [n for n in KEPT if n != "p7_no_score_ppq"]
    assert dumped == res and dumped["level"] == "RunningLevel(memory=1200, floor=None)"
    assert len(dumped["first_lead"]) == len(dumped["lead_share"]) == len(names) == text.count("of the voiced frames")
    assert "Streaming every recording" in text and "RunningLevel(memory=1200, floor=None)" in text


def test_driver_running_level_needs_the_bank(capsys):
    from audio_sheet_retrieval_amd import umc_a2s_server
    with pytest.raises(SystemExit) as err:
        umc_a2s_server._arguments(["--model", "models/%s.py" % MODEL, "--data_dir", "x", "--live", "--level", "running"],
                                  "A2S")
    assert err.value.code == 2 and "--level running needs --live --bank" in capsys.readouterr().err
