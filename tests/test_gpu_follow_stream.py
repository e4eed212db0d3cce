"""GPU: score following for parallel live streams with the state on the device (asr_follow_stream_windows_dev,
asr_follow_stream_log_dev, csrc/follow_stream_kernels.hip, piece_identification.ScoreFollowerBank,
audio_sheet_server --follow --bank).  Every comparison is exact: the windows call against numpy slices of the whole
stream, the log call against a Python list, the bank against ScoreFollower / follow_scores and against the numpy
restatement follow_bank_host - the two calls only move floats, and every accumulated value of the follow call is one
fixed sequence of correctly rounded float64 operations."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")
MODEL = "mutopia_ccal_cont"
SENTINEL = np.float32(-1234.5)
GAP = 7                                                      # canary floats behind every tail


@pytest.fixture(scope="module")
def engine():
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine(MODEL)
    yield eng
    eng.close()


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)


# ---- 1. the windows call ---------------------------------------------------------------------------------------------
def _deliveries(lengths, kind, rng):
    """rounds of columns per stream: one column each, uneven blocks of 0..11, or everything at once"""
    left, rounds = np.array(lengths), []
    while left.any():
        if kind == "columns":
            take = np.minimum(1, left)
        elif kind == "uneven":
            take = np.minimum(rng.integers(0, 12, len(left)), left)
        else:
            take = left.copy()
        rounds.append(take.astype(np.int32))
        left = left - take
    return rounds


def _run_windows(engine, specs, width, step, rounds):
    """pushes the streams through one call per round; checks n_win, the tails and the canaries after every round
    -> per stream its windows concatenated"""
    from audio_sheet_retrieval_amd.piece_identification import follow_window_plan
    bins, t, n = specs[0].shape[0], width - 1, len(specs)
    tail_off = np.arange(n, dtype=np.int64) * (bins * t + GAP)
    tail_floats = n * (bins * t + GAP)
    tail0 = np.full(tail_floats, np.nan, np.float32)                 # a new stream's tail is not read
    canary = np.ones(tail_floats, bool)
    for o in tail_off:
        canary[o:o + bins * t] = False
    tail0[canary] = SENTINEL
    cap_cols = max(int(r.sum()) for r in rounds)
    cap_win = cap_cols                                               # a window per new column at the most
    d_tail = engine.alloc(tail0.nbytes).upload(tail0)
    d_cols = engine.alloc(max(4, cap_cols * bins * 4))
    d_win = engine.alloc((cap_win + 1) * bins * width * 4)
    done, out = [0] * n, [[] for _ in range(n)]
    try:
        tail_before = tail0
        for rnd, take in enumerate(rounds):
            blocks = [np.ascontiguousarray(specs[s][:, done[s]:done[s] + take[s]]) for s in range(n)]
            if take.sum():
                d_cols.upload(np.concatenate([b.ravel() for b in blocks]))
            plan = [follow_window_plan(done[s], int(take[s]), width, step)[0] for s in range(n)]
            total = sum(len(p) for p in plan)
            d_win.upload(np.full((cap_win + 1) * bins * width, SENTINEL, np.float32))
            n_win = engine.follow_stream_windows_dev(d_cols.ptr, cap_cols * bins, _offsets([b.size for b in blocks]), take,
                                                     done, bins, width, step, d_tail.ptr, tail_floats, tail_off, d_win.ptr,
                                                     total)
            assert n_win.dtype == np.int32 and n_win.tolist() == [len(p) for p in plan], (rnd, n_win)
            win = d_win.download((cap_win + 1, bins, width), np.float32)
            assert (win[total:] == SENTINEL).all(), rnd              # nothing past the last window
            tail = d_tail.download((tail_floats,), np.float32)
            assert (tail[canary] == SENTINEL).all(), rnd
            w0 = 0
            for s in range(n):
                out[s].append(win[w0:w0 + len(plan[s])].copy())
                w0 += len(plan[s])
                done[s] += int(take[s])
                lo, hi = int(tail_off[s]), int(tail_off[s]) + bins * t
                if take[s]:                                          # the last width - 1 columns so far, zeros before
                    padded = np.hstack([np.zeros((bins, t), np.float32), specs[s][:, :done[s]]])
                    assert tail[lo:hi].tobytes() == np.ascontiguousarray(padded[:, -t:]).tobytes(), (rnd, s)
                else:                                                # untouched, NaN filling included
                    assert tail[lo:hi].tobytes() == tail_before[lo:hi].tobytes(), (rnd, s)
            tail_before = tail
    finally:
        for b in (d_tail, d_cols, d_win):
            b.free()
    return [np.concatenate(o) if o else np.zeros((0, bins, width), np.float32) for o in out]


@pytest.mark.parametrize("bins", [5, 92])
@pytest.mark.parametrize("width,step", [(8, 1), (8, 11), (42, 2), (47, 3)])
def test_windows_call_cuts_the_step_grid_whatever_the_block_cut(engine, width, step, bins):
    rng = np.random.default_rng(100 * width + bins)
    lengths = [0, 1, width - 1, 3 * width + 5]
    specs = [rng.random((bins, T)).astype(np.float32) for T in lengths]
    want = []
    for spec, T in zip(specs, lengths):
        n = 0 if T < width else (T - width) // step + 1
        want.append(np.stack([spec[:, k * step:k * step + width] for k in range(n)]) if n
                    else np.zeros((0, bins, width), np.float32))
    assert [len(w) for w in want[:3]] == [0, 0, 0] and len(want[3]) >= 2
    for kind in ("columns", "uneven", "whole"):
        got = _run_windows(engine, specs, width, step, _deliveries(lengths, kind, rng))
        for s in range(4):
            assert got[s].shape == want[s].shape and got[s].tobytes() == want[s].tobytes(), (kind, s)


# ---- 2. the log call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0, 1, 4, 64])
@pytest.mark.parametrize("dim", [32, 1, 31])
def test_log_call_equals_a_list(engine, dim, keep):
    rng = np.random.default_rng(1000 * dim + keep)
    n, gap = 4, 4
    pattern = [0, 1, max(keep - 1, 0), keep, keep + 3]
    cap = 2 * keep + 3                                               # rows: max(rows_in_log, kept + new) never exceeds it
    log_off = np.arange(n, dtype=np.int64) * (cap * dim + gap)
    log_off[3] += 1                                                  # one log at an offset that is no multiple of 4
    log_floats = n * (cap * dim + gap) + 1
    log0 = rng.random(log_floats).astype(np.float32)
    canary = np.ones(log_floats, bool)
    for o in log_off:
        canary[o:o + cap * dim] = False
    log0[canary] = SENTINEL
    d_log = engine.alloc(log0.nbytes).upload(log0)
    d_codes = engine.alloc(max(4, n * (keep + 3) * dim * 4))
    model, in_log, before = [[] for _ in range(n)], np.zeros(n, np.int32), log0
    try:
        for rnd in range(2 * len(pattern)):
            count = np.array([pattern[(rnd + 2 * s) % len(pattern)] for s in range(n)], np.int32)
            rows = rng.random((int(count.sum()), dim)).astype(np.float32)
            if len(rows):
                d_codes.upload(rows)
            new_in_log = engine.follow_stream_log_dev(d_codes.ptr, len(rows), count, in_log, keep, dim, d_log.ptr,
                                                      log_floats, log_off)
            log = d_log.download((log_floats,), np.float32)
            assert (log[canary] == SENTINEL).all(), rnd
            r0 = 0
            for s in range(n):
                lo = int(log_off[s])
                if count[s]:
                    kept = min(len(model[s]), keep)
                    model[s] = model[s][len(model[s]) - kept:] + [rows[r0 + k] for k in range(count[s])]
                    r0 += int(count[s])
                    assert new_in_log[s] == len(model[s])
                    assert log[lo:lo + len(model[s]) * dim].tobytes() == np.concatenate(model[s]).tobytes(), (rnd, s)
                else:                                                # untouched: the whole region
                    assert new_in_log[s] == in_log[s]
                    assert log[lo:lo + cap * dim].tobytes() == before[lo:lo + cap * dim].tobytes(), (rnd, s)
            in_log, before = new_in_log, log
        assert keep == 0 or max(len(m) for m in model) > keep         # logs were full and slid
    finally:
        d_log.free()
        d_codes.free()


# ---- 3. invalid arguments --------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing_and_touch_no_state(engine):
    from audio_sheet_retrieval_amd import _lib
    lib = engine.lib
    q = lambda x: None if x is None else x.ctypes.data
    i32, i64 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.int64))
    rng = np.random.default_rng(3)
    # the windows call: two streams, 5 bins, width 8
    cols, tail = rng.random(25).astype(np.float32), rng.random(70).astype(np.float32)
    d_cols, d_tail, d_win = engine.alloc(cols.nbytes).upload(cols), engine.alloc(tail.nbytes).upload(tail), engine.alloc(5 * 40 * 4)
    nw = np.full(2, -5, np.int32)
    good = dict(cols_floats=25, n=2, col_off=i64(0, 15), n_new=i32(3, 2), before=i64(10, 10), bins=5, width=8, step=1,
                tail_floats=70, tail_off=i64(0, 35), win_cap=5)
    bad = [dict(width=7), dict(width=129), dict(bins=0), dict(n=0), dict(step=0), dict(n_new=i32(3, -1)),
           dict(col_off=i64(0, 16)), dict(col_off=i64(-1, 15)), dict(tail_off=i64(0, 36)), dict(tail_off=i64(-1, 35)),
           dict(tail_off=i64(0, 34)), dict(win_cap=4), dict(before=i64(10, -1))]
    try:
        state = None
        for change in [{}] + bad:
            a = dict(good, **change)
            rc = lib.asr_follow_stream_windows_dev(engine.ctx, d_cols.ptr, a["cols_floats"], a["n"], q(a["col_off"]),
                                                   q(a["n_new"]), q(a["before"]), a["bins"], a["width"], a["step"],
                                                   d_tail.ptr, a["tail_floats"], q(a["tail_off"]), d_win.ptr, a["win_cap"],
                                                   q(nw))
            assert rc == (_lib.ASR_ERR_INVALID if change else _lib.ASR_OK), change
            now = d_tail.download((70,), np.float32).tobytes()
            if change:
                assert b"asr_follow_stream_windows_dev" in lib.asr_last_error(engine.ctx), change
                assert now == state, change
            else:
                assert now != tail.tobytes() and nw.tolist() == [3, 2]       # the good call slid both tails
            state = now
        with pytest.raises(_lib.AsrError, match="asr_follow_stream_windows_dev"):
            engine.follow_stream_windows_dev(d_cols.ptr, 25, [0, 15], [3, 2], [10, 10], 5, 8, 0, d_tail.ptr, 70, [0, 35],
                                             d_win.ptr, 5)
    finally:
        for b in (d_cols, d_tail, d_win):
            b.free()
    # the log call: two streams, dim 2, keep 2, logs of 5 rows
    codes, log = rng.random(8).astype(np.float32), rng.random(20).astype(np.float32)
    d_codes, d_log = engine.alloc(codes.nbytes).upload(codes), engine.alloc(log.nbytes).upload(log)
    good = dict(n_rows=4, n=2, count=i32(3, 1), in_log=i32(4, 0), keep=2, dim=2, log_floats=20, log_off=i64(0, 10))
    bad = [dict(n=0), dict(dim=0), dict(dim=65), dict(keep=-1), dict(n_rows=3), dict(n_rows=5), dict(count=i32(5, -1)),
           dict(in_log=i32(4, -1)), dict(log_off=i64(0, 9)), dict(log_off=i64(-1, 10)), dict(log_off=i64(0, 19)),
           dict(log_floats=9), dict(in_log=i32(6, 0)), dict(count=i32(4, 0))]
    try:
        state = None
        for change in [{}] + bad:
            a = dict(good, **change)
            rc = lib.asr_follow_stream_log_dev(engine.ctx, d_codes.ptr, a["n_rows"], a["n"], q(a["count"]), q(a["in_log"]),
                                               a["keep"], a["dim"], d_log.ptr, a["log_floats"], q(a["log_off"]))
            assert rc == (_lib.ASR_ERR_INVALID if change else _lib.ASR_OK), change
            now = d_log.download((20,), np.float32)
            if change:
                assert b"asr_follow_stream_log_dev" in lib.asr_last_error(engine.ctx), change
                assert now.tobytes() == state.tobytes(), change
            else:                                                     # [rows 2, 3 | three new rows] and [one new row]
                assert now[:10].tobytes() == np.concatenate([log[4:8], codes[:6]]).tobytes()
                assert now[10:12].tobytes() == codes[6:8].tobytes() and now[12:].tobytes() == log[12:].tobytes()
            state = now
    finally:
        d_codes.free()
        d_log.free()


# ---- 4. the bank -----------------------------------------------------------------------------------------------------
KEYS = ("cost", "row", "start_row", "x", "start_x")
CANDS = [[1, 0, 3], ["synthetic_001"], [2, 3], [3, 0, 1, 2]]


@pytest.fixture(scope="module")
def synthetic(engine):
    """4 synthetic pieces on trained parameters: the recordings, the data base, its strip coordinates, follow_scores'
    results for CANDS and the codes of follow_scores' windows, computed once"""
    from audio_sheet_retrieval_amd import audio2sheet_align, audio_sheet_server as drv, piece_identification as pid
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(PARAMS) as z:
        engine.set_params([z["p%02d" % i] for i in range(len(param_shapes(MODEL)))])
    data = audio2sheet_align.select_pieces("synthetic:4", 23)
    pool = AudioScoreRetrievalPool(engine, data["images"], data["specs"], data["o2c_maps"],
                                   data_augmentation=dict(NO_AUGMENT), shuffle=False)
    db = pid.EmbeddingDB.from_pool(engine, pool, 1, names=data["names"])
    specs = [np.ascontiguousarray(s[0], dtype=np.float32) for s in pool.specs]
    cols = drv.pool_sheet_columns(pool, len(db))
    whole = pid.follow_scores(engine, db, specs, CANDS, step_spec=2, sheet_columns=cols)
    codes = []
    for spec in specs:
        st = pid.follow_window_plan(0, spec.shape[1], 42, 2)[0]
        d_src = engine.alloc(spec.nbytes).upload(spec)
        d_win, d_codes = engine.alloc(len(st) * 92 * 42 * 4), engine.alloc(len(st) * 32 * 4)
        try:
            pid.embed_windows_dev(engine, 2, d_src.ptr, spec.size, pid._identity_desc(0, 92, spec.shape[1], 0, st), (92, 42),
                                  d_win, d_codes, len(st))
            codes.append(d_codes.download((len(st), 32), np.float32))
        finally:
            for b in (d_src, d_win, d_codes):
                b.free()
    yield dict(specs=specs, db=db, cols=cols, whole=whole, codes=codes, names=data["names"])
    db.close()


def _cuts(T, kind, rng):
    if kind == "even":
        return list(range(0, T, 20)) + [T]
    cuts = [0]
    while cuts[-1] < T:
        cuts.append(min(T, cuts[-1] + int(rng.integers(1, 12))))
    return cuts


def _push_rounds(engine, bank, specs, cuts, device, before_round=None):
    """the streams through `bank`, stream s cut at cuts[s] (empty blocks once it is over) -> per stream its results"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    parts = [[] for _ in specs]
    for rnd in range(max(len(c) for c in cuts) - 1):
        if before_round is not None:
            before_round(rnd)
        blocks = [np.ascontiguousarray(x[:, c[rnd]:c[rnd + 1]] if rnd + 1 < len(c) else x[:, :0]) for x, c in zip(specs, cuts)]
        if device:
            buf = engine.alloc(max(4, sum(b.nbytes for b in blocks)))
            try:
                if sum(b.size for b in blocks):
                    buf.upload(np.concatenate([b.ravel() for b in blocks]))
                res = bank.push(pid.DeviceArrays(buf, _offsets([b.size for b in blocks]), [b.shape for b in blocks]))
            finally:
                buf.free()
        else:
            res = bank.push(blocks)
        for s, r in enumerate(res):
            parts[s].append(r)
    return parts


@pytest.mark.parametrize("kind,device", [("even", False), ("uneven", False), ("even", True)])
def test_bank_with_fixed_candidates_equals_score_follower_and_follow_scores(engine, synthetic, kind, device):
    from audio_sheet_retrieval_amd import piece_identification as pid
    specs, db, cols, whole = synthetic["specs"], synthetic["db"], synthetic["cols"], synthetic["whole"]
    rng = np.random.default_rng(5)
    cuts = [_cuts(x.shape[1], kind, rng) for x in specs]
    bank = pid.ScoreFollowerBank(engine, db, 4, n_slots=5, step_spec=2, sheet_columns=cols)
    bank.stages = {}
    try:
        for s, cands in enumerate(CANDS):
            bank.set_candidates(s, cands)
        assert bank.slots(3) == [3, 0, 1, 2, None]
        parts = _push_rounds(engine, bank, specs, cuts, device)
        state = bank.state()
    finally:
        bank.close()
    assert sorted(bank.stages) == ["embed", "follow", "log", "windows"]
    for s, (cands, want) in enumerate(zip(CANDS, whole)):
        C = len(cands)
        got = pid._concat_bank_results(parts[s], 5, db.id_to_name)
        assert got.frames.dtype == want.frames.dtype and np.array_equal(got.frames, want.frames), s
        assert got.piece[:, :C].tolist() == [want.pieces] * len(want.frames) and (got.piece[:, C:] == -1).all(), s
        assert (got.since[:, :C] == 0).all() and (got.since[:, C:] == -1).all() and np.isinf(got.cost[:, C:]).all(), s
        for key in KEYS:
            g, w = getattr(got, key)[:, :C], getattr(want, key)
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (s, key)
        assert got.best.dtype == want.best.dtype and np.array_equal(got.best, want.best), s
        assert state[s][C:] == [None] * (5 - C) and all(st[3][2] == len(want.frames) for st in state[s][:C])
    if kind == "even" and not device:                        # ... and one ScoreFollower per stream over the same blocks
        for s in (0, 3):
            session = pid.ScoreFollower(engine, db, CANDS[s], step_spec=2, sheet_columns=cols)
            try:
                for rnd, (a, b) in enumerate(zip(cuts[s][:-1], cuts[s][1:])):
                    want, got = session.push(specs[s][:, a:b]), parts[s][rnd]
                    assert np.array_equal(got.frames, want.frames) and np.array_equal(got.best, want.best), (s, rnd)
                    for key in KEYS:
                        assert np.array_equal(getattr(got, key)[:, :len(CANDS[s])], getattr(want, key)), (s, rnd, key)
            finally:
                session.close()


@pytest.mark.parametrize("catch_up", [0, 3, 64])
def test_bank_with_a_scripted_schedule_equals_the_host(engine, synthetic, catch_up):
    from audio_sheet_retrieval_amd import piece_identification as pid
    db, cols = synthetic["db"], synthetic["cols"]
    specs = list(synthetic["specs"][:3]) + [np.ascontiguousarray(synthetic["specs"][3][:, :100])]     # stream 3 ends early
    codes = list(synthetic["codes"][:3]) + [synthetic["codes"][3][:(100 - 42) // 2 + 1]]
    # stream 0: fixed; stream 1: empty, then [2], [2, 3, 0], [0, 1] - 0 keeps its state and its since; stream 2: never;
    # stream 3: gets its candidate when it brings no windows any more
    schedule = {0: {0: [1, 0, 3]}, 3: {1: [2]}, 6: {1: [2, 3, 0]}, 8: {3: [1]}, 9: {1: [0, 1]}}
    cuts = [list(range(0, x.shape[1], 20)) + [x.shape[1]] for x in specs]
    n_rounds = max(len(c) for c in cuts) - 1
    counts = [[len(pid.follow_window_plan(c[r], c[r + 1] - c[r], 42, 2)[0]) if r + 1 < len(c) else 0 for c in cuts]
              for r in range(n_rounds)]
    assert sum(counts[r][3] for r in range(8, n_rounds)) == 0         # stream 3 is over when its candidate comes
    assert sum(counts[r][1] for r in range(3)) == 10                  # stream 1's history at its first entry: 3 < 10 < 64
    segs = pid.piece_segments(db.ids)
    want, want_state = pid.follow_bank_host(codes, counts, schedule, db.codes, segs, n_slots=5, catch_up=catch_up,
                                            sheet_columns=cols, step_spec=2)
    bank = pid.ScoreFollowerBank(engine, db, 4, n_slots=5, step_spec=2, catch_up=catch_up, sheet_columns=cols)

    def wishes(rnd):
        for s, pieces in schedule.get(rnd, {}).items():
            bank.set_candidates(s, pieces)
    try:
        parts = _push_rounds(engine, bank, specs, cuts, False, before_round=wishes)
        state = bank.state()
    finally:
        bank.close()
    for s in range(4):
        got = pid._concat_bank_results(parts[s], 5, db.id_to_name)
        for key in ("frames", "piece", "since", "best") + KEYS:
            g, w = getattr(got, key), getattr(want[s], key)
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (s, key)
        for k in range(5):
            if want_state[s][k] is None or want_state[s][k][2]:
                assert state[s][k] == want_state[s][k], (s, k)       # empty, or pending for good
            else:                                                    # the host's last accumulated row
                (p, since, pending, (acc, org, rows)), (wp, wsince, _, (wacc, worg, wrows)) = state[s][k], want_state[s][k]
                assert (p, since, pending, rows) == (wp, wsince, False, wrows), (s, k)
                assert np.array_equal(acc, wacc) and np.array_equal(org, worg), (s, k)
    got1 = pid._concat_bank_results(parts[1], 5, db.id_to_name)
    assert got1.piece[-1].tolist() == [1, -1, 0, -1, -1]
    entered = np.flatnonzero(got1.piece[:, 2] == 0)                   # piece 0 entered at round 6 and kept its since
    assert len(set(got1.since[entered, 2].tolist())) == 1 and (got1.piece[entered[0]:, 2] == 0).all()
    assert (pid._concat_bank_results(parts[2], 5, None).best == -1).all()
    assert state[3] == [(1, -1, True, None)] + [None] * 4


def test_a_push_larger_than_the_round_limit(engine, synthetic):
    """step_spec = 1 over 1331 columns: 1290 windows; catch_up = 64 leaves rounds of 960 columns, so one push of the
    whole is cut in two; pushes of 600 columns give the same"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    db = synthetic["db"]
    spec = np.ascontiguousarray(np.hstack([synthetic["specs"][1], synthetic["specs"][2]]))
    assert spec.shape[1] - 42 + 1 == 1290
    results = []
    for cuts in ([0, spec.shape[1]], [0, 600, 1200, spec.shape[1]]):
        bank = pid.ScoreFollowerBank(engine, db, 1, n_slots=2, step_spec=1)
        try:
            assert bank.round_rows == 960
            bank.set_candidates(0, [2, 1])
            results.append(pid._concat_bank_results(_push_rounds(engine, bank, [spec], [cuts], False)[0], 2, None))
        finally:
            bank.close()
    assert results[0].cost.shape == (1290, 2) and np.array_equal(results[0].frames, np.arange(1290))
    for key in ("frames", "piece", "since", "best") + KEYS:
        assert np.array_equal(getattr(results[0], key), getattr(results[1], key)), key
    assert (results[0].since == 0).all() and np.isfinite(results[0].cost).all()


# ---- 5. the driver ---------------------------------------------------------------------------------------------------
def test_driver_follow_bank_dumps_one_entry_per_piece(tmp_path):
    """audio_sheet_server --follow --bank in a child process on four synthetic pieces; without --bank the same command
    gives the report it gave before"""
    import pickle
    import yaml
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(PARAMS) as z:
        trained = [z["p%02d" % i] for i in range(len(param_shapes(MODEL)))]
    d = tmp_path / MODEL
    d.mkdir()
    with open(d / "params_all_split_mutopia_full_aug.pkl", "wb") as fp:
        pickle.dump(trained, fp, protocol=2)
    env = dict(os.environ, ASR_EXP_ROOT=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "audio_sheet_retrieval_amd.audio_sheet_server", "--model", "models/mutopia_ccal_cont.py",
           "--data", "synthetic:4", "--train_split", "splits/all_split.yaml", "--config", "exp_configs/mutopia_full_aug.yaml",
           "--init_sheet_db", "--follow", "--dump_results", "--block_frames", "50", "--locate_pieces", "3"]
    lengths = [464, 644, 687, 490]
    for bank in (True, False):
        out = subprocess.run(cmd + (["--bank"] if bank else []), capture_output=True, text=True, env=env, cwd=str(tmp_path),
                             timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        with open(d / "following_all_split_mutopia_full_aug_A2S.yaml") as fp:
            dumped = yaml.safe_load(fp)
        assert [e["name"] for e in dumped] == ["synthetic_%03d" % i for i in range(4)]
        fields = ["best_share", "candidate", "median_error", "name", "windows"] + (["occupied_share"] if bank else [])
        for e, T in zip(dumped, lengths):
            assert sorted(e) == sorted(fields)
            assert e["windows"] == (T - 42) // 2 + 1 and 0.0 <= e["best_share"] <= 1.0
            assert e["candidate"] == (e["median_error"] is not None)
            if bank:
                assert 0.0 < e["occupied_share"] <= 1.0 and e["candidate"]
        lines = out.stdout.splitlines()
        assert all(sum(ln.startswith("own piece") and ln.endswith(e["name"]) for ln in lines) == 1 for e in dumped)
        assert "following of 4 pieces written to" in out.stdout
