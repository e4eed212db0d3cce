"""GPU: the running vote for parallel live streams with the state on the device (asr_track_stream_gate_dev,
asr_track_stream_vote_dev, csrc/track_stream_kernels.hip, piece_identification.PieceTrackerBank,
live_track_scores(batched=True), umc_a2s_server --live --bank).  Every comparison is exact: the gate call against
track_gate_host and the columns themselves, the vote call against track_vote_host and asr_track_vote_batch_dev, the
bank against PieceTracker and track_score_host.  NaNs (a silent stream's 0 / 0) are compared by position, as
tests/test_gpu_track.py does."""
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
GARBAGE = np.int32(0)                # what an unwritten ring slot holds: a valid index, so a vote that read it would show


@pytest.fixture(scope="module")
def engine():
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine(MODEL)
    yield eng
    eng.close()


def _bytes(m_prob):
    """float32 bytes with every NaN replaced by one NaN"""
    m = np.array(m_prob, np.float32)
    m[np.isnan(m)] = np.float32(np.nan)
    return m.tobytes()


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)


# ---- 1. the gate call ----------------------------------------------------------------------------------------------
def _gate_streams(width, bins):
    rng = np.random.default_rng(100 * width + bins)
    ramp = np.abs(np.linspace(-1.0, 1.0, 300, dtype=np.float32)) ** 3                  # loud - silent - loud
    specs = [(3.0 * rng.random((bins, 300)) ** 2).astype(np.float32),
             (3.0 * rng.random((bins, 300)) ** 2).astype(np.float32) * ramp,
             np.zeros((bins, 300), np.float32),                                        # level 0: 0 / 0 at every frame
             np.zeros((bins, 300), np.float32),                                        # level 1: m_prob 0
             (3.0 * rng.random((bins, 43)) ** 2).astype(np.float32)]
    levels = [specs[0].sum(axis=0).max(), specs[1].sum(axis=0).max(), 0.0, 1.0, specs[4].sum(axis=0).max()]
    return specs, np.asarray(levels, np.float32)


def _run_gate(engine, specs, levels, width, order):
    """pushes the streams `order` (indices into specs) through one call per round, checks tails, sentinels and counts
    after every round -> {stream: (m_prob, voiced, windows)} with everything concatenated"""
    bins, t = specs[0].shape[0], width - 1
    pattern = [0, 1, width - 2, width - 1, width, 3 * width + 5]
    n, gap = len(order), 7
    tail_off = np.arange(n, dtype=np.int64) * (bins * t)
    tail_off[n // 2:] += gap                                         # an unused gap between two tails
    tail_floats = n * bins * t + gap
    tail0 = np.full(tail_floats, np.nan, np.float32)                 # a new stream's tail is not read
    gap_at = int(tail_off[n // 2]) - gap
    tail0[gap_at:gap_at + gap] = SENTINEL
    cap = sum(min(max(pattern), s.shape[1]) for s in specs)
    d_tail = engine.alloc(tail0.nbytes).upload(tail0)
    d_cols = engine.alloc(cap * bins * 4)
    d_win = engine.alloc((cap + 1) * bins * width * 4)
    done = [0] * n
    out = {s: ([], [], []) for s in order}
    try:
        tail_before, rnd = tail0, 0
        while any(done[k] < specs[s].shape[1] for k, s in enumerate(order)):
            take = [min(pattern[(rnd + s) % len(pattern)], specs[s].shape[1] - done[k]) for k, s in enumerate(order)]
            blocks = [np.ascontiguousarray(specs[s][:, done[k]:done[k] + take[k]]) for k, s in enumerate(order)]
            total = sum(take)
            if total:
                d_cols.upload(np.concatenate([b.ravel() for b in blocks]))
            d_win.upload(np.full((cap + 1) * bins * width, SENTINEL, np.float32))
            m, v, nv = engine.track_stream_gate_dev(d_cols.ptr, cap * bins, _offsets([b.size for b in blocks]), take, done,
                                                    levels[order], bins, width, d_tail.ptr, tail_floats, tail_off,
                                                    d_win.ptr, total)
            assert m.dtype == np.float32 and v.dtype == bool and nv.dtype == np.int32
            assert m.shape == v.shape == (total,) and nv.shape == (n,)
            win = d_win.download(((cap + 1), bins, width), np.float32)
            assert (win[int(nv.sum()):] == SENTINEL).all()           # nothing past the last window
            tail = d_tail.download((tail_floats,), np.float32)
            assert (tail[gap_at:gap_at + gap] == SENTINEL).all()
            f0, w0 = 0, 0
            for k, s in enumerate(order):
                f1, w1 = f0 + take[k], w0 + int(nv[k])
                assert int(v[f0:f1].sum()) == nv[k]
                out[s][0].append(m[f0:f1]), out[s][1].append(v[f0:f1]), out[s][2].append(win[w0:w1].copy())
                done[k] += take[k]
                lo, hi = int(tail_off[k]), int(tail_off[k]) + bins * t
                if take[k]:                                          # the last width - 1 columns so far, zeros before
                    padded = np.hstack([np.zeros((bins, t), np.float32), specs[s][:, :done[k]]])
                    assert tail[lo:hi].tobytes() == np.ascontiguousarray(padded[:, -t:]).tobytes(), (rnd, s)
                else:                                                # untouched, NaN filling included
                    assert tail[lo:hi].tobytes() == tail_before[lo:hi].tobytes(), (rnd, s)
                f0, w0 = f1, w1
            tail_before, rnd = tail, rnd + 1
    finally:
        for b in (d_tail, d_cols, d_win):
            b.free()
    return {s: (np.concatenate(o[0]), np.concatenate(o[1]), np.concatenate(o[2])) for s, o in out.items()}


@pytest.mark.parametrize("bins", [5, 92])
@pytest.mark.parametrize("width", [8, 42, 47])
def test_gate_call_equals_the_host_gate_and_cuts_the_windows(engine, width, bins):
    from audio_sheet_retrieval_amd.piece_identification import track_gate_host
    specs, levels = _gate_streams(width, bins)
    refs = [track_gate_host(s, width, lv) for s, lv in zip(specs, levels)]
    d = np.diff(refs[1][1].astype(int))
    assert (d == 1).any() and (d == -1).any()                        # the gate opens and closes
    assert np.isnan(refs[2][0]).all() and not refs[2][1].any()
    assert (refs[3][0] == 0).all() and not refs[3][1].any()
    got = _run_gate(engine, specs, levels, width, [0, 1, 2, 3, 4])
    for s, (rm, rv) in enumerate(refs):
        gm, gv, gw = got[s]
        assert np.array_equal(np.isnan(gm), np.isnan(rm)) and _bytes(gm) == _bytes(rm), s
        assert np.array_equal(gv, rv), s
        padded = np.hstack([np.zeros((bins, width - 1), np.float32), specs[s]])
        frames = np.flatnonzero(rv)
        want = np.stack([padded[:, i:i + width] for i in frames]) if len(frames) else np.zeros((0, bins, width), np.float32)
        assert gw.shape == want.shape and gw.tobytes() == want.tobytes(), s
    # the composition of the call changes no byte: the streams in reversed order, and one stream alone
    for order in ([4, 3, 2, 1, 0], [1]):
        other = _run_gate(engine, specs, levels, width, order)
        for s in order:
            for a, b in zip(other[s], got[s]):
                assert _bytes(a) == _bytes(b) if a.dtype == np.float32 and a.ndim == 1 else a.tobytes() == b.tobytes(), s


# ---- 2. the vote call ----------------------------------------------------------------------------------------------
def _vote_ref(idx, ids, first, count, top_k, running_frames):
    from audio_sheet_retrieval_amd.piece_identification import track_vote_host
    P, K, N = [], [], []
    for r in range(len(first)):
        rows = idx[first[r]:first[r] + count[r]]
        p, c, n, _ = track_vote_host(ids[rows].reshape(len(rows), idx.shape[1]), top_k, running_frames)
        P.append(p), K.append(c), N.append(n)
    return np.concatenate(P), np.concatenate(K), np.concatenate(N)


def _vote_rounds(engine, idx, first, count, deliveries, n_candidates, running_frames, d_ids, n_db, n_pieces, top_k):
    """delivers the rows of the streams in the rounds `deliveries` (rows per stream and round) to a ring that starts
    as garbage -> (pieces, counts, n_out) in table order, the downloaded ring (streams x keep x n_candidates)"""
    n, keep = len(count), running_frames - 1
    slice_len = keep * n_candidates
    hist_off = np.arange(n, dtype=np.int64) * slice_len
    d_hist = engine.alloc(max(4, n * slice_len * 4)).upload(np.full(max(1, n * slice_len), GARBAGE, np.int32))
    d_new = engine.alloc(max(4, idx.nbytes))
    outs = [[[], [], []] for _ in range(n)]
    done = np.zeros(n, np.int64)
    try:
        for take in deliveries:
            rows = np.concatenate([idx[first[s] + done[s]:first[s] + done[s] + take[s]] for s in range(n)])
            if len(rows):
                d_new.upload(rows)
            got = engine.track_stream_vote_dev(d_new.ptr, len(rows), take, done, n_candidates, running_frames, d_ids.ptr,
                                               n_db, n_pieces, top_k, d_hist.ptr if keep else None, n * slice_len,
                                               hist_off if keep else None)
            assert got[0].shape == got[1].shape == (len(rows), top_k) and got[2].shape == (len(rows),)
            at = 0
            for s in range(n):
                for k in range(3):
                    outs[s][k].append(got[k][at:at + take[s]])
                at += take[s]
                done[s] += take[s]
        assert np.array_equal(done, count)
        ring = d_hist.download((n, keep, n_candidates), np.int32) if keep else None
    finally:
        d_hist.free()
        d_new.free()
    return tuple(np.concatenate([np.concatenate(outs[s][k]) for s in range(n)]) for k in range(3)), ring


def _deliveries(count):
    """rounds of 1 + (s + round) % 4 rows per stream, zeros once a stream is exhausted"""
    left, rnd, res = np.array(count), 0, []
    while left.any():
        take = np.minimum([1 + (s + rnd) % 4 for s in range(len(count))], left)
        res.append(take.astype(np.int32))
        left = left - take
        rnd += 1
    return res


@pytest.mark.parametrize("n_pieces,lds_cap", [(1, None), (2, None), (300, None), (300, "1")])
def test_vote_call_equals_numpy_and_the_batch_call(engine, monkeypatch, n_pieces, lds_cap):
    monkeypatch.setenv("ASR_TRACK_SEG_FRAMES", "4")                 # 13 rows in one round span four segments
    if lds_cap:
        monkeypatch.setenv("ASR_TRACK_LDS_PIECES", lds_cap)         # the workspace path
    rng = np.random.default_rng(n_pieces)
    n_db = 900
    ids = rng.integers(0, n_pieces, size=n_db).astype(np.int32)
    d_ids = engine.alloc(ids.nbytes).upload(ids)
    voted = rng.choice(n_pieces, size=min(3, n_pieces), replace=False)           # ties are the rule
    pool = np.flatnonzero(np.isin(ids, voted))
    try:
        for running_frames in (1, 2, 3, 7):
            keep = running_frames - 1
            count = np.array([0, 1, running_frames - 1, running_frames, running_frames + 1, 13], np.int64)
            first = _offsets(count)
            for n_candidates in (1, 3, 25):
                idx = rng.choice(pool, size=(int(count.sum()), n_candidates)).astype(np.int32)
                d_idx = engine.alloc(idx.nbytes).upload(idx)
                args = (n_candidates, running_frames, d_ids, n_db, n_pieces)
                try:
                    for top_k in (1, 3, 64):
                        tag = (running_frames, n_candidates, top_k)
                        want = _vote_ref(idx, ids, first, count, top_k, running_frames)
                        batch = engine.track_vote_batch_dev(d_idx.ptr, len(idx), first, count, n_candidates, running_frames,
                                                            d_ids.ptr, n_db, n_pieces, top_k)
                        for deliveries in (_deliveries(count), [count.astype(np.int32)]):      # in rounds; in one round
                            got, ring = _vote_rounds(engine, idx, first, count, deliveries, *args, top_k)
                            for g, w, b in zip(got, want, batch):
                                assert g.dtype == np.int32 and np.array_equal(g, w) and np.array_equal(g, b), tag
                            # the ring holds the last running_frames - 1 rows in their slots, garbage where none came
                            for s in range(len(count) if keep else 0):
                                slots = np.full((keep, n_candidates), GARBAGE, np.int32)
                                for v in range(max(0, int(count[s]) - keep), int(count[s])):
                                    slots[v % keep] = idx[first[s] + v]
                                assert np.array_equal(ring[s], slots), (tag, s)
                finally:
                    d_idx.free()
    finally:
        d_ids.free()


def test_vote_call_ignores_invalid_entries(engine, monkeypatch):
    monkeypatch.setenv("ASR_TRACK_SEG_FRAMES", "4")
    ids = np.array([0, 1, 1, 7, -2, 2], np.int32)                   # piece ids 7 and -2 lie outside [0, 3)
    idx = np.array([[0, 3], [4, 1], [2, -1], [6, 5], [5, 5], [1, 0]], np.int32)   # -1 and 6 outside [0, 6)
    d_ids = engine.alloc(ids.nbytes).upload(ids)
    try:
        (p, c, n), _ = _vote_rounds(engine, idx, [0], np.array([6]), [np.array([3], np.int32)] * 2, 2, 2, d_ids, 6, 3, 2)
        assert p.tolist() == [[0, -1], [1, 0], [1, -1], [2, 1], [2, -1], [2, 1]]
        assert c.tolist() == [[1, 0], [1, 1], [2, 0], [1, 1], [3, 0], [2, 1]] and n.tolist() == [1, 2, 1, 2, 1, 2]
    finally:
        d_ids.free()


# ---- 3. invalid arguments ------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing_and_touch_no_state(engine):
    from audio_sheet_retrieval_amd import _lib
    lib = engine.lib
    q = lambda x: None if x is None else x.ctypes.data
    i32, i64 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.int64))
    rng = np.random.default_rng(3)
    # the gate call: two streams, 5 bins, width 8
    cols, tail = rng.random(25).astype(np.float32), rng.random(70).astype(np.float32)
    d_cols, d_tail, d_win = engine.alloc(cols.nbytes).upload(cols), engine.alloc(tail.nbytes).upload(tail), engine.alloc(5 * 40 * 4)
    m, v, nv = np.empty(5, np.float32), np.empty(5, np.uint8), np.empty(2, np.int32)
    good = dict(cols_floats=25, n=2, col_off=i64(0, 15), n_new=i32(3, 2), before=i64(10, 10), level=np.ones(2, np.float32),
                bins=5, width=8, tail_floats=70, tail_off=i64(0, 35), win_cap=5)
    bad = [dict(width=7), dict(width=129), dict(bins=0), dict(n=0), dict(n_new=i32(3, -1)), dict(col_off=i64(0, 16)),
           dict(col_off=i64(-1, 15)), dict(tail_off=i64(0, 36)), dict(tail_off=i64(-1, 35)), dict(tail_off=i64(0, 34)),
           dict(win_cap=4), dict(before=i64(10, -1))]
    try:
        state = None
        for change in [{}] + bad:
            a = dict(good, **change)
            rc = lib.asr_track_stream_gate_dev(engine.ctx, d_cols.ptr, a["cols_floats"], a["n"], q(a["col_off"]), q(a["n_new"]),
                                               q(a["before"]), q(a["level"]), a["bins"], a["width"], d_tail.ptr,
                                               a["tail_floats"], q(a["tail_off"]), d_win.ptr, a["win_cap"], q(m), q(v), q(nv))
            assert rc == (_lib.ASR_ERR_INVALID if change else _lib.ASR_OK), change
            now = d_tail.download((70,), np.float32).tobytes()
            if change:
                assert b"asr_track_stream_gate_dev" in lib.asr_last_error(engine.ctx), change
                assert now == state, change
            else:
                assert now != tail.tobytes()                          # the good call slid both tails
            state = now
    finally:
        for b in (d_cols, d_tail, d_win):
            b.free()
    # the vote call: two streams, rings of 2 x 2
    ids, idx = np.zeros(8, np.int32), np.arange(8, dtype=np.int32).reshape(4, 2)
    hist = np.full(8, 5, np.int32)
    d_ids, d_idx, d_hist = (engine.alloc(x.nbytes).upload(x) for x in (ids, idx, hist))
    out = np.empty(4 * 64, np.int32)
    p = out.ctypes.data
    good = dict(n_rows=4, n=2, count=i32(3, 1), before=i64(5, 0), n_cand=2, rf=3, n_db=8, n_pieces=3, top_k=2, hist_len=8,
                hist_off=i64(0, 4))
    bad = [dict(top_k=0), dict(top_k=65), dict(n_cand=0), dict(rf=0), dict(n_pieces=0), dict(n=0), dict(n_rows=3),
           dict(n_rows=5), dict(count=i32(5, -1)), dict(hist_off=i64(0, 5)), dict(hist_off=i64(-1, 4)), dict(hist_off=i64(0, 3)),
           dict(hist_len=7), dict(before=i64(5, -1)), dict(n_db=1)]
    try:
        state = None
        for change in [{}] + bad:
            a = dict(good, **change)
            rc = lib.asr_track_stream_vote_dev(engine.ctx, d_idx.ptr, a["n_rows"], a["n"], q(a["count"]), q(a["before"]),
                                               a["n_cand"], a["rf"], d_ids.ptr, a["n_db"], a["n_pieces"], a["top_k"],
                                               d_hist.ptr, a["hist_len"], q(a["hist_off"]), p, p, p)
            assert rc == (_lib.ASR_ERR_INVALID if change else _lib.ASR_OK), change
            now = d_hist.download((8,), np.int32)
            if change:
                assert b"asr_track_stream_vote_dev" in lib.asr_last_error(engine.ctx), change
                assert np.array_equal(now, state), change
            else:                                                     # frames 6, 7 -> slots 0, 1 (5 is not kept); frame 0 -> slot 0
                assert now.tolist() == [2, 3, 4, 5, 6, 7, 5, 5]
            state = now
        with pytest.raises(_lib.AsrError, match="asr_track_stream_vote_dev"):
            engine.track_stream_vote_dev(d_idx.ptr, 4, [3, 1], [5, 0], 2, 3, d_ids.ptr, 8, 3, 65, d_hist.ptr, 8, [0, 4])
    finally:
        for b in (d_ids, d_idx, d_hist):
            b.free()


# ---- 4. the bank ---------------------------------------------------------------------------------------------------
TOP_K, N_CAND, RUNNING = 5, 5, 20


@pytest.fixture(scope="module")
def trained():
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        return [z["p%02d" % i] for i in range(len(param_shapes(MODEL)))]


@pytest.fixture(scope="module")
def case(engine, trained):
    """the data base, the recordings and track_score_host's results of tests/test_gpu_track.py, computed once"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    engine.set_params(trained)
    rng = np.random.default_rng(8)
    n_pieces = 11
    codes = rng.standard_normal((700, 32)).astype(np.float32)
    ids = np.sort(rng.integers(0, n_pieces, size=700))
    db = pid.EmbeddingDB(engine, codes, ids, {i: "piece_%02d" % i for i in range(n_pieces)})
    specs = [(3.0 * rng.random((92, T)) ** 2).astype(np.float32) for T in (43, 60, 400)]
    specs[1][:, 45:55] = 0.0
    specs[2][:, 150:250] = 0.0                                       # a silent stretch in the middle
    host = [pid.track_score_host(engine, db, s, TOP_K, N_CAND, RUNNING) for s in specs]
    yield db, specs, host
    db.close()


def _same(a, b):
    assert np.array_equal(np.isnan(a.m_prob), np.isnan(b.m_prob)) and _bytes(a.m_prob) == _bytes(b.m_prob)
    assert a.m_prob.dtype == b.m_prob.dtype == np.float32
    assert a.voiced.dtype == b.voiced.dtype == bool and np.array_equal(a.voiced, b.voiced)
    for name in ("frames", "pieces", "counts", "n_out", "history", "idx"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), name
    for i in (0, 41, 42, 45, 200, len(a.m_prob) - 1):
        ra, rb = a.ranking(i), b.ranking(i)
        assert (ra is None) == (rb is None)
        if ra is not None:
            assert ra[0] == rb[0] and ra[1].dtype == np.float64 and ra[1].tobytes() == rb[1].tobytes()


def _cuts(T, sizes):
    """the block lengths `sizes` until T columns are used up, the last one taking what is left"""
    res = []
    for n in sizes:
        if sum(res) >= T:
            break
        res.append(min(n, T - sum(res)))
    if sum(res) < T:
        res.append(T - sum(res))
    return res


def _run_bank(engine, bank, specs, cuts, trackers=None, device=False):
    """pushes the recordings round by round (a recording that has run out brings (92, 0)) -> per stream the
    concatenated TrackResult; trackers: every push result is compared with the PieceTracker of that stream"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    parts, at = [[] for _ in specs], [0] * len(specs)
    for rnd in range(max(len(c) for c in cuts)):
        take = [c[rnd] if rnd < len(c) else 0 for c in cuts]
        blocks = [np.ascontiguousarray(s[:, a:a + n]) for s, a, n in zip(specs, at, take)]
        if device:
            flat = np.concatenate([b.ravel() for b in blocks])
            buf = engine.alloc(max(4, flat.nbytes)).upload(flat)
            try:
                got = bank.push(pid.DeviceArrays(buf, _offsets([b.size for b in blocks]), [b.shape for b in blocks]))
            finally:
                buf.free()
        else:
            got = bank.push(blocks)
        assert len(got) == len(specs)
        for s, (r, n) in enumerate(zip(got, take)):
            assert r.m_prob.shape == r.voiced.shape == (n,)
            if n == 0:
                assert r.pieces.shape == r.counts.shape == (0, TOP_K) and r.idx.shape == (0, N_CAND)
                assert len(r.frames) == len(r.n_out) == len(r.history) == 0
                continue
            if trackers is not None:
                _same(r, trackers[s].push(blocks[s]))
            r.frames = r.frames + at[s]
            parts[s].append(r)
            at[s] += n
    assert at == [s.shape[1] for s in specs] and list(bank.n_frames) == at
    assert list(bank.n_voiced) == [sum(len(p.frames) for p in ps) for ps in parts]
    cat = lambda ps, name: np.concatenate([getattr(p, name) for p in ps])
    return [pid.TrackResult(*[cat(ps, n) for n in ("m_prob", "voiced", "frames", "pieces", "counts", "n_out", "history")],
                            bank.db.id_to_name, cat(ps, "idx")) for ps in parts]


@pytest.mark.parametrize("blocks", ["5", "irregular"])
def test_bank_equals_a_tracker_per_stream_and_the_host_loop(engine, case, blocks):
    from audio_sheet_retrieval_amd import piece_identification as pid
    db, specs, host = case
    assert all(len(h.frames) for h in host) and not host[2].voiced[195:245].any()      # the gate opens, closes, reopens
    sizes = {"5": [5] * 80, "irregular": [1, 41, 42, 43]}[blocks]
    cuts = [_cuts(s.shape[1], sizes) for s in specs]
    levels = [s.sum(axis=0).max() for s in specs]
    bank = pid.PieceTrackerBank(engine, db, levels, TOP_K, N_CAND, RUNNING)
    try:
        trackers = [pid.PieceTracker(engine, db, lv, TOP_K, N_CAND, RUNNING) for lv in levels]
        for g, h in zip(_run_bank(engine, bank, specs, cuts, trackers=trackers), host):
            _same(g, h)
        bank.reset()                                                 # a second pass over buffers nobody zeroed,
        for g, h in zip(_run_bank(engine, bank, specs, cuts, device=True), host):      # the rounds as device handles
            _same(g, h)
    finally:
        bank.close()
    small = pid.PieceTrackerBank(engine, db, levels, TOP_K, N_CAND, RUNNING, max_windows=7)
    try:
        for g, h in zip(_run_bank(engine, small, specs, cuts), host):
            _same(g, h)
    finally:
        small.close()


def test_bank_of_one_stream_pushed_column_by_column(engine, case):
    from audio_sheet_retrieval_amd import piece_identification as pid
    db, specs, host = case
    bank = pid.PieceTrackerBank(engine, db, [specs[1].sum(axis=0).max()], TOP_K, N_CAND, RUNNING)
    try:
        tracker = pid.PieceTracker(engine, db, specs[1].sum(axis=0).max(), TOP_K, N_CAND, RUNNING)
        _same(_run_bank(engine, bank, specs[1:2], [[1] * 60], trackers=[tracker])[0], host[1])
        with pytest.raises(ValueError, match="blocks for 1 streams"):
            bank.push([specs[1][:, :1]] * 2)
        with pytest.raises(ValueError, match=r"expected a \(92, n >= 0\) block"):
            bank.push([specs[1][:91, :1]])
    finally:
        bank.close()
    with pytest.raises(ValueError, match="closed"):
        bank.push([specs[1][:, :1]])
    with pytest.raises(ValueError, match="n_candidates=701"):
        pid.PieceTrackerBank(engine, db, [1.0], n_candidates=701)
    with pytest.raises(ValueError, match="running_frames"):
        pid.PieceTrackerBank(engine, db, [1.0], running_frames=0)


# ---- 5. samples in, ranking out ------------------------------------------------------------------------------------
def _recording(rate, seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    t = np.arange(n) / float(rate)
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in
            zip(rng.uniform(0.1, 0.4, 4), rng.uniform(80, 3000, 4), rng.uniform(0, 6, 4)))
    return (x / np.abs(x).max() * 0.8 + 0.01 * rng.standard_normal(n)).astype(np.float32)


def _same_track(a, b):
    assert a.m_prob.tobytes() == b.m_prob.tobytes() and not np.isnan(a.m_prob).any()
    for name in ("voiced", "frames", "pieces", "counts", "n_out", "history", "idx"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and np.array_equal(x, y), name


def test_batched_live_tracking_equals_the_default_and_the_finished_spectrograms(engine, case):
    from audio_sheet_retrieval_amd import piece_identification as pid
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    db = case[0]
    processor = SpectrogramProcessor(engine)
    rates = [44100, 22050, 44100]
    recs = [_recording(r, sec, 90 + k) for k, (r, sec) in enumerate(zip(rates, (3.0, 3.1, 2.4)))]
    specs = processor.process_many(recs, None, rates)
    want = pid.track_scores(engine, db, specs, 3, 5, 10, return_idx=True)
    assert all(len(w.frames) > 5 for w in want)                             # the gate opens: the vote is exercised
    steps = [r // 10 for r in rates]
    default = pid.live_track_scores(engine, db, processor, recs, rates, steps, None, 3, 5, 10)
    got = pid.live_track_scores(engine, db, processor, recs, rates, steps, None, 3, 5, 10, batched=True)
    assert len(got) == len(default) == 3
    for g, d, w in zip(got, default, want):
        _same_track(g, d)
        _same_track(g, w)


# ---- 6. the driver -------------------------------------------------------------------------------------------------
sys.path.insert(0, HERE)
from test_gpu_umc import KEPT, TAG, _engine, _omr_flags, _umc_dir, exp_root  # noqa: E402,F401


def test_driver_live_bank_prints_and_dumps_what_live_does(exp_root, tmp_path, capsys):  # noqa: F811
    """one run of the driver with --live --bank; what --live prints and dumps for the same recordings and the saved data
    base comes from the driver's own live_track and report_tracking (tests/test_gpu_audio_stream.py runs --live itself)"""
    from audio_sheet_retrieval_amd import umc_a2s_server
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    from audio_sheet_retrieval_amd.audio_sheet_server import report_tracking
    from audio_sheet_retrieval_amd.piece_identification import EmbeddingDB
    data_dir = _umc_dir(tmp_path)
    res = umc_a2s_server.main(["--model", "models/%s.py" % MODEL, "--data_dir", data_dir, "--train_split",
                               "splits/all_split.yaml", "--config", "exp_configs/mutopia_full_aug.yaml", "--n_candidates",
                               "5", "--init_sheet_db", "--live", "--bank", "--block_ms", "100", "--resample",
                               "--dump_results"] + _omr_flags(exp_root))
    text = capsys.readouterr().out
    dump = exp_root / MODEL / ("umc_tracking_%s_umc_test_A2S.yaml" % TAG)
    with open(dump) as fp:
        dumped = yaml.safe_load(fp)
    names = [n for n in KEPT if n != "p7_no_score_ppq"]
    eng = _engine()
    db = EmbeddingDB.load(eng, "umc_sheet_db_file.pkl")
    try:
        tracked = umc_a2s_server.live_track(eng, db, SpectrogramProcessor(eng), [os.path.join(data_dir, n) for n in names],
                                            names, "score_ppq", 5, 100, 100.0)
        want = report_tracking(*tracked, res_file=str(dump))
    finally:
        db.close()
        eng.close()
    want_text = capsys.readouterr().out
    with open(dump) as fp:
        assert yaml.safe_load(fp) == dumped == res == want
    assert len(want["first_lead"]) == len(names) == want_text.count("of the voiced frames")
    assert text.endswith(want_text) and "Streaming every recording" in text


def test_driver_bank_needs_live(capsys):
    from audio_sheet_retrieval_amd import umc_a2s_server
    with pytest.raises(SystemExit) as err:
        umc_a2s_server._arguments(["--model", "models/%s.py" % MODEL, "--data_dir", "x", "--bank"], "A2S")
    assert err.value.code == 2 and "--bank needs --live" in capsys.readouterr().err
