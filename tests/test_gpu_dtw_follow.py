"""GPU: streaming subsequence DTW (asr_dtw_follow_batch_dev / Engine.dtw_follow_batch), bit for bit against the numpy
restatement of its definition (alignment.follow_dtw_host on the oracle's float64 cosine distances) and, on the small
cases, directly against alignment.subseq_dtw_host on every prefix; the routes built on it: ScoreFollower over block
cuts against follow_scores and follow_scores_host, audio_sheet_server --follow.  Every accumulated value is one fixed
sequence of correctly rounded float64 operations, so every check is for equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")

# (B, S): one row / one column, one wave with and without idle lanes, the wave boundary, B > S, the largest block
SHAPES = [(1, 9), (9, 1), (7, 300), (63, 200), (64, 200), (65, 200), (129, 128), (300, 90), (1024, 1100)]
# reference rows (and state entries) per staged tile (csrc/dtw_follow_kernels.hip: FolCfg), several waves / one wave
TILE_ROWS = {32: (16, 8), 64: (8, 4)}


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _planted(rng, Q, S, dim):
    """a reference of S random rows and a query that follows a stretch of it (or all of it, resampled) with noise"""
    ref = rng.standard_normal((S, dim))
    L = max(1, min(S, int(round(Q / rng.uniform(0.6, 1.6)))))
    s0 = int(rng.integers(0, S - L + 1))
    rows = np.round(np.linspace(s0, s0 + L - 1, Q)).astype(int)
    qry = ref[rows] + 0.3 * rng.standard_normal((Q, dim))
    if dim == 1:
        qry, ref = np.sign(qry) + (qry == 0), np.sign(ref) + (ref == 0)      # 1-d codes: the direction is the sign
    return _unit(qry), _unit(ref)


def _tie_heavy(rng, Q, S, n_distinct, dim=32):
    """codes drawn from a handful of rows: many exactly equal distances, so the first-minimum order decides"""
    rows = rng.standard_normal((n_distinct, dim)).astype(np.float32)
    return rows[rng.integers(0, n_distinct, Q)], rows[rng.integers(0, n_distinct, S)]


def _host(q, r, state=None):
    from audio_sheet_retrieval_amd import alignment as al
    from oracle import retrieval as oret
    return al.follow_dtw_host(oret.cdist_cosine64(q, r), state)


def _same(got, want, what, state=True):
    """(cost, start, pos, (acc, org, rows)) of the device against the host's"""
    for k, name in enumerate(("cost", "start", "pos")):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, name)
    if state:
        assert np.array_equal(got[3][0], want[3][0]) and np.array_equal(got[3][1], want[3][1]), (what, "state")
        assert got[3][2] == want[3][2], (what, "rows")


@pytest.fixture(scope="module")
def engine():
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine("mutopia_ccal_cont")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def cases():
    """{dim: [(query, reference, host result)]}, computed once"""
    rng = np.random.default_rng(29)
    out = {32: [_planted(rng, B, S, 32) for B, S in SHAPES]}
    out[32] += [_planted(rng, 70, S, 32) for S in (15, 16, 17, 31, 32, 33)]          # around the staged tile length
    out[32] += [_planted(rng, 20, S, 32) for S in (7, 8, 9)]                         # ... and a one-wave workgroup's
    out[32] += [_tie_heavy(rng, 90, 260, 2), _tie_heavy(rng, 150, 100, 4), _tie_heavy(rng, 30, 40, 3)]
    out[1] = [_planted(rng, 20, 50, 1), _planted(rng, 70, 17, 1)]
    out[31] = [_planted(rng, 40, 300, 31), _planted(rng, 130, 33, 31), _tie_heavy(rng, 66, 90, 3, dim=31)]
    out[64] = [_planted(rng, 40, 300, 64), _planted(rng, 200, 150, 64), _tie_heavy(rng, 66, 90, 3, dim=64)]
    out[64] += [_planted(rng, 70, S, 64) for S in (7, 8, 9)] + [_planted(rng, 20, S, 64) for S in (3, 4, 5)]
    out[64] += [_planted(rng, 600, 100, 64)]        # its ring does not fit the LDS: reference rows read from global memory
    return {d: [(q, r, _host(q, r)) for q, r in v] for d, v in out.items()}


def _run(engine, items):
    return engine.dtw_follow_batch([q for q, _, _ in items], [r for _, r, _ in items], [(k, k) for k in range(len(items))])


@pytest.mark.parametrize("dim", [32, 1, 31, 64])
def test_device_equals_the_definition(engine, cases, dim):
    from audio_sheet_retrieval_amd import alignment as al
    from oracle import retrieval as oret
    if dim in (32, 64):     # S one below, equal to and one above the staged tile length, for either kind of workgroup
        for waves, tile in zip((2, 1), TILE_ROWS[dim]):
            assert all(any(len(r) == tile + k and (len(q) > 64) == (waves > 1) for q, r, _ in cases[dim])
                       for k in (-1, 0, 1))
    for (q, r, want), got in zip(cases[dim], _run(engine, cases[dim])):
        _same(got, want, (dim, q.shape, r.shape))
        if q.shape[0] * r.shape[0] <= 2100:                # directly against the parent call's definition, per prefix
            D = oret.cdist_cosine64(q, r)
            for i in range(len(q)):
                c, s, e, _ = al.subseq_dtw_host(D[:i + 1])
                assert (got[0][i], got[1][i], got[2][i]) == (c, s, e), (dim, q.shape, r.shape, i)


def test_rows_from_global_memory_give_the_same(engine, cases, monkeypatch):
    """ASR_DTW_SUBSEQ_LDS_CAP=1: every multi-wave workgroup reads its reference rows from global memory"""
    monkeypatch.setenv("ASR_DTW_SUBSEQ_LDS_CAP", "1")
    for dim in (32, 31, 64):
        items = [c for c in cases[dim] if len(c[0]) <= 300]
        for (q, r, want), got in zip(items, _run(engine, items)):
            _same(got, want, (dim, q.shape, r.shape))


@pytest.fixture(scope="module")
def stream():
    """a 340-row stream against 210 rows, a tie-heavy one against 97 rows, with the host results of the whole"""
    rng = np.random.default_rng(31)
    items = [_planted(rng, 340, 210, 32), _tie_heavy(rng, 340, 97, 3)]
    return [(q, r, _host(q, r)) for q, r in items]


CUTS = [0, 5, 69, 139, 140, 340]                            # blocks of 5, 64, 70, 1 and 200 rows


def test_carried_state_across_size_classes(engine, stream):
    """blocks of 5, 64, 70, 1 and 200 rows - one wave, a full wave, two waves, one lane, four waves - equal one call of
    340 rows and the host, outputs and final state"""
    for q, r, want in stream:
        _same(engine.dtw_follow_batch([q], [r], [(0, 0)])[0], want, "whole")
        state, parts = None, []
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            got = engine.dtw_follow_batch([q[a:b]], [r], [(0, 0)], [state])[0]
            # ... and every block against the host continued from the host's own state
            _same(got, _host(q[a:b], r, _host(q[:a], r)[3] if a else None), (a, b))
            state = got[3]
            parts.append(got)
        whole = tuple(np.concatenate([p[k] for p in parts]) for k in range(3)) + (state,)
        _same(whole, want, "blocks")


class _Raw(object):
    """queries, references and a state buffer on the device for calls of Engine.dtw_follow_batch_dev"""

    def __init__(self, engine, q, r, state_len, dim=32):
        self.engine, self.q, self.r, self.dim, self.state_len = engine, q, r, dim, state_len
        self.dq, self.dr = engine.alloc(q.nbytes).upload(q), engine.alloc(r.nbytes).upload(r)
        self.da, self.do = engine.alloc(state_len * 8), engine.alloc(state_len * 4)

    def put(self, acc, org):
        self.da.upload(np.ascontiguousarray(acc, np.float64))
        self.do.upload(np.ascontiguousarray(org, np.int32))

    def get(self):
        return self.da.download((self.state_len,), np.float64), self.do.download((self.state_len,), np.int32)

    def call(self, q_row, n_q, r_row, n_r, before, off, want=True, q_rows=None, r_rows=None, dim=None, state_len=None):
        return self.engine.dtw_follow_batch_dev(
            self.dq.ptr, len(self.q) if q_rows is None else q_rows, self.dr.ptr, len(self.r) if r_rows is None else r_rows,
            q_row, n_q, r_row, n_r, before, self.dim if dim is None else dim, self.da.ptr, self.do.ptr,
            self.state_len if state_len is None else state_len, off, want=want)

    def free(self):
        for b in (self.dq, self.dr, self.da, self.do):
            b.free()


def test_fresh_and_carried_pairs_at_odd_state_offsets(engine, stream):
    """one call: pair 0 carried (rows 139..), pair 1 fresh with its state full of NaN, pair 2 carried by one row; the
    states at odd offsets of a larger buffer, whose guard elements stay as they were"""
    (q0, r0, _), (q1, r1, _) = stream
    q, r = np.concatenate([q0, q1]), np.concatenate([r0, r1])
    S0, S1 = len(r0), len(r1)
    off = np.array([3, 3 + S0 + 5, 3 + S0 + 5 + S1 + 1], np.int64)       # pair 2: q1 against r0
    n = int(off[2] + S0 + 7)
    acc, org = np.full(n, -7.25), np.full(n, -99, np.int32)
    h0, h2 = _host(q0[:139], r0), _host(q1[:1], r0)
    acc[off[0]:off[0] + S0], org[off[0]:off[0] + S0] = h0[3][0], h0[3][1]
    acc[off[1]:off[1] + S1] = np.nan
    acc[off[2]:off[2] + S0], org[off[2]:off[2] + S0] = h2[3][0], h2[3][1]
    guard = np.ones(n, bool)
    for o, s in zip(off, (S0, S1, S0)):
        guard[o:o + s] = False
    raw = _Raw(engine, q, r, n)
    try:
        raw.put(acc, org)
        got = raw.call([139, 340, 341], [201, 66, 100], [0, S0, 0], [S0, S1, S0], [139, 0, 1], off)
        new_acc, new_org = raw.get()
    finally:
        raw.free()
    want = [_host(q0[139:], r0, h0[3]), _host(q1[:66], r1), _host(q1[1:101], r0, h2[3])]
    for p, (o, s) in enumerate(zip(off, (S0, S1, S0))):
        _same(got[p] + ((new_acc[o:o + s], new_org[o:o + s], want[p][3][2]),), want[p], p)
    assert np.array_equal(new_acc[guard], acc[guard]) and np.array_equal(new_org[guard], org[guard])
    assert guard.sum() == 3 + 5 + 1 + 7


def test_shared_sequences_and_batch_order(engine, cases):
    """pairs that share queries and references: each equals the pair alone and the host; the reversed batch gives the
    same"""
    items = cases[32]
    queries, refs = [q for q, _, _ in items[3:8]], [r for _, r, _ in items[2:7]]
    pairs = [(a, b) for a in range(len(queries)) for b in range(len(refs))]
    batch = engine.dtw_follow_batch(queries, refs, pairs)
    for (a, b), got in zip(pairs, batch):
        if (a + 2 * b) % 3 == 0:                                   # a third of them against the host, all against each other
            _same(got, _host(queries[a], refs[b]), (a, b))
        if a == b:
            _same(engine.dtw_follow_batch([queries[a]], [refs[b]], [(0, 0)])[0], got, (a, b, "alone"))
    for got, want in zip(engine.dtw_follow_batch(queries, refs, pairs[::-1]), batch[::-1]):
        _same(got, want, "reversed")


def test_a_query_longer_than_a_call(engine):
    """Engine.dtw_follow_batch splits 1500 rows into calls of 1024 and 476; a second pair ends in the first call"""
    rng = np.random.default_rng(37)
    q, r = _planted(rng, 1500, 130, 32)
    got = engine.dtw_follow_batch([q, q[:40]], [r], [(0, 0), (1, 0)])
    _same(got[0], _host(q, r), "long")
    _same(got[1], _host(q[:40], r), "short")


def test_all_outputs_null_still_advances(engine, stream):
    q, r, want = stream[0]
    S = len(r)
    raw = _Raw(engine, q, r, S)
    try:
        raw.put(np.full(S, np.nan), np.zeros(S, np.int32))
        assert raw.call([0], [100], [0], [S], [0], [0], want=False) is None
        got = raw.call([100], [240], [0], [S], [100], [0])[0]
        acc, org = raw.get()
    finally:
        raw.free()
    _same(got + ((acc, org, 340),), tuple(w[100:] for w in want[:3]) + (want[3],), "second call")


def test_invalid_arguments_are_refused_and_touch_no_state(engine):
    from audio_sheet_retrieval_amd import _lib
    rng = np.random.default_rng(41)
    q = _unit(rng.standard_normal((1030, 32)))
    raw = _Raw(engine, q, q, 64)
    acc, org = rng.random(64), rng.integers(0, 9, 64).astype(np.int32)
    try:
        raw.put(acc, org)
        bad = [dict(n_q=[0, 10]), dict(n_q=[1025, 10]), dict(dim=0), dict(dim=65), dict(q_row=[1025, 0]),
               dict(r_row=[0, 1011]), dict(r_row=[-1, 0]), dict(off=[0, 45]), dict(off=[-1, 30]), dict(off=[0, 19]),
               dict(off=[10, 0]), dict(before=[-1, 0]), dict(before=[2 ** 31 - 10, 0])]
        for kw in bad:
            a = dict(q_row=[0, 0], n_q=[10, 10], r_row=[0, 100], n_r=[20, 20], before=[3, 0], off=[0, 30], dim=None)
            a.update(kw)
            with pytest.raises(_lib.AsrError) as e:
                raw.call(a["q_row"], a["n_q"], a["r_row"], a["n_r"], a["before"], a["off"], dim=a["dim"])
            assert e.value.code == _lib.ASR_ERR_INVALID, kw
            now = raw.get()
            assert now[0].tobytes() == acc.tobytes() and now[1].tobytes() == org.tobytes(), kw
        # the same tables are accepted as they stand, and an empty batch is
        assert len(raw.call([0, 0], [10, 10], [0, 100], [20, 20], [3, 0], [0, 30])) == 2
        assert raw.call([], [], [], [], [], []) == []
        assert engine.dtw_follow_batch([], [], []) == []
    finally:
        raw.free()


# ---- ScoreFollower / follow_scores: window codes and the carried alignment against the resident data base ------------
@pytest.fixture(scope="module")
def synthetic(engine):
    """4 synthetic pieces on trained parameters: the pool and its from_pool data base"""
    from audio_sheet_retrieval_amd import audio2sheet_align
    from audio_sheet_retrieval_amd.piece_identification import EmbeddingDB
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(PARAMS) as z:
        engine.set_params([z["p%02d" % i] for i in range(len(param_shapes("mutopia_ccal_cont")))])
    data = audio2sheet_align.select_pieces("synthetic:4", 23)
    pool = AudioScoreRetrievalPool(engine, data["images"], data["specs"], data["o2c_maps"],
                                   data_augmentation=dict(NO_AUGMENT), shuffle=False)
    db = EmbeddingDB.from_pool(engine, pool, 1, names=data["names"])
    yield data, pool, db
    db.close()


def _same_following(got, want):
    assert got.pieces == want.pieces and got.names == want.names
    for key in ("frames", "cost", "row", "start_row", "x", "start_x", "best"):
        g, w = getattr(got, key), getattr(want, key)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), key


def _pushed(pid, engine, db, spec, pieces, cuts, **kw):
    session = pid.ScoreFollower(engine, db, pieces, **kw)
    try:
        res = [session.push(spec[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        state = session.state()
    finally:
        session.close()
    cat = lambda key: np.concatenate([getattr(r, key) for r in res])
    return res, pid.FollowResult(cat("frames"), cat("cost"), cat("row"), cat("start_row"), cat("x"), cat("start_x"),
                                 res[0].pieces, res[0].names), state


def test_score_follower_equals_follow_scores_and_the_host(engine, synthetic):
    from audio_sheet_retrieval_amd import audio_sheet_server as drv, piece_identification as pid
    data, pool, db = synthetic
    cols = drv.pool_sheet_columns(pool, len(db))
    specs = [s[0] for s in pool.specs]
    cands = [[1, 0, 3], ["synthetic_001"], [2, 3], [3, 0, 1, 2]]
    kw = dict(step_spec=2, sheet_columns=cols)
    whole = pid.follow_scores(engine, db, specs, cands, **kw)
    host = pid.follow_scores_host(engine, db, specs, cands, **kw)
    segs = pid.piece_segments(db.ids)
    for e, (got, want) in enumerate(zip(whole, host)):
        _same_following(got, want)
        T = specs[e].shape[1]
        assert np.array_equal(got.frames, np.arange(0, T - 42 + 1, 2)) and got.cost.shape == (len(got.frames), len(cands[e]))
        assert got.names == [data["names"][p] if not isinstance(p, str) else p for p in cands[e]]
        assert np.array_equal(got.best, np.argmin(got.cost, axis=1))
        for c, piece in enumerate(got.pieces):
            first, n = segs[piece]
            assert (0 <= got.start_row[:, c]).all() and (got.start_row[:, c] <= got.row[:, c]).all() and (got.row[:, c] < n).all()
            assert np.array_equal(got.x[:, c], cols[first + got.row[:, c]])
            assert np.array_equal(got.start_x[:, c], cols[first + got.start_row[:, c]])
    # the stream of recording 0 in blocks of 20 columns, and in blocks shorter than a window of uneven lengths
    T = specs[0].shape[1]
    rng = np.random.default_rng(3)
    uneven = [0]
    while uneven[-1] < T:
        uneven.append(min(T, uneven[-1] + int(rng.integers(1, 12))))
    for cuts in (list(range(0, T, 20)) + [T], uneven):
        res, cat, state = _pushed(pid, engine, db, specs[0], cands[0], cuts, **kw)
        _same_following(cat, whole[0])
        assert len(res[0].frames) == 0 and res[0].cost.shape == (0, 3) and res[0].best.shape == (0,)   # no window yet
        assert sum(len(r.frames) > 0 for r in res) > 10
        for c, piece in enumerate(cat.pieces):               # the final state is that of the whole stream on the host
            first, n = segs[piece]
            acc, org, rows = state[c]
            assert rows == len(cat.frames) and acc.shape == (n,)
            assert acc[cat.row[-1, c]] / rows == cat.cost[-1, c] and org[cat.row[-1, c]] == cat.start_row[-1, c]


def test_a_recording_of_more_than_1024_windows(engine, synthetic):
    """step_spec = 1 over 1331 columns: 1290 windows, two follow calls per route; one push of the whole and pushes of
    600 columns give the same"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    data, pool, db = synthetic
    spec = np.ascontiguousarray(np.hstack([pool.specs[1][0], pool.specs[2][0]]))
    assert spec.shape[1] - 42 + 1 == 1290
    whole = pid.follow_scores(engine, db, [spec], [[2, 1]], step_spec=1)[0]
    _same_following(whole, pid.follow_scores_host(engine, db, [spec], [[2, 1]], step_spec=1)[0])
    assert whole.cost.shape == (1290, 2)
    for cuts in ([0, spec.shape[1]], [0, 600, 1200, spec.shape[1]]):
        _same_following(_pushed(pid, engine, db, spec, [2, 1], cuts, step_spec=1)[1], whole)


def test_driver_follow_dumps_one_entry_per_piece(tmp_path):
    """audio_sheet_server --follow in a child process on four synthetic pieces"""
    import pickle
    import yaml
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(PARAMS) as z:
        trained = [z["p%02d" % i] for i in range(len(param_shapes("mutopia_ccal_cont")))]
    d = tmp_path / "mutopia_ccal_cont"
    d.mkdir()
    with open(d / "params_all_split_mutopia_full_aug.pkl", "wb") as fp:
        pickle.dump(trained, fp, protocol=2)
    env = dict(os.environ, ASR_EXP_ROOT=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "audio_sheet_retrieval_amd.audio_sheet_server", "--model",
                          "models/mutopia_ccal_cont.py", "--data", "synthetic:4", "--train_split", "splits/all_split.yaml",
                          "--config", "exp_configs/mutopia_full_aug.yaml", "--init_sheet_db", "--follow", "--dump_results",
                          "--block_frames", "50", "--locate_pieces", "3"],
                         capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    with open(d / "following_all_split_mutopia_full_aug_A2S.yaml") as fp:
        dumped = yaml.safe_load(fp)
    assert [e["name"] for e in dumped] == ["synthetic_%03d" % i for i in range(4)]
    lengths = [464, 644, 687, 490]
    for e, T in zip(dumped, lengths):
        assert sorted(e) == ["best_share", "candidate", "median_error", "name", "windows"]
        assert e["windows"] == (T - 42) // 2 + 1 and 0.0 <= e["best_share"] <= 1.0
        assert e["candidate"] == (e["median_error"] is not None)
    lines = out.stdout.splitlines()
    assert all(sum(ln.startswith("own piece") and ln.endswith(e["name"]) for ln in lines) == 1 for e in dumped)
    assert "following of 4 pieces written to" in out.stdout
