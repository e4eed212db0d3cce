"""GPU: the running vote of the live server (asr_track_gate_dev, asr_track_vote_batch_dev, piece_identification.
track_scores / track_score / PieceTracker, audio_sheet_server --track) - every comparison exact: the vote kernel against
numpy, the gate kernel against track_gate_host, the batched pass and the streaming session against track_score_host.
The sign and payload of a NaN (a silent recording's 0 / 0) are the dividing unit's choice and not part of any
format: NaNs are compared by position, everything else by its bytes."""
import os
import pickle

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = "mutopia_ccal_cont"


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


# ---- the vote kernel ---------------------------------------------------------------------------------------------
def _vote_ref(idx, ids, first, count, top_k, running_frames, emit_from=None):
    from audio_sheet_retrieval_amd.piece_identification import track_vote_host
    P, K, N = [], [], []
    for r in range(len(first)):
        rows = idx[first[r]:first[r] + count[r]]
        p, c, n, _ = track_vote_host(ids[rows].reshape(len(rows), idx.shape[1]), top_k, running_frames)
        e = 0 if emit_from is None else emit_from[r]
        P.append(p[e:]), K.append(c[e:]), N.append(n[e:])
    return np.concatenate(P), np.concatenate(K), np.concatenate(N)


@pytest.mark.parametrize("n_pieces", [1, 2, 300])
@pytest.mark.parametrize("lds_cap", [None, "1"])
def test_vote_kernel_equals_numpy(engine, monkeypatch, n_pieces, lds_cap):
    monkeypatch.setenv("ASR_TRACK_SEG_FRAMES", "4")                 # 13 frames span four segments
    if lds_cap:
        monkeypatch.setenv("ASR_TRACK_LDS_PIECES", lds_cap)         # n_pieces > 1: the workspace path
    rng = np.random.default_rng(n_pieces)
    n_db = 900
    ids = rng.integers(0, n_pieces, size=n_db).astype(np.int32)
    d_ids = engine.alloc(ids.nbytes).upload(ids)
    voted = rng.choice(n_pieces, size=min(3, n_pieces), replace=False)           # ties are the rule
    pool = np.flatnonzero(np.isin(ids, voted))
    try:
        for running_frames in (1, 2, 3, 7):
            lengths = [0, 1, running_frames - 1, running_frames, running_frames + 1, 13]
            count = np.array(lengths, np.int64)
            first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
            for n_candidates in (1, 3, 25):
                idx = rng.choice(pool, size=(int(count.sum()), n_candidates)).astype(np.int32)
                d_idx = engine.alloc(idx.nbytes).upload(idx)
                args = (n_candidates, running_frames, d_ids.ptr, n_db, n_pieces)
                try:
                    for top_k in (1, 3, 64):
                        tag = (running_frames, n_candidates, top_k)
                        got = engine.track_vote_batch_dev(d_idx.ptr, len(idx), first, count, *args, top_k)
                        want = _vote_ref(idx, ids, first, count, top_k, running_frames)
                        assert got[0].shape == (len(idx), top_k) and got[2].shape == (len(idx),)
                        for g, w in zip(got, want):
                            assert g.dtype == np.int32 and np.array_equal(g, w), tag
                        assert top_k < 64 or np.all(got[2] < top_k)                 # fewer voted pieces than top_k
                        if top_k != 3:
                            continue
                        # three recordings of different lengths in one call = three single calls
                        sel = [5, 1, 4]
                        one = engine.track_vote_batch_dev(d_idx.ptr, len(idx), first[sel], count[sel], *args, top_k)
                        singles = [engine.track_vote_batch_dev(d_idx.ptr, len(idx), first[[r]], count[[r]], *args, top_k)
                                   for r in sel]
                        for k in range(3):
                            assert np.array_equal(one[k], np.concatenate([s[k] for s in singles])), tag
                            assert np.array_equal(one[k], np.concatenate([got[k][first[r]:first[r] + count[r]]
                                                                          for r in sel])), tag
                        # emit_from: the frames before it only feed the history
                        emit = np.array([0, 1, 0, running_frames - 1, 1, 6], np.int64)
                        tail = engine.track_vote_batch_dev(d_idx.ptr, len(idx), first, count, *args, top_k, emit_from=emit)
                        keep = np.concatenate([np.arange(first[r] + emit[r], first[r] + count[r]) for r in range(6)])
                        for k in range(3):
                            assert np.array_equal(tail[k], got[k][keep]), tag
                finally:
                    d_idx.free()
    finally:
        d_ids.free()


def test_vote_ignores_invalid_entries(engine, monkeypatch):
    monkeypatch.setenv("ASR_TRACK_SEG_FRAMES", "4")
    ids = np.array([0, 1, 1, 7, -2, 2], np.int32)                   # piece ids 7 and -2 lie outside [0, 3)
    idx = np.array([[0, 3], [4, 1], [2, -1], [6, 5], [5, 5], [1, 0]], np.int32)   # -1 and 6 outside [0, 6)
    d_ids, d_idx = engine.alloc(ids.nbytes).upload(ids), engine.alloc(idx.nbytes).upload(idx)
    try:
        p, c, n = engine.track_vote_batch_dev(d_idx.ptr, 6, [0], [6], 2, 2, d_ids.ptr, 6, 3, 2)
        assert p.tolist() == [[0, -1], [1, 0], [1, -1], [2, 1], [2, -1], [2, 1]]
        assert c.tolist() == [[1, 0], [1, 1], [2, 0], [1, 1], [3, 0], [2, 1]] and n.tolist() == [1, 2, 1, 2, 1, 2]
    finally:
        d_ids.free()
        d_idx.free()


def test_invalid_sizes_return_invalid(engine):
    from audio_sheet_retrieval_amd import _lib
    lib = engine.lib
    ids, idx = np.zeros(8, np.int32), np.zeros((4, 2), np.int32)
    d_ids, d_idx = engine.alloc(ids.nbytes).upload(ids), engine.alloc(idx.nbytes).upload(idx)
    out = np.empty(4 * 64, np.int32)
    p = out.ctypes.data
    one, four, five, neg = (np.array([v], np.int64) for v in (0, 4, 5, -1))
    q = lambda x: x.ctypes.data
    good = dict(n_rows=4, first=one, count=four, emit=None, n_cand=2, rf=3, n_db=8, n_pieces=3, top_k=2)
    bad = [dict(top_k=0), dict(top_k=65), dict(n_cand=0), dict(rf=0), dict(n_db=1), dict(n_pieces=0), dict(count=five),
           dict(first=neg), dict(emit=five), dict(emit=neg), dict(n_rows=3)]
    try:
        for change in [{}] + bad:
            a = dict(good, **change)
            rc = lib.asr_track_vote_batch_dev(engine.ctx, d_idx.ptr, a["n_rows"], 1, q(a["first"]), q(a["count"]),
                                              None if a["emit"] is None else q(a["emit"]), a["n_cand"], a["rf"],
                                              d_ids.ptr, a["n_db"], a["n_pieces"], a["top_k"], p, p, p)
            assert rc == (_lib.ASR_ERR_INVALID if change else _lib.ASR_OK), change
            if change:
                assert b"track_vote_batch" in lib.asr_last_error(engine.ctx)
        with pytest.raises(_lib.AsrError, match="track_vote_batch"):
            engine.track_vote_batch_dev(d_idx.ptr, 4, [0], [4], 2, 3, d_ids.ptr, 8, 3, 65)
        spec = np.ones((5, 50), np.float32)
        d_spec = engine.alloc(spec.nbytes).upload(spec)
        try:
            for width in (7, 129, 0, -1):
                with pytest.raises(_lib.AsrError, match="track_gate"):
                    engine.track_gate_dev(d_spec.ptr, spec.size, [0], [spec.shape], width)
            for off, shape in ((1, (5, 50)), (0, (5, 51)), (0, (0, 50)), (0, (5, 0)), (-1, (5, 50))):
                with pytest.raises(_lib.AsrError, match="track_gate"):
                    engine.track_gate_dev(d_spec.ptr, spec.size, [off], [shape], 8)
            m, v, level = engine.track_gate_dev(d_spec.ptr, spec.size, [0], [spec.shape], 8)      # still works
            assert m.tolist() == [np.float32(5.0 / 8.0) / np.float32(np.float32(5.0) * np.float32(0.15))] + [1.0] * 49
            assert v.tolist() == [False] * 8 + [True] * 42 and level.tolist() == [5.0]
        finally:
            d_spec.free()
    finally:
        d_ids.free()
        d_idx.free()


# ---- the gate kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [8, 42, 47])
def test_gate_kernel_equals_the_host_gate(engine, width):
    from audio_sheet_retrieval_amd.piece_identification import track_gate_host
    rng = np.random.default_rng(width)
    specs = [(3.0 * rng.random((bins, T)) ** 2).astype(np.float32) for bins in (5, 92) for T in (41, 42, 43, 44, 300)]
    specs.append(np.zeros((92, 60), np.float32))                                       # silent: 0 / 0
    ramp = np.abs(np.linspace(-1.0, 1.0, 300, dtype=np.float32)) ** 3                  # loud - silent - loud
    specs.append((3.0 * rng.random((92, 300)) ** 2).astype(np.float32) * ramp)
    refs = [track_gate_host(s, width) for s in specs]
    d = np.diff(refs[-1][1].astype(int))
    assert (d == 1).any() and (d == -1).any()                       # m_prob crosses 0.5 in both directions
    assert np.isnan(refs[-2][0]).all()
    assert not any(r[1].any() for s, r in zip(specs, refs) if s.shape[1] <= width)     # no eligible frame
    offsets = np.concatenate([[0], np.cumsum([s.size for s in specs])[:-1]])
    flat = np.concatenate([s.ravel() for s in specs])
    d_src = engine.alloc(flat.nbytes).upload(flat)
    try:
        shapes = [s.shape for s in specs]
        m, v, level = engine.track_gate_dev(d_src.ptr, flat.size, offsets, shapes, width)
        assert m.dtype == np.float32 and v.dtype == bool
        first = np.concatenate([[0], np.cumsum([s.shape[1] for s in specs])])
        for r, (rm, rv) in enumerate(refs):
            gm, gv = m[first[r]:first[r + 1]], v[first[r]:first[r + 1]]
            assert np.array_equal(np.isnan(gm), np.isnan(rm)) and _bytes(gm) == _bytes(rm), (r, specs[r].shape)
            assert np.array_equal(gv, rv), (r, specs[r].shape)
            assert level[r].tobytes() == specs[r].sum(axis=0).max().tobytes()
            # one recording on its own, and with its level passed in: the same bits
            for norm in (None, [level[r]]):
                sm, sv, _ = engine.track_gate_dev(d_src.ptr, flat.size, [offsets[r]], [shapes[r]], width, norm=norm)
                assert _bytes(sm) == _bytes(gm) and np.array_equal(sv, gv), (r, norm)
        # frame0: the stream position of column 0 decides from where frames are eligible
        sm, sv, _ = engine.track_gate_dev(d_src.ptr, flat.size, [offsets[4]], [shapes[4]], width, frame0=[-5])
        assert _bytes(sm) == _bytes(refs[4][0]) and np.array_equal(sv, refs[4][1] & (np.arange(300) >= width + 5))
    finally:
        d_src.free()


# ---- end to end ------------------------------------------------------------------------------------------------------
TOP_K, N_CAND, RUNNING = 5, 5, 20


@pytest.fixture(scope="module")
def trained():
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        return [z["p%02d" % i] for i in range(len(param_shapes(MODEL)))]


@pytest.fixture(scope="module")
def case(engine, trained):
    """the data base, the recordings and track_score_host's results, computed once"""
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


def _same(a, b, idx=True):
    assert np.array_equal(np.isnan(a.m_prob), np.isnan(b.m_prob)) and _bytes(a.m_prob) == _bytes(b.m_prob)
    assert a.voiced.dtype == b.voiced.dtype == bool and np.array_equal(a.voiced, b.voiced)
    for name in ("frames", "pieces", "counts", "n_out", "history") + (("idx",) if idx else ()):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and np.array_equal(x, y), name
    for i in (0, 41, 42, 45, 200, len(a.m_prob) - 1):
        ra, rb = a.ranking(i), b.ranking(i)
        assert (ra is None) == (rb is None)
        if ra is not None:
            assert ra[0] == rb[0] and ra[1].dtype == np.float64 and ra[1].tobytes() == rb[1].tobytes()


def test_track_scores_equals_the_host_loop(engine, case):
    from audio_sheet_retrieval_amd import piece_identification as pid
    db, specs, host = case
    # what the recordings are made to cover: one eligible frame; ten silent columns do not close the gate; a hundred do
    assert host[0].frames.tolist() == [42] and host[1].frames.tolist() == list(range(42, 60))
    v = host[2].voiced
    assert v[42:150].all() and not v[195:245].any() and v[300:].all() and not v[:42].any()
    assert host[2].ranking(41) is None and host[2].ranking(240)[0] == host[2].ranking(int(host[2].frames[host[2].frames < 195][-1]))[0]
    got = pid.track_scores(engine, db, specs, TOP_K, N_CAND, RUNNING, return_idx=True)
    chunked = pid.track_scores(engine, db, specs, TOP_K, N_CAND, RUNNING, max_windows=7, return_idx=True)
    for g, c, h in zip(got, chunked, host):
        _same(g, h)
        _same(c, h)
    assert pid.track_scores(engine, db, specs, TOP_K, N_CAND, RUNNING)[0].idx is None
    _same(pid.track_score(engine, db, specs[2], TOP_K, N_CAND, RUNNING, return_idx=True), host[2])
    # a device handle in place of host arrays
    flat = np.concatenate([s.ravel() for s in specs])
    buf = engine.alloc(flat.nbytes).upload(flat)
    try:
        offsets = [0, specs[0].size, specs[0].size + specs[1].size]
        dev = pid.track_scores(engine, db, pid.DeviceArrays(buf, offsets, [s.shape for s in specs]), TOP_K, N_CAND,
                               RUNNING, return_idx=True)
    finally:
        buf.free()
    for g, h in zip(dev, host):
        _same(g, h)


@pytest.mark.parametrize("blocks", ["1", "5", "irregular"])
def test_streaming_equals_the_whole_recording(engine, case, blocks):
    from audio_sheet_retrieval_amd import piece_identification as pid
    db, specs, host = case
    spec = specs[2]
    T = spec.shape[1]
    whole = pid.track_score(engine, db, spec, TOP_K, N_CAND, RUNNING, return_idx=True)
    _same(whole, host[2])
    sizes = {"1": [1] * T, "5": [5] * (T // 5), "irregular": [1, 41, 42, 43, T - 127]}[blocks]
    assert sum(sizes) == T
    tracker = pid.PieceTracker(engine, db, spec.sum(axis=0).max(), TOP_K, N_CAND, RUNNING)
    parts, at = [], 0
    for n in sizes:
        part = tracker.push(spec[:, at:at + n])
        assert part.m_prob.shape == part.voiced.shape == (n,)
        part.frames = part.frames + at
        parts.append(part)
        at += n
    cat = lambda name: np.concatenate([getattr(p, name) for p in parts])
    joined = pid.TrackResult(*[cat(n) for n in ("m_prob", "voiced", "frames", "pieces", "counts", "n_out", "history")],
                             db.id_to_name, cat("idx"))
    _same(joined, whole)
    assert tracker.n_frames == T and tracker.n_voiced == len(whole.frames)


# ---- the driver ----------------------------------------------------------------------------------------------------
def test_driver_track_dumps_two_lists(tmp_path, monkeypatch, trained, capsys):
    from audio_sheet_retrieval_amd import audio2sheet_align, audio_sheet_server
    monkeypatch.setattr(audio2sheet_align, "EXP_ROOT", str(tmp_path))
    d = tmp_path / MODEL
    d.mkdir()
    with open(d / "params_all_split_mutopia_full_aug.pkl", "wb") as fp:
        pickle.dump(trained, fp, protocol=2)
    monkeypatch.chdir(tmp_path)
    res = audio_sheet_server.main(["--model", "models/%s.py" % MODEL, "--data", "synthetic:3", "--train_split",
                                   "splits/all_split.yaml", "--config", "exp_configs/mutopia_full_aug.yaml",
                                   "--init_sheet_db", "--track", "--dump_results", "--n_candidates", "5",
                                   "--running_frames", "30"])
    with open(d / "tracking_all_split_mutopia_full_aug_A2S.yaml") as fp:
        dumped = yaml.safe_load(fp)
    assert dumped == res and sorted(dumped) == ["first_lead", "lead_share"]
    assert len(dumped["first_lead"]) == len(dumped["lead_share"]) == 3
    assert all(isinstance(f, int) and f >= -1 for f in dumped["first_lead"])
    assert all(0.0 <= s <= 1.0 for s in dumped["lead_share"])
    assert capsys.readouterr().out.count("of the voiced frames") == 3
