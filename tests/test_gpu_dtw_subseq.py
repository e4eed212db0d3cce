"""GPU: batched subsequence DTW (asr_dtw_subseq_batch_dev / Engine.dtw_subseq_batch), bit for bit against the numpy
restatement of its definition (alignment.subseq_dtw_host on the oracle's float64 cosine distances), and the routes built
on it: piece_identification.locate_scores against locate_scores_host, audio_sheet_server --locate.  Every accumulated
value is one fixed sequence of correctly rounded float64 operations, so every check is for equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")

# (Q, S): one row / one column, one wave with and without idle lanes, the wave boundary, Q > S, the largest query
SHAPES = [(1, 9), (9, 1), (40, 300), (63, 200), (64, 200), (65, 200), (128, 129), (129, 128), (300, 90), (1024, 1100)]
TILE_ROWS = {32: 16, 1: 16, 31: 16, 64: 8}     # reference rows per staged tile (csrc/dtw_subseq_kernels.hip: SubCfg)


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


def _host(q, r):
    from audio_sheet_retrieval_amd import alignment as al
    from oracle import retrieval as oret
    cost, start, end, path = al.subseq_dtw_host(oret.cdist_cosine64(q, r))
    return cost, start, end, len(path[0]), al.subseq_positions(path, len(q))


def _same(got, want, what):
    assert got[0] == want[0], (what, "cost", got[0], want[0])
    assert got[1:4] == want[1:4], (what, "start/end/path_len", got[1:4], want[1:4])
    assert np.array_equal(got[4], want[4]), (what, "pos")


@pytest.fixture(scope="module")
def engine():
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine("mutopia_ccal_cont")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def cases():
    """{dim: [(query, reference, host result)]}, computed once"""
    rng = np.random.default_rng(23)
    out = {32: [_planted(rng, Q, S, 32) for Q, S in SHAPES]}
    out[32] += [_planted(rng, 70, S, 32) for S in (15, 16, 17, 31, 32, 33)]          # around the staged tile length
    out[32] += [_tie_heavy(rng, 90, 260, 2), _tie_heavy(rng, 150, 100, 4)]
    out[1] = [_planted(rng, 20, 50, 1), _planted(rng, 70, 17, 1)]
    out[31] = [_planted(rng, 40, 300, 31), _planted(rng, 130, 33, 31), _tie_heavy(rng, 66, 90, 3, dim=31)]
    out[64] = [_planted(rng, 40, 300, 64), _planted(rng, 200, 150, 64), _tie_heavy(rng, 66, 90, 3, dim=64)]
    out[64] += [_planted(rng, 70, S, 64) for S in (7, 8, 9)]
    out[64] += [_planted(rng, 600, 100, 64)]        # its ring does not fit the LDS: reference rows read from global memory
    return {d: [(q, r, _host(q, r)) for q, r in v] for d, v in out.items()}


def _run(engine, items):
    return engine.dtw_subseq_batch([q for q, _, _ in items], [r for _, r, _ in items], [(k, k) for k in range(len(items))])


@pytest.mark.parametrize("dim", [32, 1, 31, 64])
def test_device_equals_the_definition(engine, cases, dim):
    if dim in (32, 64):     # S one below, equal to and one above the staged tile length is among the cases
        assert all(any(len(r) == TILE_ROWS[dim] + k for _, r, _ in cases[dim]) for k in (-1, 0, 1))
    for (q, r, want), got in zip(cases[dim], _run(engine, cases[dim])):
        _same(got, want, (dim, q.shape, r.shape))


def test_rows_from_global_memory_give_the_same(engine, cases, monkeypatch):
    """ASR_DTW_SUBSEQ_LDS_CAP=1: every multi-wave workgroup reads its reference rows from global memory"""
    monkeypatch.setenv("ASR_DTW_SUBSEQ_LDS_CAP", "1")
    for dim in (32, 31, 64):
        items = [c for c in cases[dim] if len(c[0]) <= 300]
        for (q, r, want), got in zip(items, _run(engine, items)):
            _same(got, want, (dim, q.shape, r.shape))


def test_shared_sequences_batch_order_and_chunks(engine, cases, monkeypatch):
    """pairs that share queries and references: each equals the pair alone; the reversed batch and a batch cut into
    several chunks (ASR_DTW_BUDGET_MB=1; the pairs need 2.3 MB of direction bytes) give the same"""
    items = cases[32]
    queries, refs = [q for q, _, _ in items[4:9]], [r for _, r, _ in items[3:10]]
    pairs = [(a, b) for a in range(len(queries)) for b in range(len(refs))]
    batch = engine.dtw_subseq_batch(queries, refs, pairs)
    for (a, b), got in zip(pairs, batch):
        if (a + 2 * b) % 3 == 0:                                   # a third of them against the host, all against each other
            _same(got, _host(queries[a], refs[b]), (a, b))
        _same(engine.dtw_subseq_batch([queries[a]], [refs[b]], [(0, 0)])[0], got, (a, b, "alone"))
    for got, want in zip(engine.dtw_subseq_batch(queries, refs, pairs[::-1]), batch[::-1]):
        _same(got, want, "reversed")
    monkeypatch.setenv("ASR_DTW_BUDGET_MB", "1")
    assert sum(len(queries[a]) * (len(refs[b]) + len(queries[a])) for a, b in pairs) > 2 << 20
    for got, want in zip(engine.dtw_subseq_batch(queries, refs, pairs), batch):
        _same(got, want, "chunked")


@pytest.mark.parametrize("dim", [32, 31])
def test_reference_inside_a_larger_buffer(engine, cases, dim):
    """r_dev as an offset into a larger buffer (the data-base case); with dim 31 the rows are not 16-byte aligned"""
    (q, r, want), (q2, r2, want2) = cases[dim][2], cases[dim][1]
    rng = np.random.default_rng(5)
    big = np.concatenate([rng.standard_normal((7, dim)).astype(np.float32), r, r2,
                          rng.standard_normal((3, dim)).astype(np.float32)])
    qq = np.concatenate([q, q2])
    dq, dr = engine.alloc(qq.nbytes).upload(qq), engine.alloc(big.nbytes).upload(big)
    try:
        cost, start, end, ln, pos = engine.dtw_subseq_batch_dev(
            dq.ptr, len(qq), dr.offset(5 * dim * 4), len(big) - 5, [0, len(q)], [len(q), len(q2)],
            [2, 2 + len(r)], [len(r), len(r2)], dim)
    finally:
        dq.free()
        dr.free()
    _same((cost[0], int(start[0]), int(end[0]), int(ln[0]), pos[0]), want, "first")
    _same((cost[1], int(start[1]), int(end[1]), int(ln[1]), pos[1]), want2, "second")


def test_invalid_arguments_are_refused(engine):
    from audio_sheet_retrieval_amd import _lib
    q = np.ones((1025, 32), np.float32)
    dq, dr = engine.alloc(q.nbytes).upload(q), engine.alloc(q.nbytes).upload(q)
    try:
        bad = [dict(n_q=[1025]), dict(n_q=[0]), dict(r_row=[1000], n_r=[26]), dict(dim=65), dict(q_row=[-1]),
               dict(n_q=[1024], q_row=[2])]
        for kw in bad:
            a = dict(q_row=[0], n_q=[10], r_row=[0], n_r=[20], dim=32)
            a.update(kw)
            with pytest.raises(_lib.AsrError) as e:
                engine.dtw_subseq_batch_dev(dq.ptr, 1025, dr.ptr, 1025, a["q_row"], a["n_q"], a["r_row"], a["n_r"], a["dim"])
            assert e.value.code == _lib.ASR_ERR_INVALID, kw
        one = np.array([0], np.int64), np.array([10], np.int64)
        rc = engine.lib.asr_dtw_subseq_batch_dev(engine.ctx, dq.ptr, 1025, dr.ptr, 1025, one[0].ctypes.data, None,
                                                 one[0].ctypes.data, one[1].ctypes.data, 1, 32, None, None, None, None, None)
        assert rc == _lib.ASR_ERR_INVALID
        # and a valid call with every output NULL, and an empty batch, succeed
        assert engine.lib.asr_dtw_subseq_batch_dev(engine.ctx, dq.ptr, 1025, dr.ptr, 1025, one[0].ctypes.data,
                                                   one[1].ctypes.data, one[0].ctypes.data, one[1].ctypes.data, 1, 32, None,
                                                   None, None, None, None) == _lib.ASR_OK
        assert engine.dtw_subseq_batch([], [], []) == []
    finally:
        dq.free()
        dr.free()


# ---- locate_scores: vote, window codes and the subsequence DTW against the resident data base --------------------
@pytest.fixture(scope="module")
def synthetic(engine):
    """4 synthetic pieces on trained parameters: the pool, its from_pool data base, the driver's excerpts"""
    from audio_sheet_retrieval_amd import audio2sheet_align, audio_sheet_server as drv
    from audio_sheet_retrieval_amd.piece_identification import EmbeddingDB
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(PARAMS) as z:
        engine.set_params([z["p%02d" % i] for i in range(len(param_shapes("mutopia_ccal_cont")))])
    data = audio2sheet_align.select_pieces("synthetic:4", 23)
    pool = AudioScoreRetrievalPool(engine, data["images"], data["specs"], data["o2c_maps"],
                                   data_augmentation=dict(NO_AUGMENT), shuffle=False)
    db = EmbeddingDB.from_pool(engine, pool, 1, names=data["names"])
    excerpts, _ = drv.cut_excerpts(pool.specs, pool.o2c_maps, 400, 2, 42, 23)
    yield data, pool, db, excerpts
    db.close()


def _same_candidates(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [c["name"] for c in g] == [c["name"] for c in w]
        for cg, cw in zip(g, w):
            assert sorted(cg) == sorted(cw) == ["cost", "end_row", "end_x", "name", "start_row", "start_x", "vote_rank",
                                                 "votes", "x"]
            for key in ("votes", "vote_rank", "cost", "start_row", "end_row", "start_x", "end_x"):
                assert cg[key] == cw[key], (cg["name"], key, cg[key], cw[key])
            assert np.array_equal(cg["x"], cw["x"]), cg["name"]


def test_locate_scores_equals_the_host_composition(engine, synthetic):
    from audio_sheet_retrieval_amd import audio_sheet_server as drv, piece_identification as pid
    data, pool, db, excerpts = synthetic
    cols = drv.pool_sheet_columns(pool, len(db))
    assert cols is not None and len(cols) == len(db)
    kw = dict(n_pieces=3, step_spec=2, n_candidates=5, sheet_columns=cols)
    got = pid.locate_scores(engine, db, excerpts, **kw)
    _same_candidates(got, pid.locate_scores_host(engine, db, excerpts, **kw))
    assert len(got) == 4 and all(1 <= len(c) <= 3 for c in got)
    for cands in got:
        assert [c["cost"] for c in cands] == sorted(c["cost"] for c in cands)
        for c in cands:
            first, n = pid.piece_segments(db.ids)[data["names"].index(c["name"])]
            assert 0 <= c["start_row"] <= c["end_row"] < n and len(c["x"]) == 180      # (400 - 42) // 2 + 1 windows
            assert c["start_x"] == cols[first + c["start_row"]] == c["x"][0] and c["end_x"] == cols[first + c["end_row"]]
    # one excerpt alone (locate_score), and the windows embedded in small chunks, give the same
    _same_candidates([pid.locate_score(engine, db, excerpts[2], **kw)], [got[2]])
    _same_candidates(pid.locate_scores(engine, db, excerpts, max_windows=50, **kw), got)


def test_locate_scores_on_a_from_images_data_base(engine, synthetic):
    """default segments and default columns (window k of a piece at k * 50 + 100)"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    data, _, _, excerpts = synthetic
    db = pid.EmbeddingDB.from_images(engine, data["names"], data["images"])
    try:
        kw = dict(n_pieces=2, n_candidates=5)
        got = pid.locate_scores(engine, db, excerpts[:1], **kw)
        _same_candidates(got, pid.locate_scores_host(engine, db, excerpts[:1], **kw))
        for c in got[0]:
            assert c["start_x"] == c["start_row"] * 50 + 100 and c["end_x"] == c["end_row"] * 50 + 100
        with pytest.raises(ValueError, match="not contiguous"):
            shuffled = pid.EmbeddingDB(engine, db.codes, np.roll(db.ids, 1), db.id_to_name)
            try:
                pid.locate_scores(engine, shuffled, excerpts[:1], **kw)
            finally:
                shuffled.close()
    finally:
        db.close()


def test_driver_locate_dumps_one_entry_per_piece(tmp_path, monkeypatch, capsys):
    import pickle
    import yaml
    from audio_sheet_retrieval_amd import audio2sheet_align, audio_sheet_server
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(PARAMS) as z:
        trained = [z["p%02d" % i] for i in range(len(param_shapes("mutopia_ccal_cont")))]
    monkeypatch.setattr(audio2sheet_align, "EXP_ROOT", str(tmp_path))
    d = tmp_path / "mutopia_ccal_cont"
    d.mkdir()
    with open(d / "params_all_split_mutopia_full_aug.pkl", "wb") as fp:
        pickle.dump(trained, fp, protocol=2)
    monkeypatch.chdir(tmp_path)
    res = audio_sheet_server.main(["--model", "models/mutopia_ccal_cont.py", "--data", "synthetic:4", "--train_split",
                                   "splits/all_split.yaml", "--config", "exp_configs/mutopia_full_aug.yaml",
                                   "--init_sheet_db", "--locate", "--dump_results"])
    with open(d / "location_all_split_mutopia_full_aug_A2S.yaml") as fp:
        dumped = yaml.safe_load(fp)
    assert dumped == res and [e["name"] for e in dumped] == ["synthetic_%03d" % i for i in range(4)]
    for e in dumped:
        assert sorted(e) == ["cost_rank", "end_error", "end_x", "name", "start_error", "start_x", "vote_rank"]
        assert 0 <= e["cost_rank"] <= 4 and (e["cost_rank"] == 0) == (e["start_error"] is None)
    out = capsys.readouterr().out
    assert out.count("rank by vote") == 4 and "location of 4 pieces written to" in out
