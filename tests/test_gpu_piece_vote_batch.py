"""GPU: batched piece vote (asr_piece_vote_batch_dev / Engine.piece_vote_batch_dev), the batched detection
(piece_identification.detect_scores / detect_performances), EmbeddingDB.from_pool and the two --full_eval drivers -
bit for bit against asr_piece_vote_dev, the oracle's vote and the per-piece functions."""
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


def _groups(rng, n_groups, per_group, n_db, ids, n_pieces, ties):
    """(n_groups, per_group) int32 indices: random, tie-heavy (2-3 pieces with equal counts), with -1 / out-of-range
    entries and entries whose piece id is out of range; group 0 of a multi-group batch has no valid entry"""
    idx = rng.integers(0, n_db, size=(n_groups, per_group)).astype(np.int32)
    by_piece = {p: np.flatnonzero(ids == p) for p in range(n_pieces)}
    for g in range(n_groups):
        if ties and g % 2 == 1 and per_group >= 6:
            ps = rng.choice([p for p in by_piece if len(by_piece[p])], size=min(3, n_pieces), replace=False)
            m = per_group // len(ps)
            row = np.concatenate([rng.choice(by_piece[p], size=m) for p in ps] + [np.full(per_group - m * len(ps), -1)])
            idx[g] = rng.permutation(row)
        else:
            junk = rng.random(per_group)
            idx[g, junk < 0.05] = -1
            idx[g, (junk >= 0.05) & (junk < 0.07)] = n_db + rng.integers(0, 3)
            idx[g, (junk >= 0.07) & (junk < 0.08)] = -5
    if n_groups > 1:
        idx[0] = -1
    return idx


def _oracle(idx_row, ids, n_db, n_pieces, top_k):
    from oracle import piece_vote as pv
    j = idx_row[(idx_row >= 0) & (idx_row < n_db)]
    p = ids[j]
    return pv.vote(p[(p >= 0) & (p < n_pieces)], top_k)


CASES = [  # n_pieces, per_group, n_groups, lds cap (None: default), tie-heavy
    (1, 1, 1, None, False),
    (7, 2500, 3, None, True),
    (1000, 2500, 1000, None, True),
    (4096, 2500, 3, None, True),                 # the largest LDS-path size
    (5000, 2500, 3, None, True),                 # beyond the LDS path: global counters and keys
    (7, 100000, 3, None, True),                  # per_group far beyond any LDS size (indices are streamed)
    (5000, 100000, 3, None, False),
    (1000, 2500, 5, "4", True),                  # the global path forced at small sizes
    (7, 1, 3, "4", False),
]


@pytest.mark.parametrize("n_pieces,per_group,n_groups,cap,ties", CASES)
def test_batch_vote_equals_single_calls_and_the_oracle(engine, monkeypatch, n_pieces, per_group, n_groups, cap, ties):
    from audio_sheet_retrieval_amd.piece_identification import full_eval_rank
    if cap:
        monkeypatch.setenv("ASR_VOTE_LDS_PIECES", cap)
    rng = np.random.default_rng(n_pieces * 7 + per_group + n_groups)
    n_db = max(3 * n_pieces, 50)
    ids = rng.integers(0, n_pieces, size=n_db).astype(np.int32)
    ids[rng.random(n_db) < 0.02] = n_pieces + 2                  # piece ids outside [0, n_pieces): ignored
    ids[rng.random(n_db) < 0.02] = -3
    idx = _groups(rng, n_groups, per_group, n_db, ids, n_pieces, ties)
    d_idx, d_ids = engine.alloc(idx.nbytes).upload(idx), engine.alloc(ids.nbytes).upload(ids)
    full = [_oracle(idx[g], ids, n_db, n_pieces, n_pieces)[0] for g in range(n_groups)]
    # targets: a voted piece (within or beyond top_k), every third group a random id (often not voted, or invalid)
    targets = np.array([(full[g][g % len(full[g])] if len(full[g]) else 0) if g % 3 else
                        rng.integers(-1, n_pieces + 1) for g in range(n_groups)], np.int32)
    by_k = {}
    try:
        for top_k in sorted({1, 3, n_pieces}):
            refs = [_oracle(idx[g], ids, n_db, n_pieces, top_k) for g in range(n_groups)]
            pieces, counts, n_out, ranks, ratios = by_k[top_k] = engine.piece_vote_batch_dev(
                d_idx.ptr, n_groups, per_group, d_ids.ptr, n_db, n_pieces, top_k, targets=targets)
            assert pieces.shape == (n_groups, top_k) and counts.shape == (n_groups, top_k)
            single_groups = range(n_groups) if n_groups <= 5 else rng.choice(n_groups, 40, replace=False)
            for g in range(n_groups):
                rp, rc, rv = refs[g]
                m = int(n_out[g])
                assert m == len(rp) == min(top_k, len(rp)), (g, top_k)
                assert np.array_equal(pieces[g, :m], rp) and np.array_equal(counts[g, :m], rc), (g, top_k)
                assert np.all(pieces[g, m:] == -1) and np.all(counts[g, m:] == 0)
                assert (int(ranks[g]), float(ratios[g])) == full_eval_rank(list(rp), rv, int(targets[g])), (g, top_k)
            for g in single_groups:                          # asr_piece_vote_dev on the group's slice (top_k <= 1024)
                k1 = min(top_k, 1024)
                sp, sc = engine.piece_vote_dev(d_idx.offset(int(g) * per_group * 4), per_group, d_ids.ptr, n_db,
                                               n_pieces, k1)
                m = min(int(n_out[g]), k1)
                assert np.array_equal(sp, pieces[g, :m]) and np.array_equal(sc, counts[g, :m]), (g, top_k)
            if n_groups > 1:
                assert n_out[0] == 0 and ranks[0] == 0 and ratios[0] == 0.0     # no valid entry
        # without targets: the same votes, no ranks
        p2, c2, n2, r2, q2 = engine.piece_vote_batch_dev(d_idx.ptr, n_groups, per_group, d_ids.ptr, n_db, n_pieces, 3)
        assert r2 is None and q2 is None
        assert np.array_equal(p2, by_k[3][0]) and np.array_equal(c2, by_k[3][1]) and np.array_equal(n2, by_k[3][2])
    finally:
        d_idx.free()
        d_ids.free()


def test_bad_sizes_return_invalid(engine):
    from audio_sheet_retrieval_amd import _lib
    idx = np.zeros(10, np.int32)
    ids = np.zeros(4, np.int32)
    d_idx, d_ids = engine.alloc(idx.nbytes).upload(idx), engine.alloc(ids.nbytes).upload(ids)
    out = np.empty(100, np.int32)
    p = out.ctypes.data
    lib = engine.lib
    bad = [(-1, 5, 1, 1), (2, -1, 1, 1), (2, 5, 0, 1), (2, 5, 1, 0), (2, 5, 1, -3), (2, 5, (1 << 30) + 1, 1)]
    for n_groups, per_group, n_pieces, top_k in bad:
        rc = lib.asr_piece_vote_batch_dev(engine.ctx, d_idx.ptr, n_groups, per_group, d_ids.ptr, 4, n_pieces, top_k,
                                          None, p, p, p, None, None)
        assert rc == _lib.ASR_ERR_INVALID, (n_groups, per_group, n_pieces, top_k)
        assert b"piece_vote_batch" in lib.asr_last_error(engine.ctx)
    t = np.zeros(2, np.int32)
    tp = t.ctypes.data
    for args in ((None, None, p, p, None, None), (None, p, None, p, None, None), (None, p, p, None, None, None),
                 (tp, p, p, p, None, p), (tp, p, p, p, p, None)):
        rc = lib.asr_piece_vote_batch_dev(engine.ctx, d_idx.ptr, 2, 5, d_ids.ptr, 4, 1, 1, *args)
        assert rc == _lib.ASR_ERR_INVALID
    rc = lib.asr_piece_vote_batch_dev(engine.ctx, None, 2, 5, d_ids.ptr, 4, 1, 1, None, p, p, p, None, None)
    assert rc == _lib.ASR_ERR_INVALID
    with pytest.raises(_lib.AsrError, match="piece_vote_batch"):
        engine.piece_vote_batch_dev(d_idx.ptr, 2, 5, d_ids.ptr, 4, 0, 1)
    pieces, counts, n_out, _, _ = engine.piece_vote_batch_dev(d_idx.ptr, 2, 5, d_ids.ptr, 4, 1, 2)   # still works
    assert pieces.tolist() == [[0, -1], [0, -1]] and counts.tolist() == [[5, 0], [5, 0]] and n_out.tolist() == [1, 1]
    d_idx.free()
    d_ids.free()


@pytest.fixture(scope="module")
def trained():
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        return [z["p%02d" % i] for i in range(len(param_shapes(MODEL)))]


def _random_db(engine, rng, n_db, n_pieces):
    from audio_sheet_retrieval_amd import piece_identification as pid
    codes = rng.standard_normal((n_db, 32)).astype(np.float32)
    ids = np.sort(rng.integers(0, n_pieces, size=n_db))
    return pid.EmbeddingDB(engine, codes, ids, {i: "piece_%02d" % i for i in range(n_pieces)})


def test_detect_scores_and_performances_equal_the_single_query_functions(engine, trained):
    from audio_sheet_retrieval_amd import piece_identification as pid
    engine.set_params(trained)
    rng = np.random.default_rng(8)
    n_pieces = 11
    sheet_db, audio_db = _random_db(engine, rng, 700, n_pieces), _random_db(engine, rng, 500, n_pieces)
    specs = [(3.0 * rng.random((92, T)) ** 2).astype(np.float32) for T in (42, 43, 400, 977)]
    sheets = [np.floor(255 * rng.random((r, T))).astype(np.float32) for r, T in ((160, 200), (180, 201), (181, 700))]
    for batch, single, db, inputs in ((pid.detect_scores, pid.detect_score, sheet_db, specs),
                                      (pid.detect_performances, pid.detect_performance, audio_db, sheets)):
        for top_k, n_cand, n_samples in ((3, 5, 20), (n_pieces, 25, 30)):
            ref = [single(engine, db, x, top_k=top_k, n_candidates=n_cand, n_samples=n_samples) for x in inputs]
            targets = np.arange(len(inputs), dtype=np.int32) * 3 % n_pieces
            res, ranks, ratios = batch(engine, db, inputs, top_k=top_k, n_candidates=n_cand, n_samples=n_samples,
                                       targets=targets)
            chunked = batch(engine, db, inputs, top_k=top_k, n_candidates=n_cand, n_samples=n_samples,
                            max_windows=7)
            for k, ((names, votes), (rn, rv), (cn, cv)) in enumerate(zip(ref, res, chunked)):
                assert names == rn == cn, (batch.__name__, k)
                assert votes.dtype == rv.dtype == cv.dtype == np.float64
                assert votes.tobytes() == rv.tobytes() == cv.tobytes(), (batch.__name__, k)
                want = pid.full_eval_rank(names, votes, "piece_%02d" % targets[k])
                assert (int(ranks[k]), float(ratios[k])) == want, (batch.__name__, k)
    sheet_db.close()
    audio_db.close()


@pytest.mark.parametrize("view", [1, 2])
def test_from_pool_equals_embedding_the_pool_windows(engine, trained, view):
    from audio_sheet_retrieval_amd import piece_identification as pid
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    engine.set_params(trained)
    images, specs, o2c_maps = synth_data.synth_pieces(3, seed=4)
    pool = AudioScoreRetrievalPool(engine, images, specs, o2c_maps, data_augmentation=dict(NO_AUGMENT), shuffle=False)
    names = ["a", "b", "c"]
    np.random.seed(11)
    db = pid.EmbeddingDB.from_pool(engine, pool, view, names=names)
    after = np.random.random_sample()
    np.random.seed(11)
    np.random.random_sample(pool.shape[0])                   # the reference: one sheet_scaling draw per sample
    assert np.random.random_sample() == after
    sheet, spec = pool[:]
    ref = engine.embed_view1(sheet, prepared=False) if view == 1 else engine.embed_view2(spec)
    assert db.codes.tobytes() == ref.tobytes()
    assert np.array_equal(db.ids, pool.train_entities[:, 0]) and set(db.ids.tolist()) == {0, 1, 2}
    assert np.all(np.diff(db.ids) >= 0)                       # piece after piece, as the per-piece pools list them
    assert db.id_to_name == {0: "a", 1: "b", 2: "c"}
    assert db.snippets.dtype == np.uint8 and db.snippets.shape == ((0, 80, 100) if view == 1 else (0, 46, 21))
    chunked = pid.EmbeddingDB.from_pool(engine, pool, view, names=names, max_windows=13)
    assert chunked.codes.tobytes() == db.codes.tobytes()
    db.close()
    chunked.close()


# ---- the drivers ---------------------------------------------------------------------------------------------------
TAG = "all_split_mutopia_full_aug"


@pytest.mark.parametrize("direction", ["A2S", "S2A"])
def test_driver_full_eval_equals_the_per_piece_loop(tmp_path, monkeypatch, trained, direction):
    from audio_sheet_retrieval_amd import (_lib, audio2sheet_align, audio_sheet_server, piece_identification as pid,
                                           sheet_audio_server)
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    monkeypatch.setattr(audio2sheet_align, "EXP_ROOT", str(tmp_path))
    d = tmp_path / MODEL
    d.mkdir()
    with open(d / ("params_%s.pkl" % TAG), "wb") as fp:
        pickle.dump(trained, fp, protocol=2)
    monkeypatch.chdir(tmp_path)
    main = audio_sheet_server.main if direction == "A2S" else sheet_audio_server.main
    flag, db_file = (("--init_sheet_db", "sheet_db_file.pkl") if direction == "A2S" else
                     ("--init_audio_db", "audio_db_file.pkl"))
    argv = ["--model", "models/%s.py" % MODEL, "--data", "synthetic:8", "--train_split", "splits/all_split.yaml",
            "--config", "exp_configs/mutopia_full_aug.yaml", "--full_eval", "--dump_results"]
    first = main(argv + [flag])
    out = d / ("retrieval_%s_%s.yaml" % (TAG, direction))
    with open(out) as fp:
        dumped = yaml.safe_load(fp)
    assert dumped == first and len(first) == 8

    # the per-piece loop: the same data base, detect_score / detect_performance per piece, the reference's rank rule
    eng = _lib.Engine(MODEL)
    eng.set_params(trained)
    images, specs, o2c_maps = synth_data.synth_pieces(8)
    names = ["synthetic_%03d" % i for i in range(8)]
    pool = AudioScoreRetrievalPool(eng, images, specs, o2c_maps, data_augmentation=dict(NO_AUGMENT), shuffle=False)
    db = pid.EmbeddingDB.from_pool(eng, pool, 1 if direction == "A2S" else 2, names=names)
    saved = pid.EmbeddingDB.load(eng, str(tmp_path / db_file))
    assert saved.codes.tobytes() == db.codes.tobytes() and np.array_equal(saved.ids, db.ids)
    assert saved.id_to_name == db.id_to_name
    loop = []
    for i, name in enumerate(names):
        if direction == "A2S":
            rn, rv = pid.detect_score(eng, db, specs[i][0], top_k=8, n_candidates=25)
        else:
            rn, rv = pid.detect_performance(eng, db, images[i], top_k=8, n_candidates=25)
        loop.append(pid.full_eval_rank(rn, rv, name)[0])
    assert dumped == loop
    saved.close()
    db.close()
    eng.close()

    # a second run loads the data base file and writes the same ranks
    os.remove(out)
    assert main(argv) == first
    with open(out) as fp:
        assert yaml.safe_load(fp) == dumped
