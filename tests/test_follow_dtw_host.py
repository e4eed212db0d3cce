"""CPU: alignment.follow_dtw_host, the numpy restatement of asr_dtw_follow_batch_dev's definition, against
alignment.subseq_dtw_host on every prefix of the stream; the window bookkeeping of ScoreFollower; the --follow mode of
audio_sheet_server with stubbed library calls."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _codes(rng, n, dim, distinct=0):
    """n code rows; distinct > 0: drawn from that many rows, so that distances and accumulated costs tie"""
    if distinct:
        return rng.standard_normal((distinct, dim)).astype(np.float32)[rng.integers(0, distinct, n)]
    return rng.standard_normal((n, dim)).astype(np.float32)


CASES = [(1, 1, 1, 0), (1, 9, 32, 0), (9, 1, 31, 0), (7, 80, 33, 0), (60, 80, 64, 0), (33, 17, 32, 0), (40, 60, 1, 0),
         (25, 40, 32, 2), (60, 31, 31, 3), (48, 64, 64, 4), (30, 30, 33, 2), (12, 5, 1, 2)]


def _dists(case, seed):
    from audio_sheet_retrieval_amd import alignment
    Q, S, dim, distinct = case
    rng = np.random.default_rng(seed)
    return alignment.cosine_dists_host(_codes(rng, Q, dim, distinct), _codes(rng, S, dim, distinct))


def _in_blocks(D, cuts):
    from audio_sheet_retrieval_amd import alignment
    state, outs = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        cost, start, pos, state = alignment.follow_dtw_host(D[a:b], state)
        outs.append((cost, start, pos))
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(3)) + (state,)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_d%d_t%d" % c)
def test_every_row_is_the_subsequence_dtw_of_its_prefix(case):
    from audio_sheet_retrieval_amd import alignment
    D = _dists(case, 11)
    cost, start, pos, state = alignment.follow_dtw_host(D)
    assert cost.dtype == np.float64 and start.dtype == np.int32 and pos.dtype == np.int32
    for i in range(D.shape[0]):
        c, s, e, _ = alignment.subseq_dtw_host(D[:i + 1])
        assert (cost[i], int(start[i]), int(pos[i])) == (c, s, e), i
    assert state[2] == D.shape[0] and state[0].shape == state[1].shape == (D.shape[1],)
    assert state[0][pos[-1]] / D.shape[0] == cost[-1] and state[1][pos[-1]] == start[-1]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_d%d_t%d" % c)
def test_any_cut_into_blocks_gives_the_same_bits(case):
    D = _dists(case, 12)
    Q = D.shape[0]
    whole = _in_blocks(D, [0, Q])
    rng = np.random.default_rng(Q)
    cuttings = [list(range(Q + 1))]                                       # row by row
    for _ in range(3):
        cuts, at = [0], 0
        while at < Q:
            at = min(Q, at + int(rng.integers(1, 8)))
            cuts.append(at)
        cuttings.append(cuts)
    for cuts in cuttings:
        got = _in_blocks(D, cuts)
        for k in range(3):
            assert np.array_equal(got[k], whole[k]), (cuts, k)
        assert np.array_equal(got[3][0], whole[3][0]) and np.array_equal(got[3][1], whole[3][1])
        assert got[3][2] == whole[3][2] == Q


def test_host_rejects_bad_shapes():
    from audio_sheet_retrieval_amd import alignment
    with pytest.raises(ValueError):
        alignment.follow_dtw_host(np.zeros((0, 3)))
    with pytest.raises(ValueError):
        alignment.follow_dtw_host(np.zeros((2, 3)), (np.zeros(4), np.zeros(4, np.int32), 2))
    # a state of zero rows is a fresh stream: its arrays are not read
    D = np.arange(6.0).reshape(2, 3)
    a = alignment.follow_dtw_host(D, (np.full(3, np.nan), np.zeros(3, np.int32), 0))
    b = alignment.follow_dtw_host(D)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_the_large_case_is_vectorised():
    """1024 x 1100, the largest block of the device tests, in well under their time"""
    import time
    from audio_sheet_retrieval_amd import alignment
    D = np.random.default_rng(0).random((1024, 1100))
    t0 = time.perf_counter()
    cost, start, pos, _ = alignment.follow_dtw_host(D)
    assert time.perf_counter() - t0 < 20.0
    c, s, e, _ = alignment.subseq_dtw_host(D)
    assert (cost[-1], start[-1], pos[-1]) == (c, s, e)


def test_the_call_is_exported():
    from audio_sheet_retrieval_amd import _lib
    assert "asr_dtw_follow_batch_dev" in _lib.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "asr_hip.h")).read()
    assert "int asr_dtw_follow_batch_dev(asr_ctx *ctx" in header


# ---- the window bookkeeping of ScoreFollower -------------------------------------------------------------------------
def test_follow_window_plan():
    from audio_sheet_retrieval_amd import piece_identification as pid
    st, carry = pid.follow_window_plan(0, 41, 42, 2)
    assert len(st) == 0 and carry == 0                       # no window yet: everything is carried
    st, carry = pid.follow_window_plan(41, 1, 42, 2)
    assert np.array_equal(st, [0]) and carry == 2
    st, carry = pid.follow_window_plan(42, 5, 42, 2)         # columns 42..46: windows at 2 and 4 end at 44 and 46
    assert np.array_equal(st, [2, 4]) and carry == 6
    st, carry = pid.follow_window_plan(0, 1066, 42, 1)
    assert np.array_equal(st, np.arange(1025)) and carry == 1025          # no limit of 1024 windows
    st, carry = pid.follow_window_plan(0, 100, 42, 200)      # the next window starts past the end: nothing to carry
    assert np.array_equal(st, [0]) and carry == 100
    st, carry = pid.follow_window_plan(100, 300, 42, 200)
    assert np.array_equal(st, [200]) and carry == 400
    with pytest.raises(ValueError):
        pid.follow_window_plan(0, 5, 42, 0)


@pytest.mark.parametrize("step", [1, 2, 5, 50])
def test_any_block_cut_completes_the_same_windows(step):
    """the windows of a stream are those of the whole recording, each completed exactly once, and what is carried always
    holds the next window's columns"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    T, w = 333, 42
    whole = np.arange(0, T - w + 1, step)
    rng = np.random.default_rng(step)
    for hi in (2, 9, 60, 400):
        n, col0, got = 0, 0, []
        while n < T:
            b = min(T - n, int(rng.integers(1, hi)))
            st, carry = pid.follow_window_plan(n, b, w, step)
            assert (st >= col0).all() and (st + w <= n + b).all()         # inside carried + new columns
            assert col0 <= carry <= n + b
            got.append(st)
            n, col0 = n + b, carry
        assert np.array_equal(np.concatenate(got), whole)


# ---- audio_sheet_server --follow ---------------------------------------------------------------------------------------
def test_follow_flags_parse():
    from audio_sheet_retrieval_amd import audio_sheet_server as drv
    args = drv._arguments(["--follow", "--block_frames", "7", "--locate_pieces", "3", "--step_spec", "4"], "A2S")
    assert (args.follow, args.block_frames, args.locate_pieces, args.step_spec) == (True, 7, 3, 4)
    dflt = drv._arguments([], "A2S")
    assert (dflt.follow, dflt.block_frames) == (False, 20)
    with pytest.raises(SystemExit):                          # A2S only, as --track and --locate
        drv._arguments(["--follow"], "S2A")
    assert drv.following_file("/x/m/params_all_split_mutopia_full_aug.pkl", "A2S") == \
        "/x/m/following_all_split_mutopia_full_aug_A2S.yaml"


def test_follow_streams_blocks_and_scores_against_the_onset_map(monkeypatch):
    """drv.follow with a stubbed vote and session: block cut, truth at the window centres, share and median"""
    from audio_sheet_retrieval_amd import audio_sheet_server as drv
    from audio_sheet_retrieval_amd import piece_identification as pid
    pushed = []

    class Pool(object):
        spec_dim = [92, 42]
        shape = [0]
        specs = [[np.zeros((92, 100), np.float32)], [np.zeros((92, 50), np.float32)]]
        o2c_maps = [[np.array([[0, 0], [99, 990]])], [np.array([[0, 5], [49, 495]])]]          # x = 10 f / 5 + 10 f

    class Session(object):
        def __init__(self, engine, db, pieces, step_spec, spec_shape, sheet_columns):
            self.pieces, self.step, self.n, self.w = list(pieces), step_spec, 0, spec_shape[1]
            assert sheet_columns is None                      # the pool does not describe this data base

        def push(self, cols):
            pushed.append(cols.shape[1])
            st, _ = pid.follow_window_plan(self.n, cols.shape[1], self.w, self.step)
            self.n += cols.shape[1]
            m, C = len(st), len(self.pieces)
            x = np.zeros((m, C))
            x[:, 0] = 10.0 * (st + 21) + 3.0                  # candidate 0 is 3 px off piece a's truth
            cost = np.ones((m, C))
            cost[:, 0] = np.where((st // self.step) % 2 == 0, 0.5, 2.0)   # and has the least cost at every other window
            return pid.FollowResult(st, cost, np.zeros((m, C), np.int32), np.zeros((m, C), np.int32), x, x, self.pieces,
                                    self.pieces)

        def close(self):
            pushed.append("closed")

    class DB(object):
        def __len__(self):
            return 7
    monkeypatch.setattr(drv, "ScoreFollower", Session)
    monkeypatch.setattr(drv, "detect_scores", lambda engine, db, specs, top_k, n_candidates, spec_shape:
                        [(["a", "b"][:top_k], None), (["a"], None)])
    out = drv.follow(object(), DB(), Pool(), ["a", "b"], 9, 2, 2, 30)
    assert pushed == [30, 30, 30, 10, "closed", 30, 20, "closed"]
    assert out[0] == dict(name="a", candidate=True, windows=30, best_share=0.5, median_error=3.0)
    assert out[1] == dict(name="b", candidate=False, windows=5, best_share=0.0, median_error=None)


def test_follow_reports_and_dumps(tmp_path, monkeypatch, capsys):
    import test_identify_driver as tid
    from audio_sheet_retrieval_amd import audio_sheet_server as drv
    calls = []
    tid._stub(monkeypatch, tmp_path, calls)

    def fake_follow(engine, db, pool, names, n_candidates, n_pieces, step_spec, block_frames):
        calls.append(("follow", len(names), n_candidates, n_pieces, step_spec, block_frames))
        out = [dict(name=n, candidate=True, windows=100 + i, best_share=0.25 * (i + 1), median_error=4.0 * i)
               for i, n in enumerate(names)]
        out[-1].update(candidate=False, best_share=0.0, median_error=None)
        return out
    monkeypatch.setattr(drv, "follow", fake_follow)
    common = ["--data", "synthetic:3", "--train_split", "splits/all_split.yaml", "--config",
              "exp_configs/mutopia_full_aug.yaml", "--n_candidates", "9"]
    res = drv.main(common + ["--init_sheet_db", "--follow", "--dump_results", "--block_frames", "8", "--locate_pieces", "4"])
    assert calls == [("follow", 3, 9, 4, 2, 8)]
    with open(tmp_path / "mutopia_ccal_cont" / "following_all_split_mutopia_full_aug_A2S.yaml") as fp:
        dumped = yaml.safe_load(fp)
    assert dumped == res and [e["name"] for e in dumped] == ["synthetic_%03d" % i for i in range(3)]
    out = capsys.readouterr().out
    assert "least cost at 0.50 of   101 windows, median off by    4.0 px  synthetic_001" in out
    assert "not among the candidates" in out and "own piece a candidate: 2 of 3" in out
    # none of the modes: the exit message of the other drivers' tests is unchanged
    with pytest.raises(SystemExit, match="use --full_eval"):
        drv.main(common)
