"""CPU: the piece-identification drivers (audio_sheet_server / sheet_audio_server --full_eval): dump names, the
reference's rank rule and summary, the batched path's window plan, and main() end to end with the engine stages
stubbed."""
import os
import pickle

import numpy as np
import pytest
import yaml


def _reference_rank(ret_result, ret_votes, tp):
    """audio_sheet_server.py:640-645 / sheet_audio_server.py:85-90, restated line for line"""
    if tp in ret_result:
        rank = ret_result.index(tp) + 1
        ratio = ret_votes[ret_result.index(tp)]
    else:
        rank = len(ret_result)
        ratio = 0.0
    return rank, ratio


def test_dump_file_names():
    from audio_sheet_retrieval_amd import audio_sheet_server as drv
    assert drv.result_file("/x/m/params_all_split_mutopia_full_aug.pkl", "A2S") == \
        "/x/m/retrieval_all_split_mutopia_full_aug_A2S.yaml"
    assert drv.result_file("/x/m_est_UV/params_a_b.pkl", "S2A") == "/x/m_est_UV/retrieval_a_b_S2A.yaml"
    # the reference's replace on a tag-less dump: "params_" does not occur, so the stem stays
    assert drv.result_file("/x/m/params.pkl", "A2S") == "/x/m/params_A2S.yaml"
    ref = "/x/m/params.pkl".replace("params_", "retrieval_").replace(".pkl", "_%s.yaml") % "S2A"
    assert drv.result_file("/x/m/params.pkl", "S2A") == ref


def test_rank_rule_equals_the_reference_lines():
    from audio_sheet_retrieval_amd.piece_identification import full_eval_rank
    from oracle import piece_vote as pv
    ids = [4, 4, 4, 9, 9, 1, 7, 7, 7, 7, 2]
    pieces, _, votes = pv.vote(ids, top_k=3)                      # [7, 4, 9]: 1 and 2 voted but cut by top_k
    names = ["p%d" % p for p in pieces]
    for target in ("p7", "p4", "p9",                              # present
                   "p1", "p2",                                    # voted, beyond top_k
                   "p5"):                                         # absent
        got = full_eval_rank(names, votes, target)
        want = _reference_rank(names, votes, target)
        assert got == want and type(got[1]) is float, target
    assert full_eval_rank(names, votes, "p4") == (2, 3.0 / 9.0)
    assert full_eval_rank(names, votes, "p1") == (3, 0.0)
    assert full_eval_rank([], np.zeros(0), "p1") == (0, 0.0) == _reference_rank([], [], "p1")   # no votes


def test_rank_summary_equals_eval_piece_retrieval():
    from audio_sheet_retrieval_amd.piece_identification import rank_summary
    rng = np.random.default_rng(3)
    for ranks in (rng.integers(1, 30, size=57), [1, 1, 2, 5, 6, 10, 11], [12], [1]):
        # scripts/eval_piece_retrieval.py:63-70
        r = np.sort(ranks)
        want = []
        for thr in [1, 5, 10]:
            cnt = float(np.sum(r <= thr))
            want.append("%d (%.2f)" % (cnt, (cnt / len(r))))
        cnt = float(np.sum(r > thr))
        want.append("%d (%.2f)" % (cnt, (cnt / len(r))))
        got = rank_summary(ranks)
        assert list(got) == ["<=1", "<=5", "<=10", ">10"]
        assert ["%d (%.2f)" % v for v in got.values()] == want
        assert all(v[1] == v[0] / float(len(r)) for v in got.values())


@pytest.mark.parametrize("centre", [False, True])
def test_window_plan_starts_and_gather_equal_the_reference_slices(centre):
    from audio_sheet_retrieval_amd.piece_identification import window_plan
    from oracle import piece_vote as pv
    rng = np.random.default_rng(5)
    win = (160, 200) if centre else (92, 42)
    rows = (180, 181, 160) if centre else (92, 92, 92)
    lengths = (win[1], win[1] + 1, 977)
    srcs = [rng.random((r, T)).astype(np.float32) for r, T in zip(rows, lengths)]
    flat, starts, desc = window_plan(srcs, win, 20, centre)
    assert desc.shape == (60, 9) and flat.size == sum(s.size for s in srcs)
    for i, src in enumerate(srcs):
        assert starts[i].dtype == np.int32
        assert np.array_equal(starts[i], pv.window_starts(src.shape[1], win[1], 20)), i
        r0 = src.shape[0] // 2 - win[0] // 2 if centre else 0
        ref = pv.slice_windows(src, r0, win[0], win[1], starts[i])
        # gather_windows_kernel's formula on these descriptors (utils/data_pools: out[y, x] = src[off + clamp(floor(
        # (y0 + y) * sy), 0, ymax) * stride + xadd + clamp(floor((x0 + x) * sx), 0, xmax)])
        for k in (0, 7, 19):
            d = desc[i * 20 + k]
            yy = np.clip(np.floor((d[2] + np.arange(win[0])) * d[3]), 0, d[4]).astype(np.int64)
            xx = np.clip(np.floor((d[5] + np.arange(win[1])) * d[6]), 0, d[7]).astype(np.int64)
            got = flat[int(d[0]) + yy[:, None] * int(d[1]) + int(d[8]) + xx[None, :]]
            assert np.array_equal(got, ref[k, 0]), (i, k)


def test_inputs_are_checked_before_anything_is_enqueued():
    from audio_sheet_retrieval_amd import piece_identification as pid

    class _NoDevice(object):
        def __getattr__(self, name):
            raise AssertionError("engine.%s used before the inputs were checked" % name)

    good = np.zeros((92, 100), np.float32)
    for bad, msg in ((np.zeros((92, 41), np.float32), "columns"), (np.zeros((91, 100), np.float32), "rows"),
                     (np.zeros(100, np.float32), "2-d")):
        with pytest.raises(ValueError, match=msg):
            pid.detect_scores(_NoDevice(), None, [good, bad, good], top_k=3)
    with pytest.raises(ValueError, match="rows"):
        pid.detect_performances(_NoDevice(), None, [np.zeros((159, 300), np.float32)])
    with pytest.raises(ValueError, match="targets"):
        pid.detect_scores(_NoDevice(), None, [good], targets=[0, 1])


# ---- main() with the engine stages stubbed ---------------------------------------------------------------------
class _FakeDB(object):
    saved = []

    def __init__(self, id_to_name):
        self.id_to_name = dict(id_to_name)

    @classmethod
    def from_pool(cls, engine, pool, view, names=None):
        db = cls({i: n for i, n in enumerate(names)})
        db.view = view
        return db

    @classmethod
    def load(cls, engine, path):
        with open(path, "rb") as fp:
            return cls(pickle.load(fp))

    def save(self, path):
        _FakeDB.saved.append((path, self.view))
        with open(path, "wb") as fp:
            pickle.dump(self.id_to_name, fp)

    def __len__(self):
        return len(self.id_to_name)


def _stub(monkeypatch, tmp_path, calls):
    from audio_sheet_retrieval_amd import audio2sheet_align, audio_sheet_server as drv
    param_file = str(tmp_path / "mutopia_ccal_cont" / "params_all_split_mutopia_full_aug.pkl")
    monkeypatch.setattr(audio2sheet_align, "load_network", lambda *a: (object(), param_file))

    class _Pool(object):
        def __init__(self, engine, images, specs, o2c_maps, **kw):
            self.images, self.specs = images, specs
            self.spec_dim, self.sheet_dim = [92, 42], [160, 200]
    monkeypatch.setattr(drv, "AudioScoreRetrievalPool", _Pool)
    monkeypatch.setattr(drv, "EmbeddingDB", _FakeDB)

    def fake_detect(kind):
        def detect(engine, db, queries, top_k, n_candidates, targets, **kw):
            calls.append((kind, len(queries), top_k, n_candidates, list(targets)))
            # piece i ranks at (i % 3) + 1: ranks 1, 2, 3, 1, ...
            ranks = np.array([(i % 3) + 1 for i in range(len(queries))], np.int32)
            return [None] * len(queries), ranks, 1.0 / ranks
        return detect
    monkeypatch.setattr(drv, "detect_scores", fake_detect("scores"))
    monkeypatch.setattr(drv, "detect_performances", fake_detect("performances"))
    (tmp_path / "mutopia_ccal_cont").mkdir()
    monkeypatch.chdir(tmp_path)
    return param_file


@pytest.mark.parametrize("direction", ["A2S", "S2A"])
def test_main_builds_saves_loads_and_dumps(tmp_path, monkeypatch, capsys, direction):
    from audio_sheet_retrieval_amd import audio_sheet_server, sheet_audio_server
    calls = []
    _stub(monkeypatch, tmp_path, calls)
    main = audio_sheet_server.main if direction == "A2S" else sheet_audio_server.main
    flag, db_file = (("--init_sheet_db", "sheet_db_file.pkl") if direction == "A2S" else
                     ("--init_audio_db", "audio_db_file.pkl"))
    common = ["--model", "models/mutopia_ccal_cont.py", "--data", "synthetic:4", "--train_split",
              "splits/all_split.yaml", "--config", "exp_configs/mutopia_full_aug.yaml", "--n_candidates", "7"]
    _FakeDB.saved = []
    ranks = main(common + [flag, "--full_eval", "--dump_results"])
    assert ranks == [1, 2, 3, 1]
    assert _FakeDB.saved == [(db_file, 1 if direction == "A2S" else 2)] and os.path.exists(tmp_path / db_file)
    kind = "scores" if direction == "A2S" else "performances"
    names = ["synthetic_%03d" % i for i in range(4)]
    assert calls == [(kind, 4, 4, 7, [0, 1, 2, 3])]          # top_k = number of test pieces; targets = piece ids
    out = tmp_path / "mutopia_ccal_cont" / ("retrieval_all_split_mutopia_full_aug_%s.yaml" % direction)
    with open(out) as fp:
        assert yaml.safe_load(fp) == [1, 2, 3, 1]
    text = capsys.readouterr().out
    assert "rank: 01 (1.00) synthetic_000" in text and "rank: 03 (0.33) synthetic_002" in text
    assert "2 of 4 retrieved %s ranked at position 1." % kind in text
    assert "1 of 4 retrieved %s ranked at position 3." % kind in text

    # a later run without the flag loads the file (here: with the piece names reversed, so the targets follow it)
    with open(tmp_path / db_file, "wb") as fp:
        pickle.dump({i: n for i, n in enumerate(names[::-1])}, fp)
    os.remove(out)
    _FakeDB.saved, calls[:] = [], []
    assert main(common + ["--full_eval"]) == [1, 2, 3, 1]
    assert _FakeDB.saved == [] and calls == [(kind, 4, 4, 7, [3, 2, 1, 0])]
    assert not os.path.exists(out)                           # no --dump_results


def test_unsupported_modes_exit_with_their_messages(tmp_path, monkeypatch):
    from audio_sheet_retrieval_amd import audio_sheet_server, sheet_audio_server
    _stub(monkeypatch, tmp_path, [])
    with pytest.raises(SystemExit, match="not part of this implementation"):
        audio_sheet_server.main(["--data", "synthetic:1", "--real_audio", "--full_eval"])
    with pytest.raises(SystemExit):                          # S2A has no --real_audio, as in the reference
        sheet_audio_server.main(["--data", "synthetic:1", "--real_audio"])
    for main in (audio_sheet_server.main, sheet_audio_server.main):
        with pytest.raises(SystemExit, match="only synthetic pieces"):
            main(["--data", "mutopia", "--full_eval"])
    # without --full_eval the reference runs its live server after building the data base: not here
    with pytest.raises(SystemExit, match="live server loop"):
        audio_sheet_server.main(["--data", "synthetic:2", "--init_sheet_db"])
    assert os.path.exists(tmp_path / "sheet_db_file.pkl")
    with pytest.raises(SystemExit, match="live server loop"):
        sheet_audio_server.main(["--data", "synthetic:2", "--init_audio_db", "--running_frames", "50"])
