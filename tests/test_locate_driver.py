"""CPU: the host side of excerpt localisation - audio_sheet_server --locate's arguments and report, and
piece_identification's default segments and sheet columns."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_locate_flags_parse():
    from audio_sheet_retrieval_amd import audio_sheet_server as drv
    args = drv._arguments(["--locate", "--excerpt_frames", "300", "--locate_pieces", "3", "--step_spec", "4"], "A2S")
    assert (args.locate, args.excerpt_frames, args.locate_pieces, args.step_spec) == (True, 300, 3, 4)
    dflt = drv._arguments([], "A2S")
    assert (dflt.locate, dflt.excerpt_frames, dflt.locate_pieces, dflt.step_spec) == (False, 400, 5, 2)
    with pytest.raises(SystemExit):                          # A2S only, as --track
        drv._arguments(["--locate"], "S2A")
    assert drv.location_file("/x/m/params_all_split_mutopia_full_aug.pkl", "A2S") == \
        "/x/m/location_all_split_mutopia_full_aug_A2S.yaml"


def test_default_segments():
    from audio_sheet_retrieval_amd import piece_identification as pid
    assert pid.piece_segments([]) == {}
    assert pid.piece_segments([4]) == {4: (0, 1)}
    assert pid.piece_segments(np.array([0, 0, 0, 2, 2, 1], np.int32)) == {0: (0, 3), 2: (3, 2), 1: (5, 1)}
    with pytest.raises(ValueError, match="not contiguous"):
        pid.piece_segments([0, 1, 0])
    with pytest.raises(ValueError, match="not contiguous"):
        pid.piece_segments([3, 3, 1, 1, 3, 2])


def test_default_sheet_columns_follow_from_images():
    """window k of a piece starts at k * (w // 4) (db_window_plan), so its centre is at k * (w // 4) + w // 2"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    shapes, w = [(160, 1000), (160, 430)], 200
    indices, _, ids = pid.db_window_plan(shapes, [0, 160 * 1000], (160, w), True)
    cols = pid.default_sheet_columns(ids, w)
    assert np.array_equal(cols, np.concatenate([idx + w // 2 for idx in indices]))
    assert cols[0] == 100 and cols[1] == 150 and cols[len(indices[0])] == 100
    assert np.array_equal(pid.default_sheet_columns([1, 1, 1], 42), [21, 31, 41])


def test_locate_window_plan():
    from audio_sheet_retrieval_amd import piece_identification as pid
    starts, desc = pid.locate_window_plan([(92, 400), (92, 42), (92, 45)], [0, 92 * 400, 92 * 442], (92, 42), 2)
    assert np.array_equal(starts[0], np.arange(0, 359, 2)) and len(starts[0]) == 180
    assert np.array_equal(starts[1], [0]) and np.array_equal(starts[2], [0, 2])
    assert desc.shape == (183, 9) and desc[180, 0] == 92 * 400 and desc[182, 5] == 2
    with pytest.raises(ValueError, match="a window needs 42"):
        pid.locate_window_plan([(92, 41)], [0], (92, 42), 2)
    with pytest.raises(ValueError, match="at most 1024"):
        pid.locate_window_plan([(92, 42 + 1024)], [0], (92, 42), 1)
    assert len(pid.locate_window_plan([(92, 42 + 1023)], [0], (92, 42), 1)[0][0]) == 1024


def test_excerpts_and_ground_truth():
    from audio_sheet_retrieval_amd import audio_sheet_server as drv
    rng = np.random.default_rng(0)
    specs = [[rng.random((92, 500)).astype(np.float32)], [rng.random((92, 100)).astype(np.float32)]]
    o2c = [[np.array([[0, 10], [499, 10 + 4990]])], [np.array([[0, 0], [99, 990]])]]      # x = 10 + 10 f / x = 10 f
    ex, truth = drv.cut_excerpts(specs, o2c, 400, 2, 42, seed=5)
    assert ex[0].shape == (92, 400) and ex[1].shape == (92, 100)              # a short piece gives all it has
    f0 = int(np.flatnonzero([np.array_equal(specs[0][0][:, f:f + 400], ex[0]) for f in range(101)])[0])
    assert truth[0] == (10 + 10.0 * (f0 + 21), 10 + 10.0 * (f0 + 358 + 21))   # last window starts at 358
    assert truth[1] == (210.0, 10.0 * (58 + 21))
    again, _ = drv.cut_excerpts(specs, o2c, 400, 2, 42, seed=5)
    assert np.array_equal(again[0], ex[0])


def test_locate_reports_and_dumps(tmp_path, monkeypatch, capsys):
    import test_identify_driver as tid
    from audio_sheet_retrieval_amd import audio_sheet_server as drv
    calls = []
    tid._stub(monkeypatch, tmp_path, calls)

    def fake_locate(engine, db, pool, names, n_candidates, excerpt_frames, n_pieces, step_spec, seed):
        calls.append(("locate", len(names), n_candidates, excerpt_frames, n_pieces, step_spec, seed))
        out = [dict(name=n, vote_rank=i + 1, cost_rank=1, start_x=100.0, end_x=900.0, start_error=2.5 * i,
                    end_error=10.0) for i, n in enumerate(names)]
        out[-1].update(vote_rank=0, cost_rank=0, start_x=None, end_x=None, start_error=None, end_error=None)
        return out
    monkeypatch.setattr(drv, "locate", fake_locate)
    common = ["--data", "synthetic:3", "--train_split", "splits/all_split.yaml", "--config",
              "exp_configs/mutopia_full_aug.yaml", "--n_candidates", "9"]
    res = drv.main(common + ["--init_sheet_db", "--locate", "--dump_results", "--excerpt_frames", "300", "--seed", "4"])
    assert calls == [("locate", 3, 9, 300, 5, 2, 4)]
    with open(tmp_path / "mutopia_ccal_cont" / "location_all_split_mutopia_full_aug_A2S.yaml") as fp:
        dumped = yaml.safe_load(fp)
    assert dumped == res and [e["name"] for e in dumped] == ["synthetic_%03d" % i for i in range(3)]
    out = capsys.readouterr().out
    assert "rank by vote 02, by cost 01, start off by    2.5 px, end off by   10.0 px  synthetic_001" in out
    assert "not among the candidates" in out and "own piece first by vote: 1, by cost: 2 of 3" in out


def test_pool_sheet_columns():
    from audio_sheet_retrieval_amd import audio_sheet_server as drv

    class Pool(object):
        shape = [3]
        train_entities = np.array([[0, 0, 1], [0, 0, 2], [1, 0, 0]])
        o2c_maps = [[np.array([[5, 50], [6, 60], [7, 70]])], [np.array([[1, 11]])]]
    assert np.array_equal(drv.pool_sheet_columns(Pool(), 3), [60.0, 70.0, 11.0])
    assert drv.pool_sheet_columns(Pool(), 4) is None
