"""CPU: the audio2sheet_align driver's sampling, dump naming and synthetic pieces, and the first-entry projection."""
import os
import pickle

import numpy as np
import pytest


def test_synthetic_pieces_are_deterministic_and_consistent():
    from audio_sheet_retrieval_amd.utils import synth_data
    a, b = synth_data.synth_pieces(4, seed=5), synth_data.synth_pieces(4, seed=5)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            u, v = (u[0], v[0]) if isinstance(u, list) else (u, v)
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    images, specs, o2c_maps = a
    assert synth_data.synth_piece(2, seed=5)[0].tobytes() == images[2].tobytes()
    assert synth_data.synth_pieces(1, seed=6)[0][0].tobytes() != images[0].tobytes()
    for sheet, (spec,), (o2c,) in zip(images, specs, o2c_maps):
        assert sheet.dtype == np.float32 and sheet.shape[0] == synth_data.PIECE_HEIGHT
        assert sheet.min() >= 0 and sheet.max() <= 255
        assert spec.dtype == np.float32 and spec.shape[0] == synth_data.SPEC_BINS
        assert o2c.dtype == np.int64 and o2c.shape[1] == 2 and len(o2c) >= 32
        assert np.all(np.diff(o2c[:, 0]) > 0) and np.all(np.diff(o2c[:, 1]) > 0)           # monotone map
        assert o2c[:, 1].min() >= 0 and o2c[:, 1].max() < sheet.shape[1]
        assert o2c[:, 0].min() >= 0 and o2c[:, 0].max() < spec.shape[1]
        # every note is a dark blob in the central rows at its x and a bump in the spectrogram at its onset
        r0 = sheet.shape[0] // 2 - 80
        assert all((sheet[r0:r0 + 160, x - 4:x + 4] == 0).any(axis=0).all() for x in o2c[:, 1])
        assert all(spec[:, o].max() >= 2.0 for o in o2c[:, 0])
    # the tempo changes along a piece: frames per pixel are not one constant
    o2c = o2c_maps[0][0]
    rate = np.diff(o2c[:, 0]) / np.diff(o2c[:, 1])
    assert rate.max() > 1.3 * rate.min()


@pytest.mark.parametrize("length", [431, 432, 1999, 2000])
@pytest.mark.parametrize("win,step", [(200, 10), (200, 7), (42, 2), (42, 3)])
def test_sample_points_follow_the_reference_formulas(length, win, step):
    from audio_sheet_retrieval_amd import audio2sheet_align as drv
    idxs, half = drv.sample_points(length, win, step)
    # audio2sheet_align.py:112-120
    n_steps = length // step
    ref = np.linspace(win // 2, length - win // 2, n_steps).astype(np.int32)
    assert half == win // 2 and idxs.dtype == np.int32 and np.array_equal(idxs, ref)
    # windows [x - half, x + half) lie inside the axis and are `win` wide (even widths, as in the models)
    assert np.all(idxs - half >= 0) and np.all(idxs + half <= length)


def test_sheet_window_rows_follow_the_reference():
    """r0 = H//2 - 80 for the 160-row windows (:128), odd and even strip heights"""
    from audio_sheet_retrieval_amd.utils import synth_data
    for h in (180, 181, 160):
        r0 = h // 2 - synth_data.SYSTEM_HEIGHT // 2
        assert r0 == h // 2 - 80 and r0 + 160 <= h


def test_first_entries_equals_the_reference_loop():
    from audio_sheet_retrieval_amd import alignment as al
    from oracle import alignment as oa
    rng = np.random.default_rng(4)
    for _ in range(50):
        n_r, n_c = rng.integers(1, 60, size=2)
        # a random monotone path from (0,0) to (n_r-1, n_c-1) with steps (1,1), (1,0), (0,1)
        i = j = 0
        rows, cols = [0], [0]
        while i < n_r - 1 or j < n_c - 1:
            moves = [m for m in ((1, 1), (1, 0), (0, 1)) if i + m[0] < n_r and j + m[1] < n_c]
            di, dj = moves[rng.integers(len(moves))]
            i, j = i + di, j + dj
            rows.append(i)
            cols.append(j)
        path0, path1 = np.array(cols), np.array(rows)
        loop = [int(np.flatnonzero(path0 == col)[0]) for col in range(n_c)]     # utils/alignment.py:131-138
        assert np.array_equal(al.first_entries(path0, n_c), loop)
        # the same projection the oracle's align_pydtw takes, on a distance matrix whose DTW path is this one
        d = np.ones((n_r, n_c))
        d[path1, path0] = 0.0
        ref = oa.align_pydtw(d)
        p = oa.dtw_by_dist(d)[3]
        assert np.array_equal(np.asarray(p[1])[al.first_entries(p[0], n_c)], ref)


class _StubEngine(object):
    """what the driver asks of an engine, with host arithmetic: no GPU"""


def test_dump_file_name_and_contents(tmp_path, monkeypatch):
    from audio_sheet_retrieval_amd import audio2sheet_align as drv
    assert drv.result_file("/x/m/params_all_split_mutopia_full_aug.pkl", "pydtw") == \
        "/x/m/alignment_res_all_split_mutopia_full_aug_pydtw.pkl"
    assert drv.result_file("/x/m_est_UV/params_a_b.pkl", "baseline") == "/x/m_est_UV/alignment_res_a_b_baseline.pkl"

    # main() end to end with the engine-facing stages stubbed: the dump holds {piece: pxl_errors}
    model_dir = tmp_path / "mutopia_ccal_cont"
    model_dir.mkdir()
    with open(model_dir / "params_all_split_mutopia_full_aug.pkl", "wb") as fp:
        pickle.dump([np.zeros(1, np.float32)], fp)
    monkeypatch.setattr(drv, "EXP_ROOT", str(tmp_path))
    monkeypatch.setattr(drv.network, "set_all_param_values", lambda layers, params: None)

    class _Fn(object):
        engine = _StubEngine()
    monkeypatch.setattr(drv.network, "function", lambda inputs, outputs: _Fn())
    monkeypatch.setattr(drv.network, "get_output", lambda layer, deterministic=True: None)

    class _Pool(object):
        def __init__(self, engine, images, specs, o2c_maps, **kw):
            self.o2c_maps = o2c_maps
    monkeypatch.setattr(drv, "AudioScoreRetrievalPool", _Pool)
    errors = [np.array([1.0, -2.0, 3.5]), np.array([0.0, 4.0])]
    monkeypatch.setattr(drv, "align_pieces", lambda engine, pool, by, s1, s2: (None, None, errors))
    res = drv.main(["--model", "models/mutopia_ccal_cont.py", "--data", "synthetic:2", "--align_by", "pydtw",
                    "--train_split", "splits/all_split.yaml", "--config", "exp_configs/mutopia_full_aug.yaml"])
    out = model_dir / "alignment_res_all_split_mutopia_full_aug_pydtw.pkl"
    assert os.path.exists(out)
    dumped = pickle.load(open(out, "rb"))
    assert sorted(dumped) == ["synthetic_000", "synthetic_001"]
    assert np.array_equal(dumped["synthetic_000"], errors[0]) and np.array_equal(dumped["synthetic_001"], errors[1])
    assert sorted(res) == sorted(dumped)


@pytest.mark.parametrize("flag", ["--plots", "--real_audio"])
def test_unsupported_flags_exit_with_a_message(flag):
    from audio_sheet_retrieval_amd import audio2sheet_align as drv
    with pytest.raises(SystemExit, match="not part of this implementation"):
        drv.main(["--data", "synthetic:1", flag])


def test_other_data_sets_exit_with_a_message():
    from audio_sheet_retrieval_amd import audio2sheet_align as drv
    with pytest.raises(SystemExit, match="only synthetic pieces"):
        drv.select_pieces("mutopia")
