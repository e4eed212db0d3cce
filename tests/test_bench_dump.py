"""CPU: bench.py's step accounting and output dump.  --steps is the number of timed steps in all (the repeats share
them), and --dump-outputs writes float32 / float64 arrays of at most 64 MB, sampling the same seeded rows of every
array beyond that."""
import os

import numpy as np
import pytest

import bench


def test_repeats_share_the_requested_steps():
    for steps, repeats in ((20, 5), (3, 5), (1, 5), (7, 3), (2, 2), (100, 1)):
        sizes = bench._repeat_sizes(steps, repeats)
        assert sum(sizes) == steps and len(sizes) == min(steps, repeats) and max(sizes) - min(sizes) <= 1


def test_dump_option_is_for_the_pairs_workload_only(tmp_path):
    assert bench.parse_args(["--dump-outputs", str(tmp_path)]).dump_outputs == str(tmp_path)
    with pytest.raises(SystemExit):
        bench.parse_args(["--workload", "train", "--dump-outputs", str(tmp_path)])


def test_side_legs_are_behind_full():
    """a plain command line asks for the headline alone; --full is what turns the side legs on, the --no-* switches then
    take single ones out"""
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False and (plain.steps, plain.warmup, plain.gpus) == (20, 5, 1)
    full = bench.parse_args(["--full", "--no-cpu-baseline"])
    assert full.full is True and full.no_cpu_baseline is True and full.no_host_leg is False


def test_dump_writes_float32_and_float64_arrays(tmp_path):
    rng = np.random.default_rng(0)
    lv = rng.standard_normal((10, 32)).astype(np.float32)
    ranks = np.arange(1, 11, dtype=np.int32)
    names = bench.dump_outputs(str(tmp_path), dict(lv1=lv, ranks=ranks, dstar=np.linspace(0, 1, 10)))
    assert names == ["dstar", "lv1", "ranks"]
    a = np.load(os.path.join(tmp_path, "lv1.npy"))
    assert a.dtype == np.float32 and np.array_equal(a, lv)
    r = np.load(os.path.join(tmp_path, "ranks.npy"))
    assert r.dtype == np.float64 and np.array_equal(r, ranks)
    assert bench.dump_outputs(str(tmp_path / "two"), dict(ties=ranks), rank=1, world=2) == ["ties_rank1"]


def test_dump_samples_the_same_rows_beyond_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    n = 1000
    lv = np.arange(n * 32, dtype=np.float32).reshape(n, 32)
    ranks = np.arange(n, dtype=np.int32)
    names = bench.dump_outputs(str(tmp_path / "a"), dict(lv1=lv, ranks=ranks))
    assert names == ["lv1", "ranks", "sample_rows"]
    total = sum(os.path.getsize(os.path.join(tmp_path, "a", f)) - 128 for f in os.listdir(tmp_path / "a"))
    assert total <= 4096
    rows = np.load(os.path.join(tmp_path, "a", "sample_rows.npy")).astype(np.int64)
    assert np.array_equal(np.load(os.path.join(tmp_path, "a", "ranks.npy")), rows)
    assert np.array_equal(np.load(os.path.join(tmp_path, "a", "lv1.npy")), lv[rows])
    bench.dump_outputs(str(tmp_path / "b"), dict(lv1=lv, ranks=ranks))
    assert np.array_equal(np.load(os.path.join(tmp_path, "b", "sample_rows.npy")).astype(np.int64), rows)
