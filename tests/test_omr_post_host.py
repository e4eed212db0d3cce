"""CPU: the host side of asr_systems_from_maps_dev - the restated summation orders that the kernels keep
(sheet_utils/omr.py pairwise_sum / row_sums / column_sums against numpy, bit for bit), the declaration and the Python
surface, and the wrapper's checks that come before any library call."""
import os
import re

import numpy as np
import pytest

WIDTHS = [5, 8, 100, 128, 129, 300, 512, 835, 1030, 1181, 2000, 2479]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_row_sum_order_is_numpys(dtype):
    from audio_sheet_retrieval_amd.sheet_utils.omr import row_sums
    rng = np.random.default_rng(5)
    for w in WIDTHS:
        x = (rng.random((6, w)) * 3.0 - 1.0).astype(dtype)
        x[0] = rng.random(w).astype(dtype)                    # a probability-like row
        got, ref = row_sums(x), x.sum(1)
        assert got.dtype == ref.dtype
        assert np.array_equal(got, ref), (dtype, w, got - ref)
        if dtype == np.float32:                               # imagey.mean(axis=1) of the snap
            assert np.array_equal(got / np.float32(w), x.mean(axis=1)), w


def test_column_sum_order_is_numpys():
    from audio_sheet_retrieval_amd.sheet_utils.omr import column_sums
    rng = np.random.default_rng(6)
    x = rng.random((300, 835)).astype(np.float32)
    for r0, r1 in [(0, 1), (3, 29), (10, 170), (0, 300)]:
        got = column_sums(x[r0:r1])
        assert np.array_equal(got, x[r0:r1].sum(0)), (r0, r1)
        assert np.array_equal(got / np.float32(r1 - r0), x[r0:r1].mean(axis=0)), (r0, r1)


def test_entry_point_is_declared_and_bound(repo_root):
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import omr
    text = open(os.path.join(repo_root, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(asr_[a-z0-9_]+)\s*\(", text))
    assert "asr_systems_from_maps_dev" in declared
    assert "asr_systems_from_maps_dev" in _lib.EXPORTS
    assert callable(getattr(_lib.Engine, "systems_from_maps_dev"))
    assert callable(getattr(omr.OpticalMusicRecognizer, "detect_systems_pages_dev"))
    assert callable(getattr(omr.SegmentationNetwork, "predict_pages_dev"))
    import inspect
    from audio_sheet_retrieval_amd.sheet_utils import umc
    assert inspect.signature(umc.load_umc_sheets).parameters["device_post"].default is False
    lib = _lib.load_library()
    assert hasattr(lib, "asr_systems_from_maps_dev")


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def _bare_engine():
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib, eng.ctx = _NoLibrary(), None
    return eng


def test_wrapper_rejects_small_capacity_before_any_call():
    eng = _bare_engine()
    hs, ws = np.asarray([1181, 600], np.int32), np.asarray([835, 500], np.int32)
    offs = np.asarray([0, 1181 * 835], np.int64)
    need = 1181 * 835 // 50000                                # 19
    with pytest.raises(ValueError, match="max_systems"):
        eng.systems_from_maps_dev(1, 2, offs, hs, ws, 2, None, max_systems=need - 1)
    with pytest.raises(AssertionError, match="library was called"):      # enough capacity: the call goes through
        eng.systems_from_maps_dev(1, 2, offs, hs, ws, 2, None, max_systems=need)


def test_wrapper_rejects_mismatched_tables_before_any_call():
    eng = _bare_engine()
    with pytest.raises(ValueError, match="differ in length"):
        eng.systems_from_maps_dev(1, 2, np.zeros(2, np.int64), np.asarray([600], np.int32),
                                  np.asarray([500, 500], np.int32), 2, None, max_systems=64)
    with pytest.raises(ValueError, match="differ in length"):
        eng.systems_from_maps_dev(1, 2, np.zeros(1, np.int64), np.asarray([600, 600], np.int32),
                                  np.asarray([500, 500], np.int32), 2, None, max_systems=64)
