"""GPU: peak_local_max in two dimensions on the device (asr_notes_from_map_dev) against the host path,
sheet_utils/omr.py notes_from_map / peak_local_max, on the same float64 maps: equal counts and coordinates, in the
host's order.  Shapes lie below, at and just above the kernel's 32 x 64 tile in both directions and below the window;
the maps (tests/omr_detect_cases.py note_map) hold negative values, plateaus, peaks d - 1 and d pixels off every
border, values equal to the threshold and a peak on every tile seam."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import omr_detect_cases as C  # noqa: E402


def _engine():
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    return O._engine(0)


def _device(maps, **kw):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    eng = _engine()
    buf = eng.alloc(sum(m.size for m in maps) * 8).upload(np.concatenate([m.ravel() for m in maps]))
    try:
        return O.notes_from_map_dev(eng, buf.ptr, [m.shape[0] for m in maps], [m.shape[1] for m in maps], **kw)
    finally:
        buf.free()


def _host(m, threshold_abs, threshold_rel, d):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    return O.peak_local_max(m, min_distance=d, threshold_abs=threshold_abs, threshold_rel=threshold_rel).astype(np.int64)


def _maps(d):
    maps = [C.note_map(s, k, distance=d, quantized=k % 3 == 2) for k, s in enumerate(C.NOTE_SHAPES)]
    maps.append(np.full((40, 70), 0.7))                  # a constant page
    maps.append(np.round(C.note_map((50, 90), 77, distance=d) * 4) / 4)       # few values: windows full of ties
    return maps


@pytest.mark.parametrize("thresholds", [(0.5, None), (None, None), (0.5, 0.9), (None, 0.6), (-0.1, None)],
                         ids=["abs", "none", "abs+rel", "rel", "negative"])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_pages_equal_the_host(d, thresholds):
    thr_abs, thr_rel = thresholds
    maps = _maps(d)
    kw = dict(threshold_abs=thr_abs, threshold_rel=thr_rel, min_distance=d, max_peaks=130 * 257)
    together = _device(maps, **kw)
    found = 0
    for m, (st, coords) in zip(maps, together):
        ref = _host(m, thr_abs, thr_rel, d)
        assert st == 0, (m.shape, st)
        assert coords.dtype == np.int64 and coords.shape == ref.shape and np.array_equal(coords, ref), \
            (m.shape, len(coords), len(ref))
        (alone,) = _device([m], **kw)                    # the batch does not change a page's result
        assert alone[0] == 0 and np.array_equal(alone[1], coords)
        found += len(ref)
    assert found > 50
    assert len(together[-2][1]) == 0                     # the constant page
    if thr_abs == 0.5 and thr_rel is None:               # the comparison with the threshold is strict
        big = maps[5]
        assert (big == 0.5).any() and not (big[tuple(together[5][1].T)] == 0.5).any()


def test_pages_below_the_window_have_no_peaks():
    maps = [C.note_map((6, 40), 1), C.note_map((40, 6), 2), C.note_map((16, 17), 3)]
    res = _device(maps, threshold_abs=0.5, min_distance=8)
    assert [(st, len(c)) for st, c in res[:2]] == [(0, 0), (0, 0)]
    assert all(st == 0 for st, _ in res)
    res = _device(maps[:2], threshold_abs=0.5, min_distance=3)
    assert [len(c) for _, c in res] == [0, 0]


def test_a_page_with_a_nan_is_not_decided():
    maps = [C.note_map((37, 53), 4), C.note_map((65, 129), 5), C.note_map((33, 65), 6)]
    maps[1][64, 128] = np.nan
    maps[2][0, 0] = np.inf
    res = _device(maps, threshold_abs=0.5, min_distance=3)
    assert [st for st, _ in res] == [0, 3, 3] and res[1][1] is None
    assert np.array_equal(res[0][1], _host(maps[0], 0.5, None, 3))


def test_more_peaks_than_the_capacity():
    eng = _engine()
    maps = [C.note_map((65, 129), 7), C.note_map((37, 53), 8)]
    true = [len(_host(m, 0.5, None, 3)) for m in maps]
    assert true[0] > true[1] > 1
    buf = eng.alloc(sum(m.size for m in maps) * 8).upload(np.concatenate([m.ravel() for m in maps]))
    try:
        hs, ws = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
        status, counts, coords = eng.notes_from_map_dev(buf.ptr, hs, ws, 0.5, None, 3, true[0] - 1)
        assert status.tolist() == [4, 0] and counts.tolist() == true      # the true number is reported
        assert np.array_equal(coords[1, :true[1]], _host(maps[1], 0.5, None, 3))
        status, counts, coords = eng.notes_from_map_dev(buf.ptr, hs, ws, 0.5, None, 3, true[0])
        assert status.tolist() == [0, 0] and counts.tolist() == true
        assert np.array_equal(coords[0, :true[0]], _host(maps[0], 0.5, None, 3))
        from audio_sheet_retrieval_amd._lib import AsrError
        for bad in (0, 9, -1):
            with pytest.raises(AsrError):
                eng.notes_from_map_dev(buf.ptr, hs, ws, 0.5, None, bad, 16)
    finally:
        buf.free()
