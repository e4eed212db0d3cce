"""GPU: the blob statistics of detect_bars on the device (asr_bars_from_map_dev) against the host path,
sheet_utils/omr.py bar_blobs_from_map (threshold_otsu, 8-connected labels, blob_stats), on the same float64 maps: the
ten integers of every blob, in label order.  The filters are shared host code (bars_from_stats), so equal integers give
equal bars."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import omr_detect_cases as C  # noqa: E402
import omr_post_cases as post_cases  # noqa: E402

MAX_BLOBS = 65536


def _engine():
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    return O._engine(0)


def _device(maps, max_blobs=MAX_BLOBS):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    eng = _engine()
    buf = eng.alloc(sum(m.size for m in maps) * 8).upload(np.concatenate([m.ravel() for m in maps]))
    try:
        res, passes = O.bar_blobs_from_map_dev(eng, buf.ptr, [m.shape[0] for m in maps], [m.shape[1] for m in maps],
                                               max_blobs=max_blobs)
    finally:
        buf.free()
    assert passes >= 1
    return res


def _check(m, dev):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    st, stats = dev
    ref = O.bar_blobs_from_map(m)
    assert st == 0, (m.shape, st)
    assert stats.dtype == np.int64 and stats.shape == ref.shape, (m.shape, stats.shape, ref.shape)
    assert np.array_equal(stats, ref), (m.shape, np.argwhere(stats != ref)[:5])
    bars = O.bars_from_stats(stats)
    assert np.array_equal(bars, O.bars_from_map(m))
    return ref, bars


def _strokes():
    """small maps of two values: two strokes that touch diagonally only (one blob under 8-connectivity), and a frame
    that touches all four borders around a separate dot"""
    a = np.full((70, 90), 0.1)
    a[5:35, 20:24] = 0.9
    a[35:65, 24:28] = 0.9                                # corner to corner with the first stroke
    a[10:20, 60:63] = 0.9                                # a second blob
    b = np.full((45, 131), 0.1)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = 0.9
    b[20:24, 60:70] = 0.9
    return a, b


def test_the_synthetic_blobs_and_small_pages_in_one_call():
    prob, mask = C.bar_blob_map()
    a, b = _strokes()
    maps = [prob, a, b, prob[:97, :65].copy()]
    res = _device(maps)
    refs = [_check(m, d) for m, d in zip(maps, res)]
    assert len(refs[0][0]) > len(C.BAR_BLOBS) and len(refs[0][1]) == 3       # bar70 and the two small slants
    assert len(refs[1][0]) == 2 and refs[1][0][0].tolist()[:5] == [240, 5, 20, 65, 28]
    assert len(refs[2][0]) == 2 and refs[2][0][0].tolist()[:5] == [2 * 131 + 2 * 43, 0, 0, 45, 131]
    for m, d in zip(maps, res):                          # the batch does not change a page's result
        (alone,) = _device([m])
        assert alone[0] == 0 and np.array_equal(alone[1], d[1])


@pytest.mark.parametrize("seeds", [(8, 6), (3, 9)], ids=["diagonal+borders", "spiral+mixed"])
def test_post_case_maps_two_pages_of_different_sizes(seeds):
    cases = [post_cases.make_case(s) for s in seeds]
    assert [c["scenario"] for c in cases] == [post_cases.SCENARIOS[s % 10] for s in seeds]
    maps = [c["system"] for c in cases]
    assert maps[0].shape != maps[1].shape
    for m, d in zip(maps, _device(maps)):
        ref, _ = _check(m, d)
        assert len(ref) > 3


def test_more_blobs_than_the_capacity_and_undecided_pages():
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    prob, _ = C.bar_blob_map()
    a, b = _strokes()
    n = len(O.bar_blobs_from_map(prob))
    res = _device([prob, a], max_blobs=n - 1)
    assert res[0] == (O.ST_OVERFLOW, None) and res[1][0] == 0
    eng = _engine()
    buf = eng.alloc(prob.size * 8).upload(prob.ravel())
    try:
        status, counts, _, _ = eng.bars_from_map_dev(buf.ptr, [prob.shape[0]], [prob.shape[1]], n - 1)
        assert status.tolist() == [4] and counts.tolist() == [n]
    finally:
        buf.free()
    _check(prob, _device([prob], max_blobs=n)[0])
    bad = b.copy()
    bad[3, 3] = np.nan
    res = _device([bad, b])
    assert res[0] == (O.ST_UNDECIDED, None)
    _check(b, res[1])
