"""CPU: the host side of bar and note-head detection (sheet_utils/omr.py): bar_blob_props against an independent
derivation (eigen-decomposition of the pixel covariance), the filters' verdicts on synthetic blobs, blob_stats against a
per-pixel loop, notes_from_map against a brute-force search, and the alignment of bars with systems on hand-made
cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import omr_detect_cases as C  # noqa: E402
from audio_sheet_retrieval_amd.sheet_utils import omr as O  # noqa: E402


def _eigh_props(mask):
    """(major axis, orientation modulo pi, eccentricity) from np.linalg.eigh of the covariance of the pixel
    coordinates (x = column, y = row)"""
    rr, cc = np.nonzero(mask)
    xy = np.stack([cc, rr]).astype(np.float64)
    xy -= xy.mean(1, keepdims=True)
    cov = xy @ xy.T / xy.shape[1]
    vals, vecs = np.linalg.eigh(cov)
    l2, l1 = vals
    vx, vy = vecs[:, 1]
    theta = np.arctan2(vy, vx)                           # the major axis, image coordinates (y down)
    return 4 * np.sqrt(l1), -theta, (0.0 if l1 == 0 else np.sqrt(max(0.0, 1 - l2 / l1)))


def _random_blob(seed):
    rng = np.random.default_rng(seed)
    h, w = 120, 140
    y, x = np.mgrid[:h, :w].astype(np.float64)
    y -= h / 2 + rng.uniform(-5, 5)
    x -= w / 2 + rng.uniform(-5, 5)
    t = rng.uniform(0, np.pi)
    sa, sb = rng.uniform(25, 45), rng.uniform(3, 12)
    u, v = x * np.cos(t) + y * np.sin(t), -x * np.sin(t) + y * np.cos(t)
    mask = (u / sa) ** 2 + (v / sb) ** 2 < 1
    mask &= rng.random((h, w)) < 0.9                     # holes
    return mask


def _props_cases():
    cases = list(C.bar_blob_masks().items())
    cases += [("random%d" % s, _random_blob(s)) for s in range(8)]
    return cases


@pytest.mark.parametrize("name,mask", _props_cases(), ids=[n for n, _ in _props_cases()])
def test_bar_blob_props_equal_the_eigen_decomposition(name, mask):
    stats = O.blob_stats(mask.astype(np.int64), 1)
    major, orientation, ecc = O.bar_blob_props(stats[0])
    ref_major, ref_orientation, ref_ecc = _eigh_props(mask)
    assert abs(major - ref_major) <= 1e-9 * ref_major
    assert abs(ecc - ref_ecc) <= 1e-9 * max(ref_ecc, 1e-300)
    # orientations are axes: equal modulo pi.  1e-9 relative to the half turn the angle lives in.
    diff = (orientation - ref_orientation) % np.pi
    assert min(diff, np.pi - diff) <= 1e-9 * np.pi / 2, (orientation, ref_orientation)
    assert -np.pi / 2 <= orientation <= np.pi / 2


def test_bar_blob_props_of_the_table():
    masks = C.bar_blob_masks()
    props = {k: O.bar_blob_props(O.blob_stats(m.astype(np.int64), 1)[0]) for k, m in masks.items()}
    assert round(props["bar70"][0], 2) == 80.82 and round(props["bar69"][0], 2) == 79.67
    assert round(props["block"][2], 3) == 0.943
    assert props["hstroke"][1] == 0.0
    for name, lo, hi in (("slant4.0", 85.5, 86.5), ("slant-4.5", 85.0, 86.0), ("slant6.0", 83.5, 84.5),
                         ("slant-5.5", 84.0, 85.0)):
        assert lo < abs(np.degrees(props[name][1])) < hi, (name, np.degrees(props[name][1]))
    # a == c: the quarter turn by the sign of the cross moment
    diag = np.eye(9, dtype=np.int64)
    assert O.bar_blob_props(O.blob_stats(diag, 1)[0])[1] == -np.pi / 4
    assert O.bar_blob_props(O.blob_stats(diag[::-1].copy(), 1)[0])[1] == np.pi / 4
    assert O.bar_blob_props(O.blob_stats(np.ones((1, 1), np.int64), 1)[0]) == (0.0, np.pi / 4, 0.0)


@pytest.mark.parametrize("name", C.BAR_BLOBS)
def test_filter_verdicts(name):
    mask = C.bar_blob_masks()[name]
    bars = O.bars_from_stats(O.blob_stats(mask.astype(np.int64), 1))
    assert (len(bars) == 1) == C.BAR_VERDICTS[name]
    if len(bars):
        rr, cc = np.nonzero(mask)
        col = (cc.min() + cc.max() + 1) / 2.0
        assert bars.dtype == np.float64 and bars.tolist() == [[[rr.min(), col], [rr.max() + 1, col]]]


def test_bars_from_map_keeps_the_three():
    prob, mask = C.bar_blob_map()
    lab, n = O.label8(mask)
    assert n == len(C.BAR_BLOBS)
    drawn = O.blob_stats(lab, n)
    stats = O.bar_blobs_from_map(prob)
    assert len(stats) > n                                # background pixels above the Otsu threshold: tiny blobs
    assert np.array_equal(stats[stats[:, 0] >= 100], drawn)
    bars = O.bars_from_map(prob)
    assert np.array_equal(bars, O.bars_from_stats(drawn)) and bars.shape == (3, 2, 2)
    assert bars[0].tolist() == [[10.0, 23.0], [80.0, 23.0]]


def test_blob_stats_equal_a_pixel_loop():
    rng = np.random.default_rng(3)
    fg = rng.random((41, 57)) < 0.35
    fg[0, :] = True                                      # touches borders
    lab, n = O.label8(fg)
    assert n > 5
    ref = np.zeros((n, 10), np.int64)
    ref[:, 1] = ref[:, 2] = 1 << 40
    for r in range(lab.shape[0]):
        for c in range(lab.shape[1]):
            k = lab[r, c] - 1
            if k < 0:
                continue
            ref[k, 0] += 1
            ref[k, 1] = min(ref[k, 1], r); ref[k, 2] = min(ref[k, 2], c)
            ref[k, 3] = max(ref[k, 3], r + 1); ref[k, 4] = max(ref[k, 4], c + 1)
            ref[k, 5:] += [r, c, r * r, c * c, r * c]
    got = O.blob_stats(lab, n)
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert O.blob_stats(np.zeros((3, 3), np.int64), 0).shape == (0, 10)
    # area and box agree with the region properties the system detection uses
    assert [(i + 1, int(a), tuple(b)) for i, (a, b) in enumerate(zip(got[:, 0], got[:, 1:5].tolist()))] == \
        O.regionprops(lab, n)


def _brute_peaks(m, threshold_abs, d):
    h, w = m.shape
    if np.all(m == m[0, 0]):
        return np.empty((0, 2), np.int64)
    thr = m.min() if threshold_abs is None else threshold_abs
    out = []
    for r in range(h):
        for c in range(w):
            if r < d or r >= h - d or c < d or c >= w - d:
                continue
            best = 0.0 if (r - d < 0 or c - d < 0 or r + d >= h or c + d >= w) else -np.inf
            for q in range(max(r - d, 0), min(r + d, h - 1) + 1):
                for x in range(max(c - d, 0), min(c + d, w - 1) + 1):
                    best = max(best, m[q, x])
            if m[r, c] == best and m[r, c] > thr:
                out.append((r, c))
    return np.asarray(out[::-1], np.int64).reshape(-1, 2)


@pytest.mark.parametrize("shape,d,thr", [((6, 40), 3, 0.5), ((7, 7), 3, 0.5), ((23, 31), 1, 0.5), ((23, 31), 3, None),
                                         ((19, 40), 8, 0.5), ((37, 53), 3, 0.5), ((30, 30), 2, -0.2)])
def test_notes_from_map_equals_the_brute_force_search(shape, d, thr):
    for seed, quantized in ((0, False), (1, True)):
        m = C.note_map(shape, seed, distance=d, quantized=quantized)
        assert (m < 0).any()
        got = O.notes_from_map(m, threshold_abs=thr, min_distance=d)
        ref = _brute_peaks(m, thr, d)
        assert got.dtype == np.int64 and got.shape == ref.shape and np.array_equal(got, ref)
    assert O.notes_from_map(np.full(shape, 0.7), min_distance=d).shape == (0, 2)


def _system(r0, r1, c0, c1):
    return np.asarray([[r0, c0], [r0, c1], [r1, c1], [r1, c0]], np.float64)


def _bar(r0, r1, c):
    return np.asarray([[r0, c], [r1, c]], np.float64)


def test_align_bars_with_systems():
    systems = np.stack([_system(100, 200, 50, 700), _system(300, 400, 60, 710)])
    bars = np.stack([_bar(305, 395, 710.0), _bar(102, 198, 400.0), _bar(101, 199, 50.0), _bar(300, 400, 70.0),
                     _bar(105, 195, 690.0), _bar(301, 399, 380.0)])
    by = O.bars_by_systems(bars, systems)
    assert [b[:, 0, 1].tolist() for b in by] == [[50.0, 400.0, 690.0], [70.0, 380.0, 710.0]]
    out = O.align_bars_with_systems(bars, systems)
    # system 0: the left bar is there; the last bar is exactly 10 px off the right edge - not missing.
    # system 1: the first bar is 10 px off the left edge, which is not equal to it: a bar is added there, with the
    # reference's corner indices (its second corner is [column, column] before the rows are overwritten)
    assert out.tolist() == [
        [[100.0, 50.0], [200.0, 400.0 * 0 + 50.0]], [[100.0, 400.0], [200.0, 400.0]], [[100.0, 690.0], [200.0, 690.0]],
        [[300.0, 60.0], [400.0, 60.0]], [[300.0, 70.0], [400.0, 70.0]], [[300.0, 380.0], [400.0, 380.0]],
        [[300.0, 710.0], [400.0, 710.0]]]
    # missing right bar: stacked in FRONT of the system's bars
    out = O.align_bars_with_systems(np.stack([_bar(101, 199, 50.0), _bar(102, 198, 400.0)]), systems[:1])
    assert out[:, 0, 1].tolist() == [700.0, 50.0, 400.0]
    assert out[:, :, 0].tolist() == [[100.0, 200.0]] * 3
    # missing left and right
    out = O.align_bars_with_systems(np.stack([_bar(102, 198, 400.0)]), systems[:1])
    assert out[:, 0, 1].tolist() == [700.0, 50.0, 400.0]
    # equal distances to two systems: the first one takes the bar (centres 150 and 350, the bar at 250)
    by = O.bars_by_systems(np.stack([_bar(240, 260, 300.0)]), systems)
    assert [len(b) for b in by] == [1, 0]
    # equal columns keep their order
    by = O.bars_by_systems(np.stack([_bar(110, 190, 300.0), _bar(120, 180, 300.0), _bar(100, 200, 100.0)]), systems[:1])
    assert by[0][:, 0, 0].tolist() == [100.0, 110.0, 120.0]
    with pytest.raises(IndexError):                      # a system without a bar
        O.align_bars_with_systems(np.stack([_bar(102, 198, 400.0)]), systems)
    with pytest.raises(ValueError):                      # no bars at all
        O.align_bars_with_systems(np.zeros((0, 2, 2)), systems)
    assert O.align_bars_with_systems(np.zeros((0, 2, 2)), np.zeros((0, 4, 2))).shape == (0, 2, 2)


def test_the_note_network_and_the_calls_are_declared():
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import note_detector, umc
    assert note_detector.INPUT_SHAPE == [1, 256, 512]
    assert tuple(note_detector.build_model().input_shape) == (1, 256, 512)
    for name in ("asr_notes_from_map_dev", "asr_bars_from_map_dev"):
        assert name in _lib.EXPORTS
    params = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "omr_note_params.npz"))
    arrs = [params["p%02d" % i] for i in range(99)]
    assert sum(a.size for a in arrs) == 110033 and all(a.dtype == np.float32 for a in arrs)
    assert [a.shape for a in arrs] == [tuple(s) for s in note_detector.param_shapes()]
    assert "note_params" in umc.build_recognizer.__code__.co_varnames
    for m in ("detect_notes", "detect_bars", "detect_notes_pages", "detect_bars_pages", "detect_notes_pages_dev",
              "detect_bars_pages_dev"):
        assert callable(getattr(O.OpticalMusicRecognizer, m))
