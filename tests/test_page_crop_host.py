"""CPU: the host restatement of asr_crop_estimate_dev / asr_crop_pages_dev (sheet_utils/omr.crop_counts_host /
crop_rect_host / crop_page_host / crop_margin) against the definition in include/asr_hip.h written as plain loops, the
properties the definition promises - a clean page is returned as it is, an axis-aligned frame is removed exactly, only a
run that touches the edge counts, a side without a border loses nothing, an undecided page stays whole - and what the
stage does to a tilted frame, recomputed from the committed tutorial page."""
import inspect
import os

import numpy as np
import pytest

from audio_sheet_retrieval_amd.sheet_utils import omr as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAME = (37, 52, 41, 29)                 # rows at the top and at the bottom, columns left and right


def rect_by_definition(page, floor=64, share=512, margin=None):
    """the definition, one pixel at a time"""
    h, w = len(page), len(page[0])
    if margin is None:
        margin = (w + 32) // 64
    cb0, cb1, rb0, rb1 = w // 4, w - w // 4, h // 4, h - h // 4
    rowcount = [sum(1 for x in range(cb0, cb1) if page[r][x] < floor) for r in range(h)]
    colcount = [sum(1 for y in range(rb0, rb1) if page[y][c] < floor) for c in range(w)]
    border_row = [1024 * n >= share * (cb1 - cb0) for n in rowcount]
    border_col = [1024 * n >= share * (rb1 - rb0) for n in colcount]

    def run(flags):
        n = 0
        while n < len(flags) and flags[n]:
            n += 1
        return n

    top, bottom, left, right = run(border_row), run(border_row[::-1]), run(border_col), run(border_col[::-1])
    r0, r1 = top + (margin if top else 0), h - bottom - (margin if bottom else 0)
    c0, c1 = left + (margin if left else 0), w - right - (margin if right else 0)
    if top + bottom >= h or left + right >= w or r1 - r0 < 1 or c1 - c0 < 1:
        return (0, h, 0, w), 1, rowcount, colcount
    return (r0, r1, c0, c1), 0, rowcount, colcount


def framed(page, frame=FRAME, value=0):
    top, bottom, left, right = frame
    out = np.full((top + page.shape[0] + bottom, left + page.shape[1] + right), value, np.uint8)
    out[top:top + page.shape[0], left:left + page.shape[1]] = page
    return out


@pytest.fixture(scope="module")
def tutorial():
    page = np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]
    assert page.shape == (1181, 835) and page.dtype == np.uint8
    return page


def _check_against_the_definition(page, **kwargs):
    rect, status, rows, cols = rect_by_definition(page.tolist(), **kwargs)
    assert O.crop_rect_host(page, **kwargs) == (rect, status), (page.shape, kwargs)
    counts = O.crop_counts_host(page, kwargs.get("floor", 64))
    assert counts[0].dtype == np.int32 and counts[1].dtype == np.int32
    assert counts[0].tolist() == rows and counts[1].tolist() == cols
    r0, r1, c0, c1 = rect
    assert np.array_equal(O.crop_page_host(page, **kwargs), page[r0:r1, c0:c1])
    return rect, status


def test_every_small_shape_equals_the_definition():
    rng = np.random.default_rng(31)
    for h in range(1, 6):
        for w in range(1, 6):
            for floor, share, margin in ((64, 512, None), (128, 1, 0), (200, 1024, 1), (0, 512, 0), (255, 300, 2)):
                for page in (rng.integers(0, 256, (h, w), dtype=np.uint8), np.zeros((h, w), np.uint8),
                             np.full((h, w), 255, np.uint8)):
                    _check_against_the_definition(page, floor=floor, share=share, margin=margin)


@pytest.mark.parametrize("shape", [(23, 31), (40, 17), (64, 64), (67, 129)])
def test_noise_and_frames_equal_the_definition(shape):
    rng = np.random.default_rng(shape[0])
    noise = rng.integers(0, 256, shape, dtype=np.uint8)
    for floor, share in ((64, 512), (128, 512), (128, 100), (250, 1000)):
        _check_against_the_definition(noise, floor=floor, share=share, margin=1)
    paper = (255 - (rng.random(shape) < 0.05) * 255).astype(np.uint8)
    for frame in ((3, 0, 0, 0), (0, 2, 5, 0), (1, 2, 3, 4), (0, 0, 0, 0)):
        page = framed(paper, frame)
        rect, status = _check_against_the_definition(page, margin=0)
        assert status == 0 and rect == (frame[0], frame[0] + shape[0], frame[2], frame[2] + shape[1])


def test_the_clean_page_is_returned_as_it_is(tutorial):
    assert O.crop_rect_host(tutorial) == ((0, 1181, 0, 835), 0)
    assert O.crop_rect_host(tutorial, margin=500) == ((0, 1181, 0, 835), 0)      # no border: the margin cuts nothing
    assert np.array_equal(O.crop_page_host(tutorial), tutorial)


def test_the_frame_of_the_tutorial_page_is_removed_exactly(tutorial):
    page = framed(tutorial)
    assert page.shape == (1270, 905)
    assert O.crop_rect_host(page, margin=0) == ((37, 1218, 41, 876), 0)
    assert np.array_equal(O.crop_page_host(page, margin=0), tutorial)
    assert O.crop_margin(905) == 14 and O.crop_rect_host(page) == ((51, 1204, 55, 862), 0)
    assert np.array_equal(O.crop_page_host(page), tutorial[14:-14, 14:-14])
    for value in (1, 63):                                           # a frame that is merely darker than the floor
        assert O.crop_rect_host(framed(tutorial, value=value), margin=0) == ((37, 1218, 41, 876), 0)
    assert O.crop_rect_host(framed(tutorial, value=64), margin=0) == ((0, 1270, 0, 905), 0)


def test_the_default_margin_is_that_of_the_width():
    assert [O.crop_margin(w) for w in (1, 31, 32, 95, 96, 835, 2480, 16384)] == [0, 0, 1, 1, 2, 13, 39, 256]
    assert O.CROP_SHARE == 512 and O.CROP_FLOOR == 64


@pytest.mark.parametrize("margin", [0, 1, 14, 100])
def test_a_side_without_a_border_loses_nothing(tutorial, margin):
    small = tutorial[:400, :300]
    assert O.crop_rect_host(framed(small, (9, 0, 0, 0)), margin=margin) == ((9 + margin, 409, 0, 300), 0)
    assert O.crop_rect_host(framed(small, (0, 7, 0, 5)), margin=margin) == ((0, 400 - margin, 0, 300 - margin), 0)
    assert O.crop_rect_host(framed(small, (0, 0, 11, 0)), margin=margin) == ((0, 400, 11 + margin, 311), 0)


def test_an_undecided_page_stays_whole(tutorial):
    assert O.crop_rect_host(np.zeros((30, 20), np.uint8)) == ((0, 30, 0, 20), 1)
    assert O.crop_rect_host(np.zeros((30, 20), np.uint8), margin=0) == ((0, 30, 0, 20), 1)
    assert O.crop_rect_host(np.zeros((1, 1), np.uint8)) == ((0, 1, 0, 1), 1)
    small = framed(tutorial[:100, :80], (5, 5, 5, 5))
    assert O.crop_rect_host(small, margin=39) == ((44, 66, 44, 46), 0)
    assert O.crop_rect_host(small, margin=40) == ((0, 110, 0, 90), 1)            # 90 - 10 - 80 columns: nothing is left
    assert O.crop_rect_host(small, margin=10 ** 6) == ((0, 110, 0, 90), 1)
    assert np.array_equal(O.crop_page_host(small, margin=40), small)


def test_floor_zero_is_the_identity(tutorial):
    for page in (framed(tutorial), np.zeros((9, 7), np.uint8)):
        assert O.crop_rect_host(page, floor=0) == ((0,) + (page.shape[0],) + (0,) + (page.shape[1],), 0)
        rows, cols = O.crop_counts_host(page, 0)
        assert not rows.any() and not cols.any()


def test_the_limit_is_inclusive():
    """a band of 20 columns (W = 40) at share 512: 10 dark pixels make a border row, 9 do not; at share 500 the limit
    500 * 20 / 1024 = 9.77 lies between the same two counts, and at share 461 (9.004) as well, at 460 (8.98) 9 are enough"""
    def top_row(n_dark):
        page = np.full((40, 40), 255, np.uint8)
        page[0, 10:10 + n_dark] = 0
        return page
    assert 1024 * 10 == 512 * 20
    assert O.crop_rect_host(top_row(10), margin=0) == ((1, 40, 0, 40), 0)
    assert O.crop_rect_host(top_row(9), margin=0) == ((0, 40, 0, 40), 0)
    assert O.crop_rect_host(top_row(9), share=461, margin=0) == ((0, 40, 0, 40), 0)
    assert O.crop_rect_host(top_row(9), share=460, margin=0) == ((1, 40, 0, 40), 0)
    assert O.crop_rect_host(top_row(20), share=1024, margin=0) == ((1, 40, 0, 40), 0)
    assert O.crop_rect_host(top_row(19), share=1024, margin=0) == ((0, 40, 0, 40), 0)
    assert O.crop_rect_host(top_row(1), share=1, margin=0) == ((1, 40, 0, 40), 0)
    page = top_row(20)
    page[0, :10] = 0                                                # outside the band: not counted
    page[0, 10:30] = 255
    assert O.crop_rect_host(page, share=1, margin=0) == ((0, 40, 0, 40), 0)
    column = np.full((40, 40), 255, np.uint8)
    column[10:20, 39] = 0                                           # the same limit for a column, at the far edge
    assert O.crop_rect_host(column, margin=0) == ((0, 40, 0, 39), 0)
    column[10, 39] = 255
    assert O.crop_rect_host(column, margin=0) == ((0, 40, 0, 40), 0)


def test_a_dark_row_that_does_not_touch_the_edge_is_kept():
    page = np.full((60, 50), 255, np.uint8)
    page[:4] = 0                                                    # the frame
    page[4:7] = 255                                                 # the page's white margin
    page[7:9] = 0                                                   # a staff line: a border row by its count
    page[30] = 0
    page[:, 20] = np.where(np.arange(60) >= 4, 0, page[:, 20])      # a bar line across the page
    assert O.crop_rect_host(page, margin=0) == ((4, 60, 0, 50), 0)
    assert O.crop_rect_host(page, margin=2) == ((6, 60, 0, 50), 0)


def _tilted(tutorial, k):
    """the framed tutorial page sheared by k / 1024 with black beyond the scan, and which of its pixels are paper"""
    page = framed(tutorial)
    mask = framed(np.full(tutorial.shape, 255, np.uint8))
    return O.shear_page_host(page, k, fill=0), O.shear_page_host(mask, k, fill=0) >= 128


def tilt_figures(tutorial, k, margin):
    """-> (frame pixels left in the crop, ink pixels cut off, rect): dark (< 64) pixels inside the rect that are not paper,
    and dark pixels of the paper outside it"""
    scan, paper = _tilted(tutorial, k)
    (r0, r1, c0, c1), status = O.crop_rect_host(scan, margin=margin)
    assert status == 0
    inside = np.zeros(scan.shape, bool)
    inside[r0:r1, c0:c1] = True
    dark = scan < 64
    return int((inside & ~paper & dark).sum()), int((~inside & paper & dark).sum()), (r0, r1, c0, c1)


@pytest.mark.parametrize("k", [10, 30, 64, -64])
def test_a_tilted_frame_at_the_default_margin(tutorial, k):
    """measured here: k = 10: 0 frame pixels left, 0 ink pixels cut; 30: 239, 0; 64: 9921, 151; -64: 9920, 441 - the
    corner residue of a tilted frame is about |k| * W / 2048 rows, more than the margin of 14 from |k| = 30 on"""
    assert O.crop_margin(905) == 14
    left, cut, rect = tilt_figures(tutorial, k, 14)
    print("tilt %d / 1024, margin 14: rect %s, %d frame pixels left in the crop, %d ink pixels cut off" % (k, rect, left, cut))
    if k == 10:
        assert left == 0
    if k in (10, 30):
        assert cut == 0
    bare_left, bare_cut, _ = tilt_figures(tutorial, k, 0)
    print("tilt %d / 1024, margin 0: %d frame pixels left in the crop, %d ink pixels cut off" % (k, bare_left, bare_cut))
    assert bare_cut == 0 and bare_left > left                       # without the margin no ink is lost, and more frame stays


@pytest.mark.parametrize("k", [10, 30, 64])
def test_the_skew_estimate_is_the_same_before_and_after_the_crop(tutorial, k):
    scan, _ = _tilted(tutorial, k)
    assert O.estimate_skew_host(scan) == -k
    assert O.estimate_skew_host(O.crop_page_host(scan, margin=0)) == -k


def test_a_small_share_eats_a_tilted_page(tutorial):
    """why the default share is a half: at share 16 and a tilt of 64 / 1024 the frame's wedge is wider than the page's white
    margin, the run of border columns never meets a white column and goes on into the music"""
    scan, _ = _tilted(tutorial, 64)
    (_, _, c0, _), _ = O.crop_rect_host(scan, share=16, margin=0)
    (_, _, d0, _), _ = O.crop_rect_host(scan, margin=0)
    print("tilt 64 / 1024: c0 = %d at share 16, %d at share 512" % (c0, d0))
    assert c0 > 400 and d0 == 41


def test_arguments_outside_their_ranges_raise():
    page = np.zeros((4, 4), np.uint8)
    for kwargs in (dict(floor=-1), dict(floor=256), dict(share=0), dict(share=1025), dict(margin=-1)):
        with pytest.raises(ValueError):
            O.crop_rect_host(page, **kwargs)
    with pytest.raises(ValueError):
        O.crop_counts_host(page.astype(np.float32))
    with pytest.raises(ValueError):
        O.crop_counts_host(page, floor=300)


def test_the_bindings_and_the_drivers_exist():
    from audio_sheet_retrieval_amd import _lib, umc_a2s_server
    from audio_sheet_retrieval_amd.sheet_utils import umc
    for name in ("asr_crop_estimate_dev", "asr_crop_pages_dev"):
        assert name in _lib.EXPORTS
    assert hasattr(_lib.Engine, "crop_estimate_dev") and hasattr(_lib.Engine, "crop_pages_dev")
    assert hasattr(O.DevicePages, "cropped") and callable(O.crop_pages_dev)
    params = inspect.signature(O.DevicePages.cropped).parameters
    assert [(n, p.default) for n, p in list(params.items())[1:]] == [("floor", 64), ("share", 512), ("margin", None),
                                                                      ("rects", None)]
    params = inspect.signature(O.crop_rect_host).parameters
    assert [(n, p.default) for n, p in list(params.items())[1:]] == [("floor", 64), ("share", 512), ("margin", None)]
    assert inspect.signature(O.crop_counts_host).parameters["floor"].default == 64
    params = inspect.signature(umc.load_umc_scans).parameters
    assert params["crop"].default is False
    names = list(params)
    assert names[names.index("score_map") + 1:] == ["crop", "crop_floor", "crop_share", "crop_margin"]
    assert [params[n].default for n in ("crop_floor", "crop_share", "crop_margin")] == [64, 512, None]
    assert params["flatten"].default is False and params["deskew"].default is True and params["score_map"].default is False
    for direction in ("A2S", "S2A"):
        assert umc_a2s_server._arguments(["--model", "m"], direction).crop is False
        args = umc_a2s_server._arguments(["--model", "m", "--crop"], direction)
        assert args.crop is True and args.deskew is False and args.flatten is False and args.page_width is None


def test_the_signature_of_load_umc_sheets_is_unchanged():
    from audio_sheet_retrieval_amd.sheet_utils import umc
    params = inspect.signature(umc.load_umc_sheets).parameters
    assert [(n, p.default) for n, p in params.items()] == [
        ("data_dir", inspect.Parameter.empty), ("require_performance", False), ("omr", None), ("system_params", None),
        ("bar_params", None), ("device", 0), ("return_device", False), ("device_post", False), ("page_width", None)]
