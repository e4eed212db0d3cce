"""CPU: the definition of asr_resize_pages_dev (include/asr_hip.h) as sheet_utils/omr.resize_page_host restates it - exact
integer area resampling - against an independent derivation: every source pixel replicated h_out times down and w_out
times across, h_in x w_in block sums, rounded.  Both are exact integers, so they agree exactly."""
import inspect

import numpy as np
import pytest

from audio_sheet_retrieval_amd.sheet_utils import omr as O

SHAPES = [(7, 5, 3, 4), (13, 17, 5, 6), (5, 4, 11, 9), (9, 9, 9, 9), (64, 97, 21, 33), (1, 40, 1, 7), (40, 1, 7, 1),
          (3, 836, 2, 835), (4, 836, 4, 835)]        # the last two: sliver weights (1 / 835 of a pixel at the borders)


def replicate_and_block_sum(page, h_out, w_out):
    h_in, w_in = page.shape
    big = np.repeat(np.repeat(page.astype(np.int64), h_out, axis=0), w_out, axis=1)      # (h_in * h_out, w_in * w_out)
    S = big.reshape(h_out, h_in, w_out, w_in).sum(axis=(1, 3))
    D = h_in * w_in
    return ((2 * S + D) // (2 * D)).astype(np.uint8)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_host_restatement_equals_the_replicated_block_sums(shape):
    h, w, ho, wo = shape
    rng = np.random.default_rng(h * 1000 + w)
    for page in (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.choice(np.array([0, 255], np.uint8), (h, w))):
        got = O.resize_page_host(page, ho, wo)
        assert got.dtype == np.uint8 and got.shape == (ho, wo)
        assert np.array_equal(got, replicate_and_block_sum(page, ho, wo))


@pytest.mark.parametrize("factor", [2, 3])
def test_replicated_pages_come_back_exactly(factor):
    page = np.random.default_rng(factor).integers(0, 256, (37, 29), dtype=np.uint8)
    big = np.repeat(np.repeat(page, factor, axis=0), factor, axis=1)
    assert np.array_equal(O.resize_page_host(big, *page.shape), page)
    assert np.array_equal(O.resize_page_host(page, *big.shape), big)        # and enlarging by an integer replicates


def test_constant_pages_stay_constant():
    for value in (0, 255):
        page = np.full((23, 31), value, np.uint8)
        for ho, wo in ((7, 9), (23, 31), (40, 50)):
            assert np.all(O.resize_page_host(page, ho, wo) == value)


def test_a_half_rounds_up():
    assert O.resize_page_host(np.array([[0, 1]], np.uint8), 1, 1)[0, 0] == 1
    assert O.resize_page_host(np.array([[0, 1], [0, 0]], np.uint8), 1, 1)[0, 0] == 0


def test_resized_shape_is_the_reference_rule():
    assert O.resized_shape(3508, 2480) == (1181, 835)
    assert O.resized_shape(2339, 1654) == (1180, 835)
    assert O.resized_shape(1181, 835) == (1181, 835)
    assert O.resized_shape(100, 50, width=20) == (40, 20)


def test_resize_pages_host_uses_the_shape_rule():
    rng = np.random.default_rng(5)
    pages = [rng.integers(0, 256, (30, 20), dtype=np.uint8), rng.integers(0, 256, (17, 10), dtype=np.uint8)]
    out = O.resize_pages_host(pages, width=10)
    assert [p.shape for p in out] == [(15, 10), (17, 10)]
    assert np.array_equal(out[1], pages[1])                                  # already at that width: the identity
    assert np.array_equal(out[0], O.resize_page_host(pages[0], 15, 10))


def test_a_300_dpi_page_takes_seconds():
    """time proportional to the pixels: no dense weight matrices (they would be 1181 x 3508 and 835 x 2480 doubles
    and two matrix products)"""
    page = np.random.default_rng(9).integers(0, 256, (3508, 2480), dtype=np.uint8)
    out = O.resize_page_host(page, 1181, 835)
    assert out.shape == (1181, 835)
    block = page[:42, :30].astype(np.int64)                                  # spot check of the first output pixel
    wy = np.minimum(np.arange(1, 43) * 1181, 3508) - np.minimum(np.arange(42) * 1181, 3508)
    wx = np.minimum(np.arange(1, 31) * 835, 2480) - np.minimum(np.arange(30) * 835, 2480)
    S = int(wy @ block @ wx)
    assert out[0, 0] == (2 * S + 3508 * 2480) // (2 * 3508 * 2480)


def test_the_binding_and_the_driver_argument_exist():
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import umc
    assert "asr_resize_pages_dev" in _lib.EXPORTS
    assert hasattr(_lib.Engine, "resize_pages_dev")
    params = inspect.signature(umc.load_umc_sheets).parameters
    assert params["page_width"].default is None and list(params)[-1] == "page_width"
    assert hasattr(O.DevicePages, "resized") and callable(O.resize_pages_dev)
    from audio_sheet_retrieval_amd import umc_a2s_server
    args = umc_a2s_server._arguments(["--model", "m"], "A2S")
    assert args.page_width is None
    assert umc_a2s_server._arguments(["--model", "m", "--page_width", "835"], "S2A").page_width == 835
