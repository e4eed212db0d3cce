"""CPU: staff-system detection without a device.

The restatement's self-checks (tests/omr_ref.py: transposed-conv orientation, sliding-window tiling), the package's
restated library functions (sheet_utils/omr.py) against brute-force versions, the parameter loader against the
fixture, the page anchor (the reference's weights and tutorial page: six systems where the staves are) and the loader's
page reading and unrolling rules."""
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import omr_ref  # noqa: E402

from audio_sheet_retrieval_amd.sheet_utils import omr as O  # noqa: E402


# ---- restatement self-checks ----------------------------------------------------------------------------------------

def test_transposed_conv_is_the_adjoint_of_the_strided_correlation():
    rng = np.random.default_rng(0)
    W = rng.standard_normal((5, 3, 2, 2))
    x = rng.standard_normal((5, 4, 6))
    y = rng.standard_normal((3, 8, 12))
    lhs = float(np.sum(omr_ref.strided_corr(y, W) * x))
    rhs = float(np.sum(y * omr_ref.transposed_conv(x, W, flip=True)))
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    # the other orientation is not the adjoint
    rhs_unflipped = float(np.sum(y * omr_ref.transposed_conv(x, W, flip=False)))
    assert abs(lhs - rhs_unflipped) > 1e-3


def test_transposed_conv_hand_case():
    W = np.arange(4, dtype=float).reshape(1, 1, 2, 2)        # [[0, 1], [2, 3]]
    x = np.array([[[1.0, 10.0]]])                             # 1 x 1 x 2
    y = omr_ref.transposed_conv(x, W, flip=True)
    # out[2i + a, 2j + b] = x[i, j] * W[1 - a, 1 - b]: each 2x2 block is the kernel rotated by 180 degrees
    assert np.array_equal(y[0], [[3, 2, 30, 20], [1, 0, 10, 0]])


@pytest.mark.parametrize("overlap", [0.5, 0.0, 0.75])
@pytest.mark.parametrize("shape", [(1181, 835), (300, 200), (512, 700)])
def test_tiling_all_ones_network_gives_one(overlap, shape):
    page = np.zeros(shape, np.float32)
    out = omr_ref.sliding_window(page, (512, 512), lambda t: np.ones((512, 512), np.float32), overlap)
    assert out.shape == shape
    assert np.all(out == 1.0)            # every pixel covered: R / V of identical weights is exactly 1


def test_tiling_uncovered_pixels_are_nan():
    h, w, th = 1100, 700, 512
    out = omr_ref.sliding_window(np.zeros((h, w), np.float32), (th, th), lambda t: np.ones((th, th)), overlap=0.3)
    pad_top, pad_left, row_0, col_0 = O.tile_grid(h, w, th, th, 0.3)
    cov = np.zeros((h + 2 * pad_top + 4, w + 2 * pad_left + 4), bool)
    for r in row_0:
        for c in col_0:
            cov[r:r + th, c:c + th] = True
    cov = cov[pad_top:pad_top + h, pad_left:pad_left + w]
    assert (~cov).any()
    assert np.array_equal(np.isnan(out), ~cov)
    assert np.all(out[cov] == 1.0)


def test_tile_grid_matches_the_restatement():
    for (h, w), (th, tw), ov in [((1181, 835), (512, 512), 0.5), ((1181, 835), (256, 512), 0.5), ((90, 40), (256, 512), 0.75)]:
        tiles = omr_ref.tiles_of(np.arange(h * w, dtype=np.float32).reshape(h, w) + 1, (th, tw), ov)
        pad_top, pad_left, row_0, col_0 = O.tile_grid(h, w, th, tw, ov)
        assert len(tiles) == len(row_0) * len(col_0)
        t = tiles[-1]
        r0, c0 = row_0[-1] - pad_top, col_0[-1] - pad_left
        nz = np.argwhere(t > 0)
        assert t[nz[0][0], nz[0][1]] == r0 * w + c0 + 1 + nz[0][0] * w + nz[0][1] if r0 >= 0 and c0 >= 0 else True


def test_tile_window_is_numpys():
    assert np.array_equal(O.tile_window(256, 512), np.sqrt(np.outer(np.hamming(256), np.hamming(512))))


# ---- restated library functions ------------------------------------------------------------------------------------

def _otsu_brute(x, nbins=256):
    hist, edges = np.histogram(x.ravel(), bins=nbins)
    centers = (edges[:-1] + edges[1:]) / 2
    best, arg = -1.0, None
    for k in range(nbins - 1):           # class 1: bins 0..k
        w1, w2 = hist[:k + 1].sum(), hist[k + 1:].sum()
        if w1 == 0 or w2 == 0:
            v = 0.0
        else:
            m1 = (hist[:k + 1] * centers[:k + 1]).sum() / w1
            m2 = (hist[k + 1:] * centers[k + 1:]).sum() / w2
            v = w1 * w2 * (m1 - m2) ** 2
        if v > best * (1 + 1e-12):
            best, arg = v, centers[k]
    return arg


@pytest.mark.parametrize("seed", range(4))
def test_otsu_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.normal(0.2, 0.05, 3000), rng.normal(0.7 + 0.05 * seed, 0.1, 1000)])
    assert O.threshold_otsu(x) == _otsu_brute(x)


def _close_loop(fg, k=15):
    h, w = fg.shape
    a = k // 2
    d = np.zeros_like(fg)
    for y in range(h):
        for x in range(w):
            d[y, x] = max(fg[yy, x] for yy in range(max(0, y - a), min(h, y + a + 1)))        # outside: no dilation
    e = np.zeros_like(fg)
    for y in range(h):
        for x in range(w):
            e[y, x] = min(d[yy, x] for yy in range(max(0, y - a), min(h, y + a + 1)))        # outside: no erosion
    return e


def test_vertical_closing_against_a_direct_loop():
    rng = np.random.default_rng(1)
    fg = (rng.random((60, 9)) > 0.7).astype(np.uint8)
    fg[0:3, 4] = 1                        # touches the border: the border must not erode it
    fg[-2:, 2] = 1
    got = O.close_vertical(fg, 15)
    assert got.dtype == np.uint8
    assert np.array_equal(got, _close_loop(fg, 15))


def _flood_label(fg):
    h, w = fg.shape
    lab = np.zeros((h, w), int)
    n = 0
    for y in range(h):
        for x in range(w):
            if fg[y, x] and not lab[y, x]:
                n += 1
                stack = [(y, x)]
                lab[y, x] = n
                while stack:
                    cy, cx = stack.pop()
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            yy, xx = cy + dy, cx + dx
                            if 0 <= yy < h and 0 <= xx < w and fg[yy, xx] and not lab[yy, xx]:
                                lab[yy, xx] = n
                                stack.append((yy, xx))
    return lab, n


def test_labelling_against_a_flood_fill():
    rng = np.random.default_rng(2)
    fg = rng.random((40, 50)) > 0.6
    lab, n = O.label8(fg)
    ref, nr = _flood_label(fg)
    assert n == nr and np.array_equal(lab, ref)
    props = O.regionprops(lab, n)
    for (l, area, (r0, c0, r1, c1)) in props:
        ys, xs = np.nonzero(ref == l)
        assert area == ys.size and (r0, c0, r1, c1) == (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    assert [p[0] for p in props] == list(range(1, n + 1))


def test_peak_local_max_hand_signals():
    s = np.array([0, 1, 0, 3, 3, 0, 2, 0, 5], float)
    # border points excluded (the 5 at the end), ties are both peaks, threshold 0.5 * max = 2.5: 3 and 3 only;
    # order reversed (highest index first)
    assert O.peak_local_max(s, threshold_rel=0.5)[:, 0].tolist() == [4, 3]
    assert O.peak_local_max(s, threshold_rel=0.1)[:, 0].tolist() == [6, 4, 3, 1]
    assert O.peak_local_max(np.ones(7)).shape == (0, 1)
    # argmin over the reversed order picks the larger of two equidistant candidates
    c = O.peak_local_max(np.array([0, 0, 4, 0, 0, 0, 4, 0, 0], float), threshold_rel=0.5)
    assert c[np.argmin(np.abs(4 - c)), 0] == 6


def _page_with_rect(r0, r1, c0, c1, h=200, w=300):
    img = np.ones((h, w), np.float32)
    img[r0, c0:c1 + 1] = 0                      # top and bottom lines, left and right bar lines
    img[r1, c0:c1 + 1] = 0
    img[r0:r1 + 1, c0] = 0
    img[r0:r1 + 1, c1] = 0
    return img


def test_snap_to_grid_on_a_drawn_rectangle():
    img = _page_with_rect(50, 120, 40, 250)
    # rows snap to the lines; columns: min_col snaps, but the x-direction compares with max_row (120), not max_col
    # (250): no column candidate lies within 10 of 120, so the columns stay as they were
    r = O.snap_system_to_grid(img[None, None], 53, 118, 43, 247)
    assert (int(r[0]), int(r[1]), int(r[2]), int(r[3])) == (50, 120, 43, 247)
    # with a bar line drawn at column 125 (within 10 of max_row), both column snaps happen
    img2 = img.copy()
    img2[50:121, 125] = 0
    r2 = O.snap_system_to_grid(img2[None, None], 53, 118, 43, 247)
    assert (int(r2[0]), int(r2[1]), int(r2[2]), int(r2[3])) == (50, 120, 40, 125)


def test_shrink_bounding_box_on_a_drawn_blob():
    fg = np.zeros((100, 120), bool)
    fg[20:80, 10:110] = True
    fg[15:20, 50:52] = True                     # a thin spike above: the bbox grows, the shrink removes it
    lab, n = O.label8(fg)
    (_, _, bbox), = O.regionprops(lab, n)
    assert bbox == (15, 10, 80, 110)
    assert O.shrink_bounding_box(lab == 1, bbox) == (20, 10, 79, 109)


def test_blur_against_a_direct_loop():
    rng = np.random.default_rng(3)
    x = rng.random((7, 6)).astype(np.float32)
    for kw, kh in [(1, 3), (3, 1)]:
        got = O.blur(x, (kw, kh))
        ref = np.zeros(x.shape)
        h, w = x.shape

        def r101(i, n):
            return -i if i < 0 else 2 * (n - 1) - i if i >= n else i
        for y in range(h):
            for xx in range(w):
                ref[y, xx] = sum(float(x[r101(y + dy, h), r101(xx + dx, w)]) for dy in range(-(kh // 2), kh // 2 + 1)
                                 for dx in range(-(kw // 2), kw // 2 + 1)) / (kw * kh)
        assert np.array_equal(got, ref.astype(np.float32))


def test_pickle_loader_against_the_fixture(tmp_path):
    params = omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz"))
    p = tmp_path / "system_params.pkl"
    with open(p, "wb") as fp:
        pickle.dump(params, fp, protocol=2)
    got = O.load_net_params(str(p))
    assert len(got) == 99 and all(np.array_equal(a, b) for a, b in zip(got, params))
    from audio_sheet_retrieval_amd.sheet_utils.system_detector import param_shapes
    assert [a.shape for a in got] == param_shapes()
    assert sum(a.size for a in got) == 110033


# ---- page anchor ---------------------------------------------------------------------------------------------------

STAVES = [(116, 214), (299, 393), (478, 571), (656, 760), (845, 947), (1032, 1127)]   # measured staff extents
ROW_TOL, COL_TOL = 3, 10                    # COL_TOL: the snap's own search radius


def test_page_anchor_six_systems():
    """The restatement (float32, the transposed conv in the derived orientation) on the tutorial page with the
    reference's weights finds six systems, top to bottom, each covering one measured staff: rows within ROW_TOL of
    the staff extent, columns from 39 (99 for the indented first system) to about 795 within COL_TOL."""
    page = np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]
    ps = omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz"))
    pb = omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_bar_params.npz"))
    x = O.prepare_image(page)
    sp = omr_ref.sliding_window(x, (512, 512), lambda t: omr_ref.unet_forward(t, ps, dtype=np.float32))
    bp = omr_ref.sliding_window(x, (256, 512), lambda t: omr_ref.unet_forward(t, pb, dtype=np.float32))
    systems = O.systems_from_maps(x, sp, bp)
    assert systems.shape == (6, 4, 2)
    for k, (s, (top, bottom)) in enumerate(zip(systems, STAVES)):
        assert abs(s[0, 0] - top) <= ROW_TOL and abs(s[2, 0] - bottom) <= ROW_TOL, (k, s)
        assert abs(s[0, 1] - (99 if k == 0 else 39)) <= COL_TOL and abs(s[1, 1] - 795) <= COL_TOL, (k, s)
    sheet = O.unwrap_systems(page, systems)
    assert sheet.shape == (160, int(sum(s[1, 1] - s[0, 1] for s in systems)))


# ---- loader logic --------------------------------------------------------------------------------------------------

def test_png_to_gray_as_imread(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(4)
    rgba = rng.integers(0, 256, size=(9, 11, 4), dtype=np.uint8)
    Image.fromarray(rgba, "RGBA").save(str(tmp_path / "a.png"))
    g = O.imread_gray(str(tmp_path / "a.png"))
    r, gg, b = [rgba[..., i].astype(int) for i in range(3)]
    assert g.dtype == np.uint8 and g.shape == (9, 11)
    assert np.array_equal(g, ((9797 * r + 19234 * gg + 3737 * b + 16384) >> 15).astype(np.uint8))   # alpha dropped
    gray = rng.integers(0, 256, size=(5, 6), dtype=np.uint8)
    Image.fromarray(gray, "L").save(str(tmp_path / "b.png"))
    assert np.array_equal(O.imread_gray(str(tmp_path / "b.png")), gray)


def test_unwrap_rules(capsys):
    page = (np.arange(300 * 50) % 251).astype(np.uint8).reshape(300, 50)

    def sys_at(r0, r1, c0, c1):
        return np.array([[r0, c0], [r0, c1], [r1, c1], [r1, c0]], float)

    # centred: rows 100 - 80 .. 100 + 80
    a = O.unwrap_systems(page, [sys_at(90, 110, 5, 20)])
    assert np.array_equal(a, page[20:180, 5:20])
    # clamped at the top: the window is not shifted down, the missing rows are edge-padded at the bottom
    b = O.unwrap_systems(page, [sys_at(65, 85, 0, 10)])
    assert np.array_equal(b, np.pad(page[0:155, 0:10], ((0, 5), (0, 0)), mode="edge"))
    # clamped at the bottom: max(r0, r1 - 160) does not move the window up either
    b2 = O.unwrap_systems(page, [sys_at(215, 235, 0, 10)])
    assert np.array_equal(b2, np.pad(page[145:300, 0:10], ((0, 5), (0, 0)), mode="edge"))
    # a page only 150 rows high: 10 rows edge-padded (<= 16)
    short = page[:150]
    c = O.unwrap_systems(short, [sys_at(60, 80, 0, 10)])
    assert c.shape == (160, 10) and np.array_equal(c[:150], short[:, :10]) and np.array_equal(c[150:], np.repeat(short[149:150, :10], 10, 0))
    # 140 rows: 20 missing > 16 -> skipped with the reference's message, the other system kept
    d = O.unwrap_systems(page[:140], [sys_at(60, 80, 0, 10), sys_at(60, 80, 10, 12)])
    assert d.shape == (160, 0)
    assert capsys.readouterr().out.count("Problem in system padding!!!") == 2
    # systems side by side
    e = O.unwrap_systems(page, [sys_at(90, 110, 5, 20), sys_at(150, 170, 0, 7)])
    assert e.shape == (160, 22)
