"""Staff-system detection on score pages (sheet_utils/omr.py of the reference).

The two U-Nets run on the device (asr_seg_* in include/asr_hip.h, csrc/omr_kernels.hip); what the reference does on the
host after the probability maps exist - Otsu thresholds, the vertical closing, 8-connected labelling, bounding-box
shrinking and the snap to the staff-line grid - is restated here in numpy / scipy from the published semantics of the
libraries the reference ran (scikit-image 0.13.1, OpenCV 3.1), neither of which this package needs.
"""
from __future__ import print_function

import ctypes
import pickle
from ctypes import byref, c_void_p

import numpy as np
from scipy import ndimage

SYSTEM_HEIGHT = 160          # utils/data_pools.py: height of an unrolled staff system
MIN_AREA = 50000             # detect_systems: smallest system blob

IN_F32_PREPARED, IN_F32_RAW, IN_U8_RAW = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------
# images

def prepare_image(img):
    """omr.prepare_image: float32, divided by the page maximum unless it is 0."""
    img = img.astype(np.float32)
    if img.max() != 0:
        img /= img.max()
    return img


def imread_gray(path):
    """cv2.imread(path, 0) for PNG pages, on PIL: alpha dropped, colour converted as libpng's rgb_to_gray with OpenCV's
    coefficients 0.299 / 0.587 (15-bit fixed point, truncated: 9797, 19234, blue 3737), rounded with +16384 >> 15.
    16-bit samples keep their high byte."""
    from PIL import Image
    im = Image.open(path)
    if im.mode == "P":
        im = im.convert("RGBA" if "transparency" in im.info else "RGB")
    if im.mode in ("I;16", "I;16B", "I"):
        return (np.asarray(im).astype(np.uint32) >> 8).astype(np.uint8)
    a = np.asarray(im)
    if im.mode == "1":
        return (a.astype(np.uint8) * 255)
    if im.mode in ("L",):
        return np.ascontiguousarray(a, dtype=np.uint8)
    if im.mode == "LA":
        return np.ascontiguousarray(a[..., 0], dtype=np.uint8)
    if im.mode not in ("RGB", "RGBA"):
        a = np.asarray(im.convert("RGB"))
    rgb = a[..., :3].astype(np.uint32)
    g = (9797 * rgb[..., 0] + 19234 * rgb[..., 1] + 3737 * rgb[..., 2] + 16384) >> 15
    return np.ascontiguousarray(g, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the sliding-window geometry of SegmentationNetwork._predict_proba_sliding_window

def tile_grid(h, w, th, tw, overlap=0.5):
    """(pad_top, pad_left, row_0, col_0): padding of the page to a multiple of the tile (missing // 2 top / left) and
    the tile starts in padded coordinates."""
    missing_h = int(th * np.ceil(float(h) / th) - h)
    missing_w = int(tw * np.ceil(float(w) / tw) - w)
    hp, wp = h + missing_h, w + missing_w
    row_0 = np.arange(0, hp - th + 1, int(th * (1.0 - overlap)))
    col_0 = np.arange(0, wp - tw + 1, int(tw * (1.0 - overlap)))
    return missing_h // 2, missing_w // 2, row_0, col_0


def tile_window(th, tw):
    """sqrt(outer(hamming(th), hamming(tw))), float64: the weight of every tile output"""
    return np.sqrt(np.outer(np.hamming(th), np.hamming(tw)))


# ---------------------------------------------------------------------------------------------------------------------
# restated library functions

def threshold_otsu(image, nbins=256):
    """skimage.filters.threshold_otsu (0.13.1) on a float image: np.histogram bins, the bin centre that maximises the
    between-class variance (first maximum)."""
    hist, bin_edges = np.histogram(np.asarray(image).ravel(), bins=nbins)
    bin_centers = (bin_edges[:-1] + bin_edges[1:]) / 2.
    hist = hist.astype(float)
    weight1 = np.cumsum(hist)
    weight2 = np.cumsum(hist[::-1])[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean1 = np.cumsum(hist * bin_centers) / weight1
        mean2 = (np.cumsum((hist * bin_centers)[::-1]) / weight2[::-1])[::-1]
        variance12 = weight1[:-1] * weight2[1:] * (mean1[:-1] - mean2[1:]) ** 2
    idx = np.argmax(variance12)
    return bin_centers[:-1][idx]


def peak_local_max(image, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=True):
    """skimage.feature.peak_local_max (0.13.1), indices=True, no footprint / labels / num_peaks: points equal to the
    maximum of their (2 min_distance + 1) neighbourhood (zero beyond the border), min_distance points off every border
    excluded, above max(threshold_abs or image.min(), threshold_rel * image.max()).  A constant image has no peaks.
    Order: np.nonzero's (row-major), REVERSED ("highest peak first" in that version reverses the index order)."""
    image = np.asarray(image)
    if np.all(image == image.flat[0]):
        return np.empty((0, image.ndim), np.int64)
    if type(exclude_border) == bool:
        exclude_border = min_distance if exclude_border else 0
    image_max = ndimage.maximum_filter(image, size=2 * min_distance + 1, mode="constant")
    mask = image == image_max
    if exclude_border:
        for i in range(mask.ndim):
            mask = mask.swapaxes(0, i)
            remove = 2 * exclude_border
            mask[:remove // 2] = mask[-remove // 2:] = False
            mask = mask.swapaxes(0, i)
    thresholds = [image.min() if threshold_abs is None else threshold_abs]
    if threshold_rel is not None:
        thresholds.append(threshold_rel * image.max())
    mask &= image > max(thresholds)
    coord = np.column_stack(np.nonzero(mask))
    return coord[::-1]


def blur(image, ksize):
    """cv2.blur(image, ksize=(kw, kh)) on a float32 image: box mean, BORDER_REFLECT_101, sums in float64 (OpenCV's
    sum type for float input), result float32."""
    kw, kh = ksize
    x = np.asarray(image, np.float64)
    ay, ax = kh // 2, kw // 2
    xp = np.pad(x, ((ay, kh - 1 - ay), (ax, kw - 1 - ax)), mode="reflect")
    s = np.zeros_like(x)
    for dy in range(kh):
        for dx in range(kw):
            s += xp[dy:dy + x.shape[0], dx:dx + x.shape[1]]
    return (s * (1.0 / (kw * kh))).astype(np.float32)


def close_vertical(fg, k=15):
    """cv2.morphologyEx(fg, MORPH_CLOSE, ones((k, 1))) on a 0/1 image: dilation then erosion along columns with the
    anchor at the centre and OpenCV's default border (neither dilates nor erodes: outside counts as 0 for the dilation
    and as 1 for the erosion).  uint8 0/1."""
    st = np.ones((k, 1), bool)
    d = ndimage.binary_dilation(fg.astype(bool), structure=st, border_value=0)
    e = ndimage.binary_erosion(d, structure=st, border_value=1)
    return e.astype(np.uint8)


def label8(fg):
    """skimage.measure.label(fg, neighbors=8): background 0, labels 1.. in raster order of each blob's first pixel."""
    lab, n = ndimage.label(np.asarray(fg) != 0, structure=np.ones((3, 3), int))
    return lab, n


def regionprops(label_img, n):
    """area and bbox (min_row, min_col, max_row, max_col; max exclusive) of labels 1..n, in label order"""
    areas = np.bincount(label_img.ravel(), minlength=n + 1)
    out = []
    for i, sl in enumerate(ndimage.find_objects(label_img, max_label=n)):
        if sl is None:
            continue
        out.append((i + 1, int(areas[i + 1]), (sl[0].start, sl[1].start, sl[0].stop, sl[1].stop)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# detect_systems' host steps (omr.py)

def shrink_bounding_box(fg_img, bbox):
    """OpticalMusicRecognizer._shrink_bounding_box"""
    min_row, min_col, max_row, max_col = bbox
    min_row = max(min_row, 0)
    min_col = max(min_col, 0)
    max_row = min(max_row, fg_img.shape[0] - 1)
    max_col = min(max_col, fg_img.shape[1] - 1)
    while np.mean(fg_img[min_row, min_col:max_col]) < 0.9:
        min_row += 1
    while np.mean(fg_img[max_row, min_col:max_col]) < 0.9:
        max_row -= 1
    while np.mean(fg_img[min_row:max_row, min_col]) < 0.9:
        min_col += 1
    while np.mean(fg_img[min_row:max_row, max_col]) < 0.9:
        max_col -= 1
    return min_row, min_col, max_row, max_col


def snap_system_to_grid(image, min_row, max_row, min_col, max_col):
    """omr.snap_system_to_grid, including its x-direction comparison against max_row (not max_col)."""
    image = 1.0 - image[0, 0]
    imagex = blur(image, (1, 3))
    imagey = blur(image, (3, 1))

    # y-direction
    edge_signal = imagey.mean(axis=1)
    edge_candidates = peak_local_max(edge_signal, threshold_rel=0.5)
    min_dists = np.abs(min_row - edge_candidates)
    min_idx_min = np.argmin(min_dists)
    min_dist = min_dists[min_idx_min]
    max_dists = np.abs(max_row - edge_candidates)
    min_idx_max = np.argmin(max_dists)
    max_dist = max_dists[min_idx_max]
    thresh = 10
    if min_dist < thresh and max_dist < thresh:
        min_row = edge_candidates[min_idx_min, 0]
        max_row = edge_candidates[min_idx_max, 0]

    # x-direction
    edge_signal = imagex[min_row:max_row, :].mean(axis=0)
    edge_candidates = peak_local_max(edge_signal, threshold_rel=0.5)
    min_dists = np.abs(min_col - edge_candidates)
    min_idx_min = np.argmin(min_dists)
    min_dist = min_dists[min_idx_min]
    max_dists = np.abs(max_row - edge_candidates)
    min_idx_max = np.argmin(max_dists)
    max_dist = max_dists[min_idx_max]
    if min_dist < thresh and max_dist < thresh:
        min_col = edge_candidates[min_idx_min, 0]
        max_col = edge_candidates[min_idx_max, 0]

    return min_row, max_row, min_col, max_col


def systems_from_maps(image, system_probs, bar_probs=None):
    """detect_systems after the two probability maps exist.  image: the prepared page (h, w); the maps: (h, w).
    Raises where the reference raises (IndexError when no row of the projection lies below its Otsu threshold,
    ValueError when the snap finds no edge candidate)."""
    if image.ndim == 2:
        image = image[np.newaxis, np.newaxis]
    system_probs = np.array(system_probs, copy=True)
    projection = (bar_probs if bar_probs is not None else system_probs).sum(1)

    thresh = threshold_otsu(projection)
    space_indices = np.nonzero(projection < thresh)[0]
    start_idx = prev_idx = space_indices[0]
    for idx in space_indices[1:]:
        if (idx - prev_idx) == 1:
            prev_idx = idx
        else:
            if prev_idx - start_idx > 15:
                system_probs[start_idx:prev_idx, :] = 0
            start_idx = prev_idx = idx

    fg_img = system_probs > threshold_otsu(system_probs)
    fg_img = close_vertical(fg_img, 15)

    label_img, n = label8(fg_img)
    detected_systems = np.zeros((0, 4, 2))
    for lab, area, bbox in regionprops(label_img, n):
        if area < MIN_AREA:
            continue
        min_row, min_col, max_row, max_col = shrink_bounding_box(label_img == lab, bbox)
        min_row, max_row, min_col, max_col = snap_system_to_grid(image, min_row, max_row, min_col, max_col)
        system_coords = np.zeros((4, 2))
        system_coords[0] = np.asarray([min_row, min_col])
        system_coords[1] = np.asarray([min_row, max_col])
        system_coords[2] = np.asarray([max_row, max_col])
        system_coords[3] = np.asarray([max_row, min_col])
        detected_systems = np.concatenate((detected_systems, system_coords[np.newaxis]))
    return detected_systems


def unwrap_systems(page, systems, system_height=SYSTEM_HEIGHT):
    """The unrolling loop of the tutorial and load_umc_sheets: rows centred on each system, clamped to the page,
    columns system[0, 1]:system[1, 1], edge-padded when up to 10 % of the rows are missing, skipped (with the
    reference's message) when more are; the systems side by side.  uint8 (system_height, total width)."""
    unwrapped_sheet = np.zeros((system_height, 0), dtype=np.uint8)
    for system in systems:
        r0 = int(np.mean([system[0, 0], system[2, 0]])) - system_height // 2
        r1 = r0 + system_height
        c0 = int(system[0, 1])
        c1 = int(system[1, 1])
        r0 = max(0, r0)
        r1 = min(r1, page.shape[0])
        r0 = max(r0, r1 - system_height)
        staff_img = page[r0:r1, c0:c1].astype(np.uint8)
        if staff_img.shape[0] < system_height:
            to_pad = system_height - staff_img.shape[0]
            if to_pad > (0.1 * system_height):
                print("Problem in system padding!!!")
                continue
            staff_img = np.pad(staff_img, ((0, to_pad), (0, 0)), mode="edge")
        unwrapped_sheet = np.hstack((unwrapped_sheet, staff_img))
    return unwrapped_sheet


def unroll_rows(page_shape, systems, system_height=SYSTEM_HEIGHT, with_index=False):
    """The integer rules of unwrap_systems without the copy: one (r0, r1, c0, c1, pad) per kept system - rows
    r0..r1-1, columns c0..c1-1 of the page, `pad` edge rows below them - in order; skipped systems print the
    reference's message.  Slices resolve as numpy resolves page[r0:r1, c0:c1] on a page of page_shape.
    with_index: (r0, r1, c0, c1, pad, i) with i the system's index in `systems` (the score map names a system by it)."""
    h, w = page_shape
    rows = []
    for i_system, system in enumerate(systems):
        r0 = int(np.mean([system[0, 0], system[2, 0]])) - system_height // 2
        r1 = r0 + system_height
        c0 = int(system[0, 1])
        c1 = int(system[1, 1])
        r0 = max(0, r0)
        r1 = min(r1, h)
        r0 = max(r0, r1 - system_height)
        r0, r1, _ = slice(r0, r1).indices(h)
        c0, c1, _ = slice(c0, c1).indices(w)
        n_rows, n_cols = max(0, r1 - r0), max(0, c1 - c0)
        if n_rows > system_height:
            raise ValueError("system rows %d:%d exceed the system height %d" % (r0, r1, system_height))
        to_pad = system_height - n_rows
        if to_pad > (0.1 * system_height):
            print("Problem in system padding!!!")
            continue
        if n_cols == 0:
            continue                         # an empty slice adds no column
        rows.append((r0, r1, c0, c1, to_pad, i_system) if with_index else (r0, r1, c0, c1, to_pad))
    return rows


PAGE_WIDTH = 835            # the width the OMR networks were trained on (the tutorial page is 1181 x 835)


def resized_shape(h, w, width=PAGE_WIDTH):
    """the shape scripts/prepare_umc_data.py:17-22 resizes an h x w scan to: `width` columns, rows in proportion,
    truncated - its float arithmetic restated"""
    return int(float(width) / w * h), int(width)


def _axis_sums(a, n_out):
    """a: (n_in, m) int64 -> (n_out, m): row i = sum over j of w(i, j) * a[j] with w the overlap of [i * n_in,
    (i + 1) * n_in) and [j * n_out, (j + 1) * n_out) - as differences of F(x) = n_out * P[x // n_out] +
    (x % n_out) * a[x // n_out], P the running sums of a"""
    n_in = a.shape[0]
    ext = np.concatenate([a, np.zeros((1,) + a.shape[1:], np.int64)])         # a[n_in] = 0: x = n_in * n_out
    run = np.concatenate([np.zeros((1,) + a.shape[1:], np.int64), np.cumsum(a, axis=0, dtype=np.int64)])
    x = np.arange(n_out + 1, dtype=np.int64) * n_in
    q, r = x // n_out, x % n_out
    F = n_out * run[q] + r[:, None] * ext[q]
    return F[1:] - F[:-1]


def resize_page_host(page, h_out, w_out):
    """asr_resize_pages_dev on the host (the definition in include/asr_hip.h): exact integer area resampling of a uint8
    page to h_out x w_out, in int64, in time proportional to the pixels.  The device returns the same bytes."""
    page = np.asarray(page)
    if page.ndim != 2 or page.dtype != np.uint8:
        raise ValueError("resize_page_host takes a 2-D uint8 page, got %s %s" % (page.dtype, page.shape))
    h_in, w_in = page.shape
    h_out, w_out = int(h_out), int(w_out)
    if min(h_in, w_in, h_out, w_out) < 1:
        raise ValueError("resize_page_host: %d x %d -> %d x %d" % (h_in, w_in, h_out, w_out))
    rows = _axis_sums(np.ascontiguousarray(page.T, dtype=np.int64), w_out)    # (w_out, h_in): along the width
    S = _axis_sums(np.ascontiguousarray(rows.T), h_out)                       # (h_out, w_out): along the height
    D = h_in * w_in
    return ((2 * S + D) // (2 * D)).astype(np.uint8)


def resize_pages_host(pages, width=PAGE_WIDTH):
    """every page resized to `width` columns (resized_shape) with resize_page_host"""
    return [resize_page_host(p, *resized_shape(p.shape[0], p.shape[1], width)) for p in pages]


MAX_SLOPE = 128             # the largest slope of asr_skew_estimate_dev / asr_deskew_pages_dev, in 1/1024 pixel per pixel


def _uint8_page(page, who):
    page = np.asarray(page)
    if page.ndim != 2 or page.dtype != np.uint8 or page.size == 0:
        raise ValueError("%s takes a 2-D uint8 page, got %s %s" % (who, page.dtype, page.shape))
    return page


def skew_scores_host(page, max_slope=64):
    """asr_skew_estimate_dev's scores on the host (the definition in include/asr_hip.h): int64 (2 * max_slope + 1,),
    slope k at k + max_slope - the sum of squares of the projection profile of the ink along lines of slope k / 1024.
    d_k is constant over runs of columns, so a profile is built from differences of the rows' running sums, one per
    (row, run), not from one add per pixel.  The device returns the same integers."""
    page = _uint8_page(page, "skew_scores_host")
    K = int(max_slope)
    if not 0 <= K <= MAX_SLOPE:
        raise ValueError("skew_scores_host: max_slope %d outside [0, %d]" % (K, MAX_SLOPE))
    h, w = page.shape
    run = np.zeros((w + 1, h), np.int64)                                      # run[i]: ink of the first i columns, per row
    np.cumsum(255 - page.T.astype(np.int64), axis=0, out=run[1:])
    x = np.arange(w, dtype=np.int64)
    scores = np.zeros(2 * K + 1, np.int64)
    for k in range(-K, K + 1):
        d = (k * (2 * x - (w - 1)) + 1024) >> 11
        starts = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
        ends = np.concatenate([starts[1:], [w]])
        strips = run[ends] - run[starts]                                      # (runs, h): the ink of a run, per row
        shifts = d[starts]
        dm = int(np.abs(shifts).max())
        P = np.zeros(h + 2 * dm, np.int64)                                    # P[r + dm], r = y - d
        for j, dj in enumerate(shifts):
            P[dm - dj:dm - dj + h] += strips[j]
        scores[k + K] = np.dot(P, P)
    return scores


def pick_slope(scores):
    """the slope of largest score: the candidates in the order 0, -1, +1, -2, +2, ..., replaced only on strict >"""
    scores = np.asarray(scores)
    K = (scores.size - 1) // 2
    best, top = 0, scores[K]
    for m in range(1, K + 1):
        for k in (-m, m):
            if scores[k + K] > top:
                best, top = k, scores[k + K]
    return best


def estimate_skew_host(page, max_slope=64):
    """the slope of the staves of a scanned page in 1/1024 pixel per pixel, as asr_skew_estimate_dev returns it: shearing
    the page by it (shear_page_host) makes them horizontal.  0 for a blank or ambiguous page."""
    return pick_slope(skew_scores_host(page, max_slope))


def shear_page_host(page, k, fill=255):
    """asr_deskew_pages_dev on the host (the definition in include/asr_hip.h): the page sheared by slope k / 1024 down
    its columns, then by -k / 1024 along its rows - a rotation up to a scale of 1 - (k / 1024)^2 - in integers, each pass
    rounded to uint8, `fill` outside the page.  The shape stays; k = 0 is the identity.  The device returns the same
    bytes."""
    page = _uint8_page(page, "shear_page_host")
    k, fill = int(k), int(fill)
    if abs(k) > MAX_SLOPE or not 0 <= fill <= 255:
        raise ValueError("shear_page_host: slope %d (at most %d) / fill %d (0 .. 255)" % (k, MAX_SLOPE, fill))
    h, w = page.shape
    x, y = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    t = k * (2 * x - (w - 1))
    q = t >> 11
    f = t - 2048 * q
    top, bottom = max(0, int(-q.min())), max(0, int(q.max()) + 1)
    I = np.full((top + h + bottom, w), fill, np.int64)
    I[top:top + h] = page
    rows = y[:, None] + q[None, :] + top
    A = ((2048 - f) * np.take_along_axis(I, rows, axis=0) + f * np.take_along_axis(I, rows + 1, axis=0) + 1024) >> 11
    u = -k * (2 * y - (h - 1))
    p = u >> 11
    g = (u - 2048 * p)[:, None]
    left, right = max(0, int(-p.min())), max(0, int(p.max()) + 1)
    Ap = np.full((h, left + w + right), fill, np.int64)
    Ap[:, left:left + w] = A
    cols = x[None, :] + p[:, None] + left
    out = ((2048 - g) * np.take_along_axis(Ap, cols, axis=1) + g * np.take_along_axis(Ap, cols + 1, axis=1) + 1024) >> 11
    return out.astype(np.uint8)


def deskew_page_host(page, max_slope=64, fill=255):
    """-> (the page sheared by its estimated slope, the slope): estimate_skew_host, then shear_page_host"""
    k = estimate_skew_host(page, max_slope)
    return shear_page_host(page, k, fill), k


FLATTEN_TILE = 64           # results per side of a workgroup's tile of flatten_pass_kernel (csrc/asr_kernels.h)
MAX_RADIUS = 127            # the largest radius of asr_flatten_pages_dev
FLATTEN_FLOOR = 64          # the default floor: a background darker than this is not paper


def flatten_radius(width):
    """the default radius of asr_flatten_pages_dev for a page of this width: wider than a note head, thinner than
    anything a shadow does - 13 at 835 columns, 39 at 2480"""
    return min(MAX_RADIUS, max(1, (int(width) + 32) // 64))


def _flatten_arguments(radius, floor, who):
    radius, floor = int(radius), int(floor)
    if not 1 <= radius <= MAX_RADIUS or not 0 <= floor <= 255:
        raise ValueError("%s: radius %d (1 .. %d) / floor %d (0 .. 255)" % (who, radius, MAX_RADIUS, floor))
    return radius, floor


def page_background_host(page, radius):
    """the background B of asr_flatten_pages_dev on the host (the definition in include/asr_hip.h): the grey closing of
    a uint8 page by a (2 * radius + 1)-square - the maximum over the page's radius-neighbourhood, where the outside is
    absent, then the minimum of that.  The device returns the same bytes."""
    page = _uint8_page(page, "page_background_host")
    r, _ = _flatten_arguments(radius, 0, "page_background_host")
    size = 2 * r + 1
    D = ndimage.maximum_filter(np.pad(page, r, mode="constant", constant_values=0), size=size, mode="constant", cval=0)
    B = ndimage.minimum_filter(D, size=size, mode="constant", cval=255)
    return np.ascontiguousarray(B[r:r + page.shape[0], r:r + page.shape[1]])


def flatten_page_host(page, radius=None, floor=FLATTEN_FLOOR):
    """asr_flatten_pages_dev on the host: the page divided by its background (page_background_host; radius None:
    flatten_radius of its width), 255 * P / B rounded with a half going up, where B >= max(floor, 1); the page itself
    elsewhere.  White paper (B == 255) is reproduced byte for byte.  The device returns the same bytes."""
    page = _uint8_page(page, "flatten_page_host")
    r, floor = _flatten_arguments(flatten_radius(page.shape[1]) if radius is None else radius, floor, "flatten_page_host")
    B = page_background_host(page, r).astype(np.int64)
    P = page.astype(np.int64)
    return np.where(B >= max(floor, 1), (510 * P + B) // (2 * np.maximum(B, 1)), P).astype(np.uint8)


CROP_FLOOR = 64             # the default floor of the crop: the flatten's "not paper" level
CROP_SHARE = 512            # the default share, in 1/1024: a border row is dark over half of its band


def crop_margin(width):
    """the default margin of asr_crop_estimate_dev for a page of this width: what is cut beyond a border that was found,
    the corner residue of a slightly tilted frame - 13 at 835 columns, 39 at 2480 (the rule of flatten_radius)"""
    return (int(width) + 32) // 64


def _crop_arguments(floor, share, who):
    floor, share = int(floor), int(share)
    if not 0 <= floor <= 255 or not 1 <= share <= 1024:
        raise ValueError("%s: floor %d (0 .. 255) / share %d (1 .. 1024)" % (who, floor, share))
    return floor, share


def crop_counts_host(page, floor=CROP_FLOOR):
    """asr_crop_estimate_dev's counts on the host (the definition in include/asr_hip.h) -> (row counts int32 (H,), column
    counts int32 (W,)): the pixels below `floor` of every row over the central band of the columns [W / 4, W - W / 4),
    and of every column over the central band of the rows.  The device returns the same integers."""
    page = _uint8_page(page, "crop_counts_host")
    floor, _ = _crop_arguments(floor, 1, "crop_counts_host")
    h, w = page.shape
    dark = page < floor
    return (dark[:, w // 4:w - w // 4].sum(axis=1).astype(np.int32),
            dark[h // 4:h - h // 4, :].sum(axis=0).astype(np.int32))


def _edge_run(border):
    """the length of the run of True that starts at index 0"""
    stops = np.flatnonzero(~border)
    return int(stops[0]) if stops.size else int(border.size)


def crop_rect_host(page, floor=CROP_FLOOR, share=CROP_SHARE, margin=None):
    """asr_crop_estimate_dev on the host -> ((r0, r1, c0, c1), status): the paper's rectangle inside a scanner's black
    border.  A row is a border row where 1024 * its count >= share * the band's width, a column likewise; the runs of
    border rows / columns that touch the four edges are cut off, and `margin` more (None: crop_margin of the width) on
    every side where a run was found.  Status 1 and the whole page where that leaves nothing.  The device returns the
    same integers."""
    page = _uint8_page(page, "crop_rect_host")
    floor, share = _crop_arguments(floor, share, "crop_rect_host")
    h, w = page.shape
    margin = crop_margin(w) if margin is None else int(margin)
    if margin < 0:
        raise ValueError("crop_rect_host: margin %d is negative" % margin)
    rows, cols = crop_counts_host(page, floor)
    border_rows = 1024 * rows.astype(np.int64) >= share * (w - w // 4 - w // 4)
    border_cols = 1024 * cols.astype(np.int64) >= share * (h - h // 4 - h // 4)
    top, bottom = _edge_run(border_rows), _edge_run(border_rows[::-1])
    left, right = _edge_run(border_cols), _edge_run(border_cols[::-1])
    r0, r1 = top + (margin if top else 0), h - bottom - (margin if bottom else 0)
    c0, c1 = left + (margin if left else 0), w - right - (margin if right else 0)
    if top + bottom >= h or left + right >= w or r1 - r0 < 1 or c1 - c0 < 1:
        return (0, h, 0, w), 1
    return (r0, r1, c0, c1), 0


def crop_page_host(page, floor=CROP_FLOOR, share=CROP_SHARE, margin=None):
    """asr_crop_estimate_dev + asr_crop_pages_dev on the host: the page cut to crop_rect_host's rectangle.  The device
    returns the same bytes."""
    (r0, r1, c0, c1), _ = crop_rect_host(page, floor, share, margin)
    return np.ascontiguousarray(np.asarray(page)[r0:r1, c0:c1])


class DevicePages(object):
    """uint8 pages back to back in one device buffer, as asr_seg_predict_dev (IN_U8_RAW) and asr_unroll_systems_dev
    read them: uploaded once, used by both networks and by the unroll."""

    def __init__(self, engine, pages):
        flat = [np.ascontiguousarray(p, dtype=np.uint8) for p in pages]
        for p in flat:
            if p.ndim != 2:
                raise ValueError("pages are 2-D, got shape %s" % (p.shape,))
        self.engine = engine
        self.sizes = np.asarray([p.size for p in flat], np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)[:-1]]).astype(np.int64)
        self.heights = np.asarray([p.shape[0] for p in flat], np.int32)
        self.widths = np.asarray([p.shape[1] for p in flat], np.int32)
        self.nbytes = int(self.sizes.sum())
        host = np.concatenate([p.ravel() for p in flat]) if flat else np.zeros(0, np.uint8)
        self.buf = engine.alloc(max(self.nbytes, 4)).upload(host)

    def __len__(self):
        return len(self.sizes)

    def free(self):
        self.buf.free()

    def resized(self, width=PAGE_WIDTH):
        """a new DevicePages on the same engine: every page at `width` columns (resized_shape), resampled on the device
        in one launch (asr_resize_pages_dev) - nothing is uploaded or downloaded.  A page that has the width already is
        copied by the same kernel.  This object stays valid; free both."""
        shapes = [resized_shape(int(h), int(w), width) for h, w in zip(self.heights, self.widths)]
        for i, (h, w) in enumerate(shapes):
            if h < 1 or w < 1:
                raise ValueError("page %d (%d x %d) at width %d has no rows" % (i, self.heights[i], self.widths[i], width))
        res = DevicePages.__new__(DevicePages)
        res.engine = self.engine
        res.heights = np.asarray([h for h, _ in shapes], np.int32)
        res.widths = np.asarray([w for _, w in shapes], np.int32)
        res.sizes = res.heights.astype(np.int64) * res.widths
        res.offsets = np.concatenate([[0], np.cumsum(res.sizes)[:-1]]).astype(np.int64)
        res.nbytes = int(res.sizes.sum())
        res.buf = self.engine.alloc(max(res.nbytes, 4))
        try:
            self.engine.resize_pages_dev(self.buf.ptr, self.nbytes, self.offsets, self.heights, self.widths, res.offsets,
                                         res.heights, res.widths, res.buf.ptr, res.nbytes)
        except Exception:
            res.buf.free()
            raise
        return res

    def deskewed(self, max_slope=64, slopes=None, fill=255):
        """a new DevicePages on the same engine: every page sheared so that its staves lie horizontal, in the shape it
        has (asr_skew_estimate_dev - the slopes -max_slope .. max_slope, in 1/1024 - then asr_deskew_pages_dev; with
        `slopes` those are applied and nothing is estimated).  The result carries the slopes as .slopes (int32); nothing
        else is uploaded or downloaded.  This object stays valid; free both."""
        if slopes is None:
            slopes = self.engine.skew_estimate_dev(self.buf.ptr, self.nbytes, self.offsets, self.heights, self.widths,
                                                   max_slope)
        slopes = np.ascontiguousarray(slopes, dtype=np.int32)
        if slopes.shape != (len(self),):
            raise ValueError("%d slopes for %d pages" % (slopes.size, len(self)))
        res = DevicePages.__new__(DevicePages)
        res.engine = self.engine
        res.heights, res.widths, res.sizes, res.offsets = self.heights.copy(), self.widths.copy(), self.sizes.copy(), \
            self.offsets.copy()
        res.nbytes = self.nbytes
        res.slopes = slopes
        res.buf = self.engine.alloc(max(res.nbytes, 4))
        try:
            self.engine.deskew_pages_dev(self.buf.ptr, self.nbytes, self.offsets, self.heights, self.widths, slopes,
                                         res.buf.ptr, res.nbytes, fill)
        except Exception:
            res.buf.free()
            raise
        return res

    def flattened(self, radius=None, floor=FLATTEN_FLOOR):
        """a new DevicePages on the same engine: every page divided by the grey closing of its paper, in the shape it has
        (asr_flatten_pages_dev; radius None: flatten_radius of each page's width, a number: that radius for all pages, a
        sequence: one per page).  The result carries the radii as .radii (int32); nothing is uploaded or downloaded.
        This object stays valid; free both."""
        if radius is None:
            radii = [flatten_radius(w) for w in self.widths]
        elif np.ndim(radius) == 0:
            radii = [int(radius)] * len(self)
        else:
            radii = radius
        radii = np.ascontiguousarray(radii, dtype=np.int32)
        if radii.shape != (len(self),):
            raise ValueError("%d radii for %d pages" % (radii.size, len(self)))
        res = DevicePages.__new__(DevicePages)
        res.engine = self.engine
        res.heights, res.widths, res.sizes, res.offsets = self.heights.copy(), self.widths.copy(), self.sizes.copy(), \
            self.offsets.copy()
        res.nbytes = self.nbytes
        res.radii = radii
        res.buf = self.engine.alloc(max(res.nbytes, 4))
        try:
            self.engine.flatten_pages_dev(self.buf.ptr, self.nbytes, self.offsets, self.heights, self.widths, radii,
                                          res.buf.ptr, res.nbytes, floor)
        except Exception:
            res.buf.free()
            raise
        return res

    def cropped(self, floor=CROP_FLOOR, share=CROP_SHARE, margin=None, rects=None):
        """a new DevicePages on the same engine: every page cut to the paper inside a scanner's black border
        (asr_crop_estimate_dev - the rects come to the host, they are the new shapes - then asr_crop_pages_dev; margin
        None: crop_margin of each page's width, a number: that margin for all pages, a sequence: one per page; with
        `rects`, (n, 4) rows of r0 r1 c0 c1, those are applied and nothing is estimated).  The result carries the rects
        as .rects (int32 (n, 4), in this object's coordinates) and .crop_status (int32; 1: undecided, the page is
        whole; all 0 with `rects`); the pages themselves are neither uploaded nor downloaded.  This object stays valid;
        free both."""
        n = len(self)
        if rects is None:
            if margin is None:
                margins = [crop_margin(w) for w in self.widths]
            elif np.ndim(margin) == 0:
                margins = [int(margin)] * n
            else:
                margins = margin
            margins = np.ascontiguousarray(margins, dtype=np.int32)
            if margins.shape != (n,):
                raise ValueError("%d margins for %d pages" % (margins.size, n))
            rects, status = self.engine.crop_estimate_dev(self.buf.ptr, self.nbytes, self.offsets, self.heights,
                                                          self.widths, margins, floor, share)
        else:
            rects = np.ascontiguousarray(rects, dtype=np.int32)
            if rects.shape != (n, 4):
                raise ValueError("rects of shape %s for %d pages" % (rects.shape, n))
            status = np.zeros(n, np.int32)
        res = DevicePages.__new__(DevicePages)
        res.engine = self.engine
        res.heights = (rects[:, 1] - rects[:, 0]).astype(np.int32)
        res.widths = (rects[:, 3] - rects[:, 2]).astype(np.int32)
        res.sizes = res.heights.astype(np.int64).clip(0) * res.widths.astype(np.int64).clip(0)
        res.offsets = np.concatenate([[0], np.cumsum(res.sizes)[:-1]]).astype(np.int64)
        res.nbytes = int(res.sizes.sum())
        res.rects, res.crop_status = rects, status
        res.buf = self.engine.alloc(max(res.nbytes, 4))
        try:
            self.engine.crop_pages_dev(self.buf.ptr, self.nbytes, self.offsets, self.heights, self.widths, rects,
                                       res.offsets, res.buf.ptr, res.nbytes)
        except Exception:
            res.buf.free()
            raise
        return res

    def download_page(self, i):
        """page i as a uint8 array on the host"""
        return self.engine.raw_download(self.buf.ptr + int(self.offsets[i]), (int(self.heights[i]), int(self.widths[i])),
                                        np.uint8)

    def download(self):
        """all pages as uint8 arrays on the host, in one copy"""
        flat = self.buf.download((self.nbytes,), np.uint8) if self.nbytes else np.zeros(0, np.uint8)
        return [flat[o:o + s].reshape(h, w) for o, s, h, w in zip(self.offsets, self.sizes, self.heights, self.widths)]


def resize_pages_dev(engine, pages, width=PAGE_WIDTH):
    """host pages (2-D uint8 arrays of any sizes) -> a DevicePages holding them at `width` columns: one upload of the
    raw pages, one launch.  Free it when done."""
    raw = DevicePages(engine, pages)
    try:
        return raw.resized(width)
    finally:
        raw.free()


def deskew_pages_dev(engine, pages, max_slope=64, slopes=None, fill=255):
    """host pages (2-D uint8 arrays of any sizes) -> a DevicePages holding them straightened (DevicePages.deskewed), with
    the slopes as .slopes: one upload of the raw pages.  Free it when done."""
    raw = DevicePages(engine, pages)
    try:
        return raw.deskewed(max_slope, slopes, fill)
    finally:
        raw.free()


def flatten_pages_dev(engine, pages, radius=None, floor=FLATTEN_FLOOR):
    """host pages (2-D uint8 arrays of any sizes) -> a DevicePages holding them with the paper taken out
    (DevicePages.flattened), with the radii as .radii: one upload of the raw pages.  Free it when done."""
    raw = DevicePages(engine, pages)
    try:
        return raw.flattened(radius, floor)
    finally:
        raw.free()


def crop_pages_dev(engine, pages, floor=CROP_FLOOR, share=CROP_SHARE, margin=None, rects=None):
    """host pages (2-D uint8 arrays of any sizes) -> a DevicePages holding them cut to their paper
    (DevicePages.cropped), with the rects as .rects and the statuses as .crop_status: one upload of the raw pages.  Free
    it when done."""
    raw = DevicePages(engine, pages)
    try:
        return raw.cropped(floor, share, margin, rects)
    finally:
        raw.free()


def unroll_systems_dev(dev_pages, page_rows, piece_of_page, n_pieces, system_height=SYSTEM_HEIGHT):
    """unwrap_systems + hstack for all pages of all pieces in one device call (asr_unroll_systems_dev).
    page_rows[p]: unroll_rows of page p, or None for a page that is not unrolled; piece_of_page[p]: index of the piece
    page p belongs to (pages of a piece in order).  -> (DeviceBuffer of the float32 strips, float offsets, shapes
    [(system_height, W_piece)]): piece_identification.DeviceArrays fields."""
    table, widths = [], np.zeros(n_pieces, np.int64)
    for p, rows in enumerate(page_rows):
        if rows is None:
            continue
        q = int(piece_of_page[p])
        for r0, r1, c0, c1, pad in (row[:5] for row in rows):
            table.append((p, r0, r1, c0, c1, pad, q, widths[q]))
            widths[q] += c1 - c0
    if widths.size and widths.max() > np.iinfo(np.int32).max:
        raise ValueError("a strip of %d columns is too wide" % widths.max())
    offsets = np.concatenate([[0], np.cumsum(widths * system_height)[:-1]]).astype(np.int64) if n_pieces else \
        np.zeros(0, np.int64)
    total = int(widths.sum()) * system_height
    eng = dev_pages.engine
    strips = eng.alloc(max(total * 4, 4))
    try:
        eng.unroll_systems_dev(dev_pages.buf.ptr, dev_pages.nbytes, dev_pages.offsets, dev_pages.heights,
                               dev_pages.widths, np.asarray(table, np.int32).reshape(-1, 8), system_height, offsets,
                               widths.astype(np.int32), strips.ptr, total)
    except Exception:
        strips.free()
        raise
    return strips, [int(o) for o in offsets], [(system_height, int(w)) for w in widths]


# ---------------------------------------------------------------------------------------------------------------------
# the score map: measures in strip coordinates (asr_score_map_dev; the definition is in include/asr_hip.h)

SCORE_MAP_THRESHOLD = 0.5    # a map value above this is bar line
SCORE_MAP_MIN_ROWS = 60      # a column with this many such rows in a system's band belongs to a bar line
SCORE_MAP_MAX_LINES = 64     # the default capacity: interior bar lines of one system


def strip_bar_counts_host(bar_map, r0, r1, c0, c1, threshold=SCORE_MAP_THRESHOLD):
    """count[c - c0] = the rows r in [r0, r1) with bar_map[r, c] > threshold, for the page columns c in [c0, c1):
    int64 (c1 - c0,).  A NaN is not above."""
    band = np.asarray(bar_map)[r0:r1, c0:c1]
    with np.errstate(invalid="ignore"):
        return (band > threshold).sum(axis=0).astype(np.int64)


def strip_bar_lines_host(counts, c0, min_rows=SCORE_MAP_MIN_ROWS, tol=10):
    """the boundaries B of a system whose columns c0 .. c0 + len(counts) - 1 have these counts: a bar line is a maximal
    run of columns with count >= min_rows, at (first + last) // 2; it is interior when it lies more than tol from c0
    and from c1 - 1.  -> int64 [c0, the interior lines ascending, c1]."""
    flag = np.asarray(counts) >= min_rows
    c1 = c0 + flag.size
    edge = np.diff(np.concatenate([[0], flag.astype(np.int8), [0]]))
    first, last = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1) - 1
    b = c0 + (first + last) // 2
    b = b[(b - c0 > tol) & ((c1 - 1) - b > tol)]
    return np.concatenate([[c0], b, [c1]]).astype(np.int64)


def _score_map_systems(page_rows, piece_of_page, n_pieces, page_in_piece=None):
    """the table asr_unroll_systems_dev takes, (n, 8) int32, the systems' indices on their pages and the pages' indices
    within their pieces, from unroll_rows(..., with_index=True) per page (None: a page that is not unrolled)"""
    table, index, widths = [], [], np.zeros(n_pieces, np.int64)
    first_page = {}
    auto = np.zeros(len(page_rows), np.int32)
    for p, rows in enumerate(page_rows):
        if rows is None:
            continue
        q = int(piece_of_page[p])
        auto[p] = p - first_page.setdefault(q, p)
        for row in rows:
            if len(row) != 6:
                raise ValueError("the score map takes unroll_rows(..., with_index=True)")
            r0, r1, c0, c1, pad, i = row
            table.append((p, r0, r1, c0, c1, pad, q, widths[q]))
            index.append(i)
            widths[q] += c1 - c0
    if widths.size and widths.max() > np.iinfo(np.int32).max:
        raise ValueError("a strip of %d columns is too wide" % widths.max())
    if page_in_piece is None:
        page_in_piece = auto
    return (np.asarray(table, np.int32).reshape(-1, 8), np.asarray(index, np.int32),
            np.ascontiguousarray(page_in_piece, np.int32), widths)


def score_map_host(bar_maps, page_rows, piece_of_page, n_pieces, threshold=SCORE_MAP_THRESHOLD,
                   min_rows=SCORE_MAP_MIN_ROWS, tol=None, max_lines=None, page_in_piece=None, counts=None):
    """asr_score_map_dev on the host (the definition in include/asr_hip.h).  bar_maps[p]: the bar network's map of page
    p (2-D; not read for a page whose page_rows[p] is None); page_rows[p]: unroll_rows(..., with_index=True) of page p;
    piece_of_page[p]: its piece (the pages of a piece in order; page_in_piece overrides the index counted from the
    piece's first unrolled page).  counts: instead of the maps, strip_bar_counts_host of every kept system in the
    table's order.  -> (measures (n, 8) int32 rows of x0, x1, page, system, col0, col1, row0, row1, the pieces back to
    back; piece_first (n_pieces + 1,) int32).  ValueError when a system has more than max_lines interior lines."""
    tol = BAR_MISSING_TOL if tol is None else tol
    table, index, page_in_piece, _ = _score_map_systems(page_rows, piece_of_page, n_pieces, page_in_piece)
    out, per_piece = [], np.zeros(n_pieces, np.int64)
    for i, (p, r0, r1, c0, c1, _, q, x0) in enumerate(table.tolist()):
        cnt = strip_bar_counts_host(bar_maps[p], r0, r1, c0, c1, threshold) if counts is None else np.asarray(counts[i])
        if cnt.shape != (c1 - c0,):
            raise ValueError("system %d: %d counts for columns %d:%d" % (i, cnt.size, c0, c1))
        B = strip_bar_lines_host(cnt, c0, min_rows, tol)
        if max_lines is not None and B.size - 2 > max_lines:
            raise ValueError("score_map_host: system %d (page %d, columns %d:%d) has more than max_lines = %d interior "
                             "bar lines" % (i, p, c0, c1, max_lines))
        for j in range(B.size - 1):
            out.append((x0 + B[j] - c0, x0 + B[j + 1] - c0, page_in_piece[p], index[i], B[j], B[j + 1], r0, r1))
        per_piece[q] += B.size - 1
    piece_first = np.concatenate([[0], np.cumsum(per_piece)]).astype(np.int32)
    return np.asarray(out, np.int32).reshape(-1, 8), piece_first


class DeviceMaps(object):
    """float64 probability maps of pages back to back in one device buffer, as asr_seg_predict_dev writes them: what
    detect_systems_keep_bars_dev hands on to score_map_dev.  Free it when done."""

    def __init__(self, engine, buf, heights, widths):
        self.engine, self.buf = engine, buf
        self.heights, self.widths, self.sizes, self.offsets = _map_table(heights, widths)

    def __len__(self):
        return len(self.sizes)

    def free(self):
        if self.buf is not None:
            self.buf.free()
        self.buf = None

    def download_page(self, i):
        """map i as a float64 array on the host"""
        return _download_at(self.engine, self.buf, int(self.offsets[i]) * 8,
                            int(self.sizes[i])).reshape(int(self.heights[i]), int(self.widths[i]))

    def download(self):
        """all maps as float64 arrays on the host"""
        return [self.download_page(i) for i in range(len(self))]


def upload_maps(engine, maps):
    """2-D float64 arrays -> a DeviceMaps holding them"""
    flat = [np.ascontiguousarray(m, dtype=np.float64) for m in maps]
    for m in flat:
        if m.ndim != 2:
            raise ValueError("maps are 2-D, got shape %s" % (m.shape,))
    host = np.concatenate([m.ravel() for m in flat]) if flat else np.zeros(0, np.float64)
    buf = engine.alloc(max(host.nbytes, 8)).upload(host)
    return DeviceMaps(engine, buf, [m.shape[0] for m in flat], [m.shape[1] for m in flat])


def score_map_dev(dev_maps, page_rows, piece_of_page, n_pieces, threshold=SCORE_MAP_THRESHOLD,
                  min_rows=SCORE_MAP_MIN_ROWS, tol=None, max_lines=SCORE_MAP_MAX_LINES, page_in_piece=None):
    """score_map_host for all pages of all pieces in one device call (asr_score_map_dev: three launches) on the bar
    network's maps where they are (a DeviceMaps): the same integers.  page_rows as unroll_systems_dev takes them, from
    unroll_rows(..., with_index=True).  -> (measures (n, 8) int32, piece_first (n_pieces + 1,) int32); ValueError when a
    system has more than max_lines interior bar lines."""
    tol = BAR_MISSING_TOL if tol is None else tol
    if len(page_rows) != len(dev_maps):
        raise ValueError("%d pages of rows for %d maps" % (len(page_rows), len(dev_maps)))
    table, index, page_in_piece, _ = _score_map_systems(page_rows, piece_of_page, n_pieces, page_in_piece)
    return dev_maps.engine.score_map_dev(c_void_p(dev_maps.buf.ptr), dev_maps.heights, dev_maps.widths, page_in_piece,
                                         table, index, n_pieces, threshold, min_rows, tol, max_lines)


def pairwise_sum(a):
    """np.add.reduce over a contiguous 1-D float array, restated: the order asr_systems_from_maps_dev's row sums keep
    (csrc/omr_post_kernels.hip, wave_pairwise_sum).  Below 8 elements sequential; up to 128 eight interleaved
    accumulators combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder sequentially; above, split at
    n2 = n / 2 rounded down to a multiple of 8 and recurse.  Bit-equal with a.sum() for float32 and float64."""
    n, t = a.shape[0], a.dtype.type
    if n < 8:
        res = t(0)
        for v in a:
            res = t(res + v)
        return res
    if n <= 128:
        r = [a[j] for j in range(8)]
        m = n - n % 8
        for i in range(8, m, 8):
            for j in range(8):
                r[j] = t(r[j] + a[i + j])
        res = t(t(t(r[0] + r[1]) + t(r[2] + r[3])) + t(t(r[4] + r[5]) + t(r[6] + r[7])))
        for i in range(m, n):
            res = t(res + a[i])
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return t(pairwise_sum(a[:n2]) + pairwise_sum(a[n2:]))


def row_sums(x):
    """x.sum(1) of a C-contiguous 2-D float array in the restated order (projection = maps.sum(1); with float32 and a
    division by float32(width), imagey.mean(axis=1) of the snap)"""
    return np.array([pairwise_sum(r) for r in x], dtype=x.dtype)


def column_sums(x):
    """x.sum(0) of a C-contiguous 2-D float array, restated: row after row into one accumulator per column
    (imagex[r0:r1].mean(axis=0) of the snap is this in float32, divided by float32(r1 - r0))"""
    acc = np.zeros(x.shape[1], x.dtype)
    for r in x:
        acc = acc + r
    return acc


def systems_from_maps_dev(engine, pages_ptr, in_mode, page_offsets, heights, widths, system_maps_ptr,
                          bar_maps_ptr=None, max_systems=None, system_seg=None, bar_seg=None):
    """systems_from_maps for all pages in one device call (asr_systems_from_maps_dev).  -> per page (status, corners):
    status 0 with the (n, 4, 2) float64 corner array systems_from_maps returns, or 1 / 2 / 3 with None (the host's
    IndexError / its ValueError / not decided on the device); and the number of labelling passes."""
    status, counts, systems, passes = engine.systems_from_maps_dev(
        pages_ptr, in_mode, page_offsets, heights, widths, system_maps_ptr, bar_maps_ptr, max_systems,
        system_seg, bar_seg)
    out = []
    for st, n, rows in zip(status, counts, systems):
        if st != 0:
            out.append((int(st), None))
            continue
        r = rows[:n].astype(np.float64)
        corners = np.zeros((int(n), 4, 2))
        corners[:, 0, 0] = corners[:, 1, 0] = r[:, 0]
        corners[:, 2, 0] = corners[:, 3, 0] = r[:, 1]
        corners[:, 0, 1] = corners[:, 3, 1] = r[:, 2]
        corners[:, 1, 1] = corners[:, 2, 1] = r[:, 3]
        out.append((0, corners))
    return out, passes


# ---------------------------------------------------------------------------------------------------------------------
# detect_notes' and detect_bars' host steps (omr.py)

BAR_MIN_LENGTH = 80          # detect_bars: shortest major axis of a bar blob
BAR_ANGLE_TOL = 5            # ... degrees off the vertical
BAR_MIN_ECC = 0.95           # ... smallest eccentricity
BAR_MISSING_TOL = 10         # ... a system whose outermost bar is further than this from its edge gets one added

ST_OK, ST_UNDECIDED, ST_OVERFLOW = 0, 3, 4      # asr_notes_from_map_dev / asr_bars_from_map_dev per page


def notes_from_map(note_probs, threshold_abs=0.5, min_distance=3):
    """detect_notes after the probability map exists: peak_local_max in two dimensions.  (n, 2) int64 (row, col) in
    reversed raster order."""
    return peak_local_max(note_probs, min_distance=min_distance, threshold_abs=threshold_abs).astype(np.int64)


def blob_stats(label_img, n):
    """(n, 10) int64, one row per label 1..n in label order: area, the bounding box min_row, min_col, max_row,
    max_col (max exclusive), and the raw sums sum(r), sum(c), sum(r*r), sum(c*c), sum(r*c) over the blob's pixels in
    page coordinates.  Every label 1..n must occur."""
    out = np.zeros((n, 10), np.int64)
    if n == 0:
        return out
    rr, cc = np.nonzero(label_img)
    lab = label_img[rr, cc]
    order = np.argsort(lab, kind="stable")
    rr, cc, lab = rr[order].astype(np.int64), cc[order].astype(np.int64), lab[order]
    first = np.searchsorted(lab, np.arange(1, n + 1))
    if lab.size == 0 or np.any(lab[first.clip(max=lab.size - 1)] != np.arange(1, n + 1)):
        raise ValueError("blob_stats: a label of 1..%d does not occur" % n)
    out[:, 0] = np.diff(np.append(first, lab.size))
    out[:, 1] = np.minimum.reduceat(rr, first)
    out[:, 2] = np.minimum.reduceat(cc, first)
    out[:, 3] = np.maximum.reduceat(rr, first) + 1
    out[:, 4] = np.maximum.reduceat(cc, first) + 1
    for k, v in enumerate((rr, cc, rr * rr, cc * cc, rr * cc)):
        out[:, 5 + k] = np.add.reduceat(v, first)
    return out


def bar_blob_props(stats_row):
    """(major_axis_length, orientation, eccentricity) of one blob_stats row, by the formulas of scikit-image 0.13.1's
    regionprops (inertia_tensor, inertia_tensor_eigvals, major_axis_length, orientation, eccentricity), restated from
    its published source because the package cannot be installed here (as threshold_otsu above).  With x = column and
    y = row: a = mu20 / mu00, b = -mu11 / mu00, c = mu02 / mu00.  The central second moments are formed exactly from
    the integer sums (n * sum(c*c) - sum(c)**2 and the other two in Python integers); only the division by n * n and
    what follows is float64.  This differs from scikit-image in rounding only: it subtracts a float centroid from
    every pixel first."""
    n, _, _, _, _, sr, sc, srr, scc, src = [int(v) for v in stats_row]
    nn = n * n
    a = (n * scc - sc * sc) / nn
    b = -((n * src - sr * sc) / nn)
    c = (n * srr - sr * sr) / nn
    root = np.sqrt(4 * b ** 2 + (a - c) ** 2)
    l1 = (a + c) / 2 + root / 2
    l2 = (a + c) / 2 - root / 2
    major = 4 * np.sqrt(l1)
    ecc = 0.0 if l1 == 0 else float(np.sqrt(1 - l2 / l1))
    b = -b
    if a - c == 0:
        orientation = -np.pi / 4. if b > 0 else np.pi / 4.
    else:
        orientation = -0.5 * np.arctan2(2 * b, (a - c))
    return float(major), float(orientation), ecc


def bars_from_stats(stats):
    """detect_bars' filters on blob_stats rows: (n, 2, 2) float64 [[min_row, col], [max_row, col]] of the blobs whose
    major axis is at least BAR_MIN_LENGTH, whose orientation is within BAR_ANGLE_TOL degrees of the vertical and
    whose eccentricity is at least BAR_MIN_ECC; col = mean of the box's min_col and max_col."""
    detected_bars = np.zeros((0, 2, 2))
    for row in np.asarray(stats).reshape(-1, 10):
        major, orientation, ecc = bar_blob_props(row)
        if major < BAR_MIN_LENGTH:
            continue
        if np.abs(90 - np.abs(np.degrees(orientation))) > BAR_ANGLE_TOL:
            continue
        if ecc < BAR_MIN_ECC:
            continue
        min_row, min_col, max_row, max_col = [int(v) for v in row[1:5]]
        col = np.mean([min_col, max_col])
        bar_coords = np.asarray([[min_row, col], [max_row, col]], np.float64)
        detected_bars = np.concatenate((detected_bars, bar_coords[np.newaxis]))
    return detected_bars


def bar_blobs_from_map(bar_probs):
    """detect_bars up to the region properties: Otsu of the whole map, map > t, 8-connected labels, blob_stats"""
    fg_img = bar_probs > threshold_otsu(bar_probs)
    label_img, n = label8(fg_img)
    return blob_stats(label_img, n)


def bars_from_map(bar_probs):
    """detect_bars after the probability map exists and before the alignment with the systems"""
    return bars_from_stats(bar_blobs_from_map(bar_probs))


def bars_by_systems(bars, systems):
    """OpticalMusicRecognizer._bars_by_systems: every bar goes to the system whose vertical centre is nearest to its
    own (abs of the centre difference - sklearn's Euclidean distance in one dimension without its rounding; argmin
    takes the first minimum), the bars of a system sorted by column (stable).  Raises ValueError when there is no bar
    at all while systems are given (sklearn rejects an array of 0 samples)."""
    bars, systems = np.asarray(bars, np.float64), np.asarray(systems, np.float64)
    if bars.shape[0] == 0 and systems.shape[0] > 0:
        raise ValueError("Found array with 0 sample(s) (shape=(0, 1)) while a minimum of 1 is required.")
    system_centers = systems.mean(1)[:, 0]
    bar_centers = bars.mean(1)[:, 0]
    by_system = [np.zeros((0, 2, 2))] * systems.shape[0]
    for i in range(bars.shape[0]):
        min_idx = int(np.argmin(np.abs(bar_centers[i] - system_centers)))
        by_system[min_idx] = np.vstack((by_system[min_idx], bars[i][np.newaxis]))
    for i in range(systems.shape[0]):
        by_system[i] = by_system[i][np.argsort(by_system[i][:, 0, 1], kind="stable")]
    return by_system


def align_bars_with_systems(bars, systems):
    """detect_bars' "align bars with system" block, as the reference has it: a system whose first bar is not at its
    left edge gets one there, a system whose last bar is more than BAR_MISSING_TOL off its right edge gets one there
    (stacked in FRONT of the system's bars, and both inserted bars take their second corner from the column entries
    systems[i, 3, 1] / systems[i, 2, 1] - the reference's indices), and every bar takes its system's rows.  (n, 2, 2)
    float64.  Raises IndexError for a system that receives no bar and ValueError when there are no bars at all."""
    systems = np.asarray(systems, np.float64)
    detected_bars = np.zeros((0, 2, 2))
    for i_sys, bars_i in enumerate(bars_by_systems(bars, systems)):
        s = systems[i_sys]
        if bars_i[0, 0, 1] != s[0, 1]:
            bars_i = np.vstack((np.asarray([[[s[0, 0], s[0, 1]], [s[3, 1], s[3, 1]]]]), bars_i))
        if np.abs(bars_i[0, 0, 1] - s[0, 1]) > BAR_MISSING_TOL:
            bars_i = np.vstack((np.asarray([[[s[0, 0], s[0, 1]], [s[3, 1], s[3, 1]]]]), bars_i))
        if np.abs(bars_i[-1, 0, 1] - s[1, 1]) > BAR_MISSING_TOL:
            bars_i = np.vstack((np.asarray([[[s[1, 0], s[1, 1]], [s[2, 1], s[2, 1]]]]), bars_i))
        for bar in bars_i:
            bar[0, 0] = s[0, 0]
            bar[1, 0] = s[3, 0]
            detected_bars = np.concatenate((detected_bars, bar[np.newaxis]))
    return detected_bars


def _map_table(heights, widths):
    heights = np.ascontiguousarray(heights, np.int32)
    widths = np.ascontiguousarray(widths, np.int32)
    sizes = heights.astype(np.int64) * widths
    return heights, widths, sizes, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)


def notes_from_map_dev(engine, maps_ptr, heights, widths, threshold_abs=0.5, threshold_rel=None, min_distance=3,
                       max_peaks=4096, seg=None):
    """notes_from_map for all pages in one device call (asr_notes_from_map_dev) on float64 maps that lie back to back
    on the device.  -> per page (status, coords): ST_OK with the (n, 2) int64 array of the host, ST_UNDECIDED or
    ST_OVERFLOW (more than max_peaks peaks) with None."""
    status, counts, coords = engine.notes_from_map_dev(maps_ptr, heights, widths, threshold_abs, threshold_rel,
                                                       min_distance, max_peaks, seg)
    return [(int(st), coords[p, :n].astype(np.int64) if st == 0 else None)
            for p, (st, n) in enumerate(zip(status, counts))]


def bar_blobs_from_map_dev(engine, maps_ptr, heights, widths, max_blobs=16384, seg=None):
    """bar_blobs_from_map for all pages in one device call (asr_bars_from_map_dev).  -> (per page (status, stats):
    ST_OK with the (n, 10) int64 rows of blob_stats, else None; labelling passes)."""
    status, counts, blobs, passes = engine.bars_from_map_dev(maps_ptr, heights, widths, max_blobs, seg)
    return [(int(st), blobs[p, :n].copy() if st == 0 else None)
            for p, (st, n) in enumerate(zip(status, counts))], passes


# ---------------------------------------------------------------------------------------------------------------------
# networks

def load_net_params(file_path):
    """utils/net_utils.load_net_params: the pickled list of parameter arrays (Python-2 pickles read as latin1)."""
    with open(file_path, "rb") as fp:
        try:
            return pickle.load(fp)
        except UnicodeDecodeError:
            fp.seek(0)
            return pickle.load(fp, encoding="latin1")


_ENGINES = {}


def _engine(device):
    """one context per device for all segmentation networks of the process"""
    from audio_sheet_retrieval_amd import _lib
    eng = _ENGINES.get(device)
    if eng is None or eng.ctx is None:
        eng = _ENGINES[device] = _lib.Engine("mutopia_ccal_cont", device=device)
    return eng


class SegmentationNetwork(object):
    """SegmentationNetwork(net) of the reference on the device.  `net` is a graph of system_detector.build_model() /
    bar_detector.build_model(); load() takes the reference's pickle (or a list of its 99 arrays)."""

    def __init__(self, net, device=0, print_architecture=False):
        self.net = net
        self.input_shape = (None,) + tuple(net.input_shape)
        self.device = device
        self.handle = None
        self.engine = None

    @property
    def tile_shape(self):
        return tuple(self.net.input_shape[-2:])

    def load(self, file_path):
        params = load_net_params(file_path) if isinstance(file_path, str) else list(file_path)
        self.set_params(params)

    def set_params(self, params):
        from audio_sheet_retrieval_amd import _lib
        self.close()
        arrs = [np.ascontiguousarray(np.asarray(p), dtype=np.float32) for p in params]
        eng = _engine(self.device)
        ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        sizes = np.asarray([a.size for a in arrs], np.int64)
        h = c_void_p()
        th, tw = self.tile_shape
        eng._check(eng.lib.asr_seg_create(eng.ctx, th, tw, ptrs, sizes.ctypes.data, len(arrs), byref(h)))
        self.engine, self.handle = eng, h
        win = np.ascontiguousarray(tile_window(th, tw))
        eng._check(eng.lib.asr_seg_set_window(eng.ctx, h, win.ctypes.data))
        self._lib = _lib

    def close(self):
        if self.handle is not None and self.engine is not None and self.engine.ctx is not None:
            self.engine.lib.asr_seg_destroy(self.engine.ctx, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- device call ------------------------------------------------------------------------------------------------
    def predict_pages_dev(self, pages, overlap=0.5, in_mode=IN_F32_PREPARED):
        """predict_pages with the maps left on the device.  -> (out, x, (ptr, in_mode, sizes, offs, hs, ws)): `out` the
        DeviceBuffer of the float64 maps back to back, `x` the DeviceBuffer this call uploaded the pages to (None for
        a DevicePages), and the page table asr_seg_predict_dev read.  The caller frees out and x."""
        if self.handle is None:
            raise RuntimeError("SegmentationNetwork: load() the parameters first")
        eng = self.engine
        if isinstance(pages, DevicePages):
            if pages.engine is not eng:
                raise ValueError("the pages were uploaded through another engine")
            in_mode, x = IN_U8_RAW, None
            ptr, sizes, offs, hs, ws = pages.buf.ptr, pages.sizes, pages.offsets, pages.heights, pages.widths
        else:
            dt = np.uint8 if in_mode == IN_U8_RAW else np.float32
            flat = [np.ascontiguousarray(p, dtype=dt) for p in pages]
            for p in flat:
                if p.ndim != 2:
                    raise ValueError("pages are 2-D, got shape %s" % (p.shape,))
            sizes = np.asarray([p.size for p in flat], np.int64)
            offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
            hs = np.asarray([p.shape[0] for p in flat], np.int32)
            ws = np.asarray([p.shape[1] for p in flat], np.int32)
            host = np.concatenate([p.ravel() for p in flat])
            x = eng.alloc(host.nbytes).upload(host)
            ptr = x.ptr
        out = None
        try:
            out = eng.alloc(int(sizes.sum()) * 8)
            eng._check(eng.lib.asr_seg_predict_dev(eng.ctx, self.handle, c_void_p(ptr),
                                                   in_mode, offs.ctypes.data, hs.ctypes.data, ws.ctypes.data, len(sizes),
                                                   float(overlap), c_void_p(out.ptr)))
        except Exception:
            if x is not None:
                x.free()
            if out is not None:
                out.free()
            raise
        return out, x, (ptr, in_mode, sizes, offs, hs, ws)

    def predict_pages(self, pages, overlap=0.5, in_mode=IN_F32_PREPARED):
        """float64 probability maps of a list of 2-D pages in ONE device call (every tile of every page in one forward,
        chunked under ASR_OMR_BUDGET_MB).  in_mode: IN_F32_PREPARED (float32 pages as prepare_image leaves them),
        IN_F32_RAW / IN_U8_RAW (prepare_image on the device).  `pages` may be a DevicePages (raw uint8 pages that are
        already on the device; in_mode is IN_U8_RAW then)."""
        if self.handle is None:
            raise RuntimeError("SegmentationNetwork: load() the parameters first")
        if len(pages) == 0:
            return []
        out, x, (_, _, sizes, offs, hs, ws) = self.predict_pages_dev(pages, overlap=overlap, in_mode=in_mode)
        try:
            self.engine.sync()
            res = out.download((int(sizes.sum()),), np.float64)
        finally:
            if x is not None:
                x.free()
            out.free()
        return [res[o:o + s].reshape(h, w) for o, s, h, w in zip(offs, sizes, hs, ws)]

    # -- the reference's interface ----------------------------------------------------------------------------------
    def predict_proba(self, input, squeeze=True, overlap=0.5):
        """input: (n, 1, h, w) prepared float32 (or (h, w)).  A tile-sized input goes through the network directly
        (float32 output, as theano's); any other is stitched from overlapping tiles (float64)."""
        x = np.asarray(input)
        if x.ndim == 2:
            x = x[np.newaxis, np.newaxis]
        maps = self.predict_pages([img[0] for img in x.astype(np.float32)], overlap=overlap)
        proba = np.stack(maps)[:, np.newaxis]
        if x.shape[-2:] == self.tile_shape:
            proba = proba.astype(np.float32)
        if squeeze:
            proba = proba.squeeze()
        return proba

    def predict(self, input, thresh=0.5):
        P = self.predict_proba(input, squeeze=False)
        if P.shape[1] == 1:
            return (P > thresh).squeeze()
        return np.argmax(P, axis=1).squeeze()


class OpticalMusicRecognizer(object):
    """Score segmentation networks (omr.OpticalMusicRecognizer): system, bar and note-head detection."""

    def __init__(self, note_detector=None, system_detector=None, bar_detector=None):
        self.note_detector = note_detector
        self.system_detector = system_detector
        self.bar_detector = bar_detector

    def detect_systems(self, image, verbose=False):
        """(n_systems, 4, 2) float64 corners (row, col): top-left, top-right, bottom-right, bottom-left"""
        img = image[0, 0] if image.ndim == 4 else image
        system_probs = self.system_detector.predict_proba(img[np.newaxis, np.newaxis])
        bar_probs = self.bar_detector.predict_proba(img[np.newaxis, np.newaxis]) if self.bar_detector else None
        return systems_from_maps(img, system_probs, bar_probs)

    def detect_systems_pages(self, pages, in_mode=IN_F32_PREPARED, prepared=None, dev_pages=None):
        """detect_systems for many pages: one device call per network.  pages: 2-D arrays (prepared float32, or raw
        uint8 with in_mode=IN_U8_RAW).  Returns one entry per page: the corner array, or the exception the reference's
        detect_systems would have raised on that page.  dev_pages: the same raw uint8 pages as a DevicePages - the
        networks read them there instead of uploading `pages` once each."""
        if dev_pages is not None and (in_mode != IN_U8_RAW or len(dev_pages) != len(pages)):
            raise ValueError("dev_pages goes with the same number of raw uint8 pages (in_mode=IN_U8_RAW)")
        src = pages if dev_pages is None else dev_pages
        sys_maps = self.system_detector.predict_pages(src, in_mode=in_mode)
        bar_maps = self.bar_detector.predict_pages(src, in_mode=in_mode) if self.bar_detector else [None] * len(pages)
        out = []
        for i, page in enumerate(pages):
            img = prepare_image(page) if in_mode != IN_F32_PREPARED else page
            sp, bp = sys_maps[i], bar_maps[i]
            if page.shape == self.system_detector.tile_shape:
                sp = sp.astype(np.float32)
            if bp is not None and page.shape == self.bar_detector.tile_shape:
                bp = bp.astype(np.float32)
            try:
                out.append(systems_from_maps(img, sp, bp))
            except Exception as e:          # the reference's callers catch every exception of detect_systems
                out.append(e)
        return out

    def detect_systems_pages_dev(self, pages, in_mode=IN_U8_RAW, dev_pages=None):
        """detect_systems_pages with the post-processing on the device as well (asr_systems_from_maps_dev): both
        networks write their maps into device buffers, one more call turns them into system corners, and one small
        download brings those back.  Returns exactly what detect_systems_pages returns - per page the (n, 4, 2)
        float64 corner array, or an IndexError / ValueError instance.  Pages the device does not decide (status 3: a
        page of a network's tile size, a NaN in a map, a shrink loop that leaves its blob, ...) go through
        systems_from_maps on the host, their maps alone downloaded; self.last_fallback_pages lists their indices.
        The device restates np.histogram's bin rule as numpy >= 2 computes it (checked with 2.2.6); under numpy 1.x
        the equality with detect_systems_pages is not established."""
        return self._detect_systems_dev(pages, in_mode, dev_pages, False)[0]

    def detect_systems_keep_bars_dev(self, pages, in_mode=IN_U8_RAW, dev_pages=None):
        """detect_systems_pages_dev that hands the bar network's maps on instead of freeing them: -> (what
        detect_systems_pages_dev returns, a DeviceMaps of the bar maps of all pages - also of those the host decided -
        or None without pages).  The score map (score_map_dev) reads them once the unroll rows are known, so the bar
        network runs once.  The caller frees the DeviceMaps."""
        if self.bar_detector is None:
            raise ValueError("detect_systems_keep_bars_dev needs a bar network")
        return self._detect_systems_dev(pages, in_mode, dev_pages, True)

    def _detect_systems_dev(self, pages, in_mode, dev_pages, keep_bar_maps):
        if dev_pages is not None and (in_mode != IN_U8_RAW or len(dev_pages) != len(pages)):
            raise ValueError("dev_pages goes with the same number of raw uint8 pages (in_mode=IN_U8_RAW)")
        self.last_fallback_pages = []
        self.last_label_passes = 0
        if len(pages) == 0:
            return [], None
        sysd, bard = self.system_detector, self.bar_detector
        eng = sysd.engine
        if bard is not None and bard.engine is not eng:
            raise ValueError("both networks must live on one engine")
        own = None
        if dev_pages is None:
            if in_mode == IN_U8_RAW:                 # upload once for both networks and the post-processing
                own = dev_pages = DevicePages(eng, pages)
        src = pages if dev_pages is None else dev_pages
        sys_out = bar_out = x_sys = x_bar = None
        try:
            sys_out, x_sys, (ptr, mode, sizes, offs, hs, ws) = sysd.predict_pages_dev(src, in_mode=in_mode)
            if bard is not None:
                bar_out, x_bar, _ = bard.predict_pages_dev(src, in_mode=in_mode)
            decided, self.last_label_passes = systems_from_maps_dev(
                eng, c_void_p(ptr), mode, offs, hs, ws, c_void_p(sys_out.ptr),
                c_void_p(bar_out.ptr) if bar_out is not None else None, None, sysd.handle,
                bard.handle if bard is not None else None)
            out = []
            for i, (st, corners) in enumerate(decided):
                if st == 0:
                    out.append(corners)
                elif st == 1:
                    out.append(IndexError("index 0 is out of bounds for axis 0 with size 0"))
                elif st == 2:
                    out.append(ValueError("attempt to get argmin of an empty sequence"))
                else:
                    self.last_fallback_pages.append(i)
                    page = pages[i]
                    n, o = int(sizes[i]), int(offs[i]) * 8
                    shape = (int(hs[i]), int(ws[i]))
                    sp = _download_at(eng, sys_out, o, n).reshape(shape)
                    bp = _download_at(eng, bar_out, o, n).reshape(shape) if bar_out is not None else None
                    img = prepare_image(page) if in_mode != IN_F32_PREPARED else page
                    if shape == sysd.tile_shape:
                        sp = sp.astype(np.float32)
                    if bp is not None and shape == bard.tile_shape:
                        bp = bp.astype(np.float32)
                    try:
                        out.append(systems_from_maps(img, sp, bp))
                    except Exception as e:
                        out.append(e)
            kept = None
            if keep_bar_maps:
                kept, bar_out = DeviceMaps(eng, bar_out, hs, ws), None
            return out, kept
        finally:
            for b in (sys_out, bar_out, x_sys, x_bar):
                if b is not None:
                    b.free()
            if own is not None:
                own.free()

    # -- bars and note heads ----------------------------------------------------------------------------------------
    def detect_notes(self, image, threshold_abs=0.5, min_distance=3):
        """(n, 2) int64 (row, col) of the note heads: the local maxima of the note network's map"""
        img = image[0, 0] if image.ndim == 4 else image
        note_probs = self.note_detector.predict_proba(img[np.newaxis, np.newaxis])
        return notes_from_map(note_probs, threshold_abs=threshold_abs, min_distance=min_distance)

    def detect_bars(self, image, systems=None):
        """(n, 2, 2) float64 [[min_row, col], [max_row, col]] of the bar lines; with `systems` (detect_systems'
        corners) aligned to them as align_bars_with_systems does."""
        img = image[0, 0] if image.ndim == 4 else image
        bars = bars_from_map(self.bar_detector.predict_proba(img[np.newaxis, np.newaxis]))
        return bars if systems is None else align_bars_with_systems(bars, systems)

    def _maps_pages(self, net, pages, in_mode, dev_pages):
        if dev_pages is not None and (in_mode != IN_U8_RAW or len(dev_pages) != len(pages)):
            raise ValueError("dev_pages goes with the same number of raw uint8 pages (in_mode=IN_U8_RAW)")
        maps = net.predict_pages(pages if dev_pages is None else dev_pages, in_mode=in_mode)
        return [m.astype(np.float32) if m.shape == net.tile_shape else m for m in maps]

    def detect_notes_pages(self, pages, in_mode=IN_F32_PREPARED, dev_pages=None, threshold_abs=0.5, min_distance=3):
        """detect_notes for many pages: one device call for the network, notes_from_map per page.  One entry per
        page: the coordinate array, or the exception the host steps raised on it."""
        out = []
        for m in self._maps_pages(self.note_detector, pages, in_mode, dev_pages):
            try:
                out.append(notes_from_map(m, threshold_abs=threshold_abs, min_distance=min_distance))
            except Exception as e:
                out.append(e)
        return out

    def detect_bars_pages(self, pages, systems=None, in_mode=IN_F32_PREPARED, dev_pages=None):
        """detect_bars for many pages: one device call for the network, bars_from_map (and, with systems[i] given for
        page i, align_bars_with_systems) per page.  One entry per page: the bar array, or the exception instance."""
        out = []
        for i, m in enumerate(self._maps_pages(self.bar_detector, pages, in_mode, dev_pages)):
            try:
                bars = bars_from_map(m)
                if systems is not None and systems[i] is not None:
                    bars = align_bars_with_systems(bars, systems[i])
                out.append(bars)
            except Exception as e:
                out.append(e)
        return out

    def _maps_dev(self, net, pages, in_mode, dev_pages, post):
        """the network's maps left on the device, post(engine, out, heights, widths) -> per page (status, result or
        None), and the host path - post given one downloaded map - for the pages the device did not decide"""
        if dev_pages is not None and (in_mode != IN_U8_RAW or len(dev_pages) != len(pages)):
            raise ValueError("dev_pages goes with the same number of raw uint8 pages (in_mode=IN_U8_RAW)")
        self.last_fallback_pages = []
        if len(pages) == 0:
            return []
        out = x = None
        try:
            out, x, (_, _, sizes, _, hs, ws) = net.predict_pages_dev(pages if dev_pages is None else dev_pages,
                                                                     in_mode=in_mode)
            eng = net.engine
            _, _, _, map_offs = _map_table(hs, ws)
            res = []
            for i, (st, val) in enumerate(post(eng, out, hs, ws)):
                if st != 0:
                    self.last_fallback_pages.append(i)
                    m = _download_at(eng, out, int(map_offs[i]) * 8, int(sizes[i])).reshape(int(hs[i]), int(ws[i]))
                    if m.shape == net.tile_shape:
                        m = m.astype(np.float32)
                    val = m
                res.append((st, val))
            return res
        finally:
            for b in (out, x):
                if b is not None:
                    b.free()

    def detect_notes_pages_dev(self, pages, in_mode=IN_U8_RAW, dev_pages=None, threshold_abs=0.5, min_distance=3,
                               max_peaks=4096):
        """detect_notes_pages with the peak search on the device as well (asr_notes_from_map_dev): the map stays
        there and one small download brings the coordinates back.  Returns exactly what detect_notes_pages returns.
        Pages the device does not decide (a page of the tile size, a NaN in the map, more than max_peaks peaks) go
        through notes_from_map on the host, their map alone downloaded; self.last_fallback_pages lists them."""
        net = self.note_detector

        def post(eng, out, hs, ws):
            return notes_from_map_dev(eng, c_void_p(out.ptr), hs, ws, threshold_abs, None, min_distance, max_peaks,
                                      net.handle)
        res = []
        for st, val in self._maps_dev(net, pages, in_mode, dev_pages, post):
            try:
                res.append(val if st == 0 else notes_from_map(val, threshold_abs=threshold_abs,
                                                              min_distance=min_distance))
            except Exception as e:
                res.append(e)
        return res

    def detect_bars_pages_dev(self, pages, systems=None, in_mode=IN_U8_RAW, dev_pages=None, max_blobs=16384):
        """detect_bars_pages with threshold, labelling and the blob statistics on the device (asr_bars_from_map_dev);
        the filters and the alignment are the host path's own functions, bars_from_stats and align_bars_with_systems,
        on the downloaded integers.  Returns exactly what detect_bars_pages returns; undecided pages go through the
        host path (self.last_fallback_pages).  The bar network runs here again even when detect_systems_pages_dev
        ran it just before: that call frees its maps."""
        net = self.bar_detector
        self.last_label_passes = 0

        def post(eng, out, hs, ws):
            decided, self.last_label_passes = bar_blobs_from_map_dev(eng, c_void_p(out.ptr), hs, ws, max_blobs,
                                                                     net.handle)
            return decided
        res = []
        for i, (st, val) in enumerate(self._maps_dev(net, pages, in_mode, dev_pages, post)):
            try:
                bars = bars_from_stats(val) if st == 0 else bars_from_map(val)
                if systems is not None and systems[i] is not None:
                    bars = align_bars_with_systems(bars, systems[i])
                res.append(bars)
            except Exception as e:
                res.append(e)
        return res


def _download_at(engine, buf, byte_offset, n_doubles):
    """n_doubles float64 values at byte_offset of a DeviceBuffer"""
    out = np.empty(n_doubles, np.float64)
    engine._check(engine.lib.asr_dev_download(engine.ctx, out.ctypes.data, c_void_p(buf.ptr + byte_offset), out.nbytes))
    return out
