"""Seeded maps for the tests of bar and note-head detection (tests/test_omr_detect_host.py, test_gpu_omr_notes.py,
test_gpu_omr_bars.py).  Not a test module."""
import numpy as np
from scipy import ndimage

# the synthetic bar blobs and the verdict of detect_bars' filters on each (True: kept)
BAR_BLOBS = ["bar70", "bar69", "slant4.0", "slant-4.5", "slant6.0", "slant-5.5", "block", "hstroke"]
BAR_VERDICTS = dict(zip(BAR_BLOBS, [True, False, True, True, False, False, False, False]))


def _slanted(mask, r0, c0, rows, degrees, width=6):
    for i in range(rows):
        c = int(round(c0 + np.tan(np.radians(degrees)) * i))
        mask[r0 + i, c:c + width] = True


def bar_blob_masks(shape=(300, 400)):
    """{name: bool mask of `shape`} of the blobs of BAR_BLOBS, pairwise apart (no two touch)"""
    out = {}

    def new(name):
        out[name] = np.zeros(shape, bool)
        return out[name]
    new("bar70")[10:80, 20:26] = True                   # 6 wide, 70 rows: major axis 80.82
    new("bar69")[10:79, 40:46] = True                   # 69 rows: 79.67
    _slanted(new("slant4.0"), 10, 70, 120, 4.0)
    _slanted(new("slant-4.5"), 10, 110, 120, -4.5)
    _slanted(new("slant6.0"), 10, 130, 120, 6.0)
    _slanted(new("slant-5.5"), 10, 180, 120, -5.5)
    new("block")[150:240, 20:50] = True                 # 90 x 30: eccentricity 0.943
    new("hstroke")[260:264, 100:190] = True             # 4 x 90 horizontal: orientation 0
    return out


def bar_blob_map(shape=(300, 400), seed=5):
    """float64 map with the blobs of BAR_BLOBS over low noise, and the bool mask it was drawn from"""
    rng = np.random.default_rng(seed)
    mask = np.zeros(shape, bool)
    for m in bar_blob_masks(shape).values():
        mask |= m
    noise = rng.random(shape)
    # Otsu's threshold is a bin centre inside the noise: some background pixels pass it and become one-pixel blobs.
    # A quiet margin keeps them from joining the drawn blobs.
    margin = ndimage.binary_dilation(mask, structure=np.ones((3, 3), bool), iterations=2)
    return np.where(mask, 0.8 + 0.2 * noise, np.where(margin, 0.0, 0.05 * noise)), mask


def note_map(shape, seed, distance=3, quantized=False):
    """float64 map for the peak search: noise with negative values, blobs, plateaus of equal maxima, peaks exactly
    distance - 1 and distance pixels off every border, values equal to 0.5 (the default threshold) and a peak on
    every seam of the kernel's 32 x 64 tiles"""
    h, w = shape
    rng = np.random.default_rng(100 + seed)
    m = rng.random(shape) * 0.6 - 0.3
    if quantized:                                        # many ties: equal maxima inside one window
        m = np.round(m * 8) / 8
    for _ in range(max(1, h * w // 400)):                # isolated peaks, some exactly at the threshold
        r, c = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[r, c] = [0.9, 0.5, 0.75, 0.5000000000000001][int(rng.integers(0, 4))]
    for _ in range(max(1, h * w // 1500)):               # plateaus: 2 x 2 and 1 x 3 of one value
        r, c = int(rng.integers(0, max(h - 2, 1))), int(rng.integers(0, max(w - 3, 1)))
        m[r:r + 2, c:c + 2] = 0.8
        r, c = int(rng.integers(0, h)), int(rng.integers(0, max(w - 3, 1)))
        m[r, c:c + 3] = 0.85
    d = distance
    for k in (d - 1, d):                                 # just inside the excluded border and just outside it
        if 2 * k < h and 2 * k < w:
            for r, c in ((k, w // 2), (h - 1 - k, w // 3), (h // 2, k), (h // 3, w - 1 - k), (k, k), (h - 1 - k, w - 1 - k)):
                m[r, c] = 0.95
    for r in range(31, h, 32):                           # tile seams
        for rr in (r, r + 1):
            if rr < h:
                m[rr, int(rng.integers(0, w))] = 0.97
    for c in range(63, w, 64):
        for cc in (c, c + 1):
            if cc < w:
                m[int(rng.integers(0, h)), cc] = 0.96
    return m


NOTE_SHAPES = [(6, 40), (7, 7), (37, 53), (64, 64), (65, 129), (130, 257), (32, 64), (33, 65), (16, 17), (17, 200)]
