"""Seeded pages and probability maps for the tests of asr_systems_from_maps_dev (tests/test_gpu_omr_post.py): maps built
on the host - rectangles, ragged, C-shaped and spiral blobs over noise - and synthetic pages with staff-like lines and
bar lines, so that snap_system_to_grid has edge candidates.  Not a test module."""
import numpy as np

SCENARIOS = ["plain", "ragged", "c_shape", "spiral", "area_edge", "gaps", "borders", "same_row", "diagonal", "mixed"]


def _rect(mask, r0, r1, c0, c1):
    mask[max(r0, 0):r1, max(c0, 0):c1] = True


def _spiral(mask, r0, c0, size_r, size_c, arm=22, gap=20):
    """a rectangular spiral of `arm`-thick strokes separated by `gap` (> 15: the closing does not join them)"""
    top, left, bottom, right = r0, c0, r0 + size_r, c0 + size_c
    step = arm + gap
    first = True
    while bottom - top > 2 * arm and right - left > 2 * arm:
        mask[top:top + arm, left if first else left - step:right] = True       # top stroke (joins the previous ring)
        mask[top:bottom, right - arm:right] = True                              # right
        mask[bottom - arm:bottom, left:right] = True                            # bottom
        mask[top + step:bottom, left:left + arm] = True                         # left, open at the top
        top += step; left += step; bottom -= step; right -= step
        first = False


def make_case(seed):
    """-> dict(page uint8 (h, w), system float64 (h, w), bar float64 (h, w) or None, scenario)"""
    rng = np.random.default_rng(1000 + seed)
    scenario = SCENARIOS[seed % len(SCENARIOS)]
    h = int(rng.integers(720, 980))
    w = int(rng.integers(900, 1150))
    if seed % 7 == 3:
        w = [835, 1030, 1181][seed % 3]                                          # widths of real scans
    mask = np.zeros((h, w), bool)
    systems = []                                                                 # (r0, r1, c0, c1) for the page's lines

    def stack(gaps, heights, c0, c1, top):
        r = top
        for g, hh in zip(gaps, heights):
            r += g
            if r + hh > h:
                break
            _rect(mask, r, r + hh, c0, c1)
            systems.append((r, r + hh, c0, c1))
            r += hh

    c0 = int(rng.integers(30, 80))
    c1 = w - int(rng.integers(30, 80))
    if scenario in ("plain", "ragged", "mixed"):
        n = int(rng.integers(2, 5))
        stack([int(rng.integers(30, 90)) for _ in range(n)], [int(rng.integers(100, 140)) for _ in range(n)], c0, c1,
              int(rng.integers(0, 30)))
        if scenario != "plain":
            for (r0, r1, a, b) in systems:                                       # ragged left / right ends
                for r in range(r0, r1):
                    mask[r, a:a + int(rng.integers(0, 12))] = False
                    mask[r, b - int(rng.integers(0, 12)):b] = False
        if scenario == "mixed":                                                  # small blobs that are dropped
            for _ in range(6):
                r, c = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
                if not mask[max(r - 20, 0):r + 60, max(c - 2, 0):c + 42].any():
                    _rect(mask, r, r + 30, c, c + 40)
    elif scenario == "c_shape":
        stack([40, 60], [130, 150], c0, c1, 10)
        for (r0, r1, a, b) in systems:
            mask[r0 + 40:r1 - 40, b - int(rng.integers(20, 60)):b] = False       # a notch: the right side shrinks
    elif scenario == "spiral":
        _spiral(mask, 30, c0, min(h - 250, 520), c1 - c0)
        systems.append((30, 30 + min(h - 250, 520), c0, c1))
        stack([0], [120], c0, c1, h - 170)
    elif scenario == "area_edge":
        # exactly MIN_AREA (kept) and MIN_AREA - 1 (dropped): 100 x 500 and the same without a corner pixel
        stack([30], [100], 100, 600, 0)
        stack([40], [100], 120, 620, 140)
        mask[systems[1][0], 120] = False
        stack([50], [120], c0, c1, 300)
    elif scenario == "gaps":
        g = [15, 16, 17]
        rng.shuffle(g)
        stack([int(rng.integers(20, 60))] + g, [105, 100, 110, 100], c0, c1, 0)
    elif scenario == "borders":
        _rect(mask, 0, 110, 0, w - 200); systems.append((0, 110, 0, w - 200))                   # top and left
        _rect(mask, 200, 320, 150, w); systems.append((200, 320, 150, w))                       # right
        _rect(mask, h - 115, h, 0, w); systems.append((h - 115, h, 0, w))                       # bottom, left, right
    elif scenario == "same_row":
        mid = w // 2
        top = int(rng.integers(20, 60))
        _rect(mask, top, top + 135, c0, mid - 10); systems.append((top, top + 135, c0, mid - 10))
        _rect(mask, top, top + 150, mid + 10, c1); systems.append((top, top + 150, mid + 10, c1))
        stack([60], [120], c0, c1, top + 150)
    elif scenario == "diagonal":
        top = int(rng.integers(50, 90))
        _rect(mask, top, top + 120, c0 + 30, c1); systems.append((top, top + 120, c0 + 30, c1))
        _rect(mask, top - 28, top, c0 + 2, c0 + 30)                              # touches the big blob's corner only
        stack([70], [125], c0, c1, top + 120)
        _rect(mask, h - 60, h - 30, c0, c0 + 30)
        _rect(mask, h - 30, h - 2, c0 + 30, c0 + 70)                             # two small ones joined diagonally

    noise = rng.random((h, w))
    system = np.where(mask, 0.82 + 0.17 * noise, 0.08 * noise)
    if scenario == "area_edge":                  # a quiet margin: the two areas are exactly what was drawn
        for (r0, r1, a, b) in systems[:2]:
            win = (slice(max(r0 - 20, 0), r1 + 20), slice(max(a - 20, 0), b + 20))
            system[win] = np.where(mask[win], system[win], 0.0)
    bar = None
    if (seed // len(SCENARIOS)) % 2:             # every scenario with and without the bar map
        bar = 0.05 * rng.random((h, w))
        for (r0, r1, a, b) in systems:
            for x in range(max(a, 0) + 5, min(b, w) - 5, 90):
                bar[r0 + 3:r1 - 3, x:x + 6] = 0.8 + 0.2 * rng.random((r1 - r0 - 6, 6))

    page = np.full((h, w), 250, np.uint8)
    for (r0, r1, a, b) in systems:
        off = int(rng.integers(2, 14))                                           # some snap (< 10), some do not
        a, b = max(a, 2), min(b, w - 2)
        lines = np.linspace(r0 + off, r1 - off, 10).astype(int)
        for y in lines:
            if 1 <= y < h - 1:
                page[y, a:b] = 20
        xo = int(rng.integers(0, 13))
        for x in (a + xo, b - 1 - xo):
            if 1 <= x < w - 1:
                page[max(r0, 1):min(r1, h - 1), x:x + 2] = 10
    page = np.clip(page.astype(int) + rng.integers(-5, 6, size=page.shape), 0, 255).astype(np.uint8)
    return dict(page=page, system=system, bar=bar, scenario=scenario)


N_CASES = 40
