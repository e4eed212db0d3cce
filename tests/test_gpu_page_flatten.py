"""GPU: the paper of scanned pages (asr_flatten_pages_dev, csrc/page_flatten_kernels.hip) - the flattened page and the
background byte for byte against the host restatements sheet_utils/omr.flatten_page_host / page_background_host
(tests/test_page_flatten_host.py holds those against the definition), the bytes between the pages through a guard pattern,
the chunking, the argument checks, and DevicePages.flattened / load_umc_scans end to end on the shaded tutorial page."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
from test_gpu_page_deskew import recognizer  # noqa: E402,F401  (the real weights from tests/golden)
from test_page_flatten_host import shaded  # noqa: E402

MODEL = "mutopia_ccal_cont"
GUARD = 0xA5
GAP = 5


def _mixed_shapes():
    """(h, w, radius): the smallest pages, a window that covers the page, every width below a dword and past two, and
    one tile less, one tile, one tile more and two tiles and one along each axis"""
    from audio_sheet_retrieval_amd.sheet_utils.omr import FLATTEN_TILE as T
    shapes = [(1, 1, 1), (1, 300, 2), (300, 1, 13), (17, 9, 127)]
    shapes += [(5, w, (1, 2, 13, 127)[w % 4]) for w in range(1, 10)]
    shapes += [(T - 1, 2 * T + 1, 13), (T, T + 1, 2), (T + 1, T - 1, 1), (2 * T + 1, T, 13), (T, T, 127), (T + 1, T + 1, 13)]
    return shapes


@pytest.fixture(scope="module")
def eng():
    from audio_sheet_retrieval_amd import _lib
    engine = _lib.Engine(MODEL, device=0)
    yield engine
    engine.close()


@pytest.fixture(scope="module")
def mixed():
    """random pages, their radii and, computed once, (background, flattened at floor 64) on the host"""
    from audio_sheet_retrieval_amd.sheet_utils.omr import flatten_page_host, page_background_host
    rng = np.random.default_rng(29)
    shapes = _mixed_shapes()
    pages = [rng.integers(0, 256, (h, w), dtype=np.uint8) for h, w, _ in shapes]
    radii = [r for _, _, r in shapes]
    assert {1, 2, 13, 127} == set(radii)
    return pages, radii, [(page_background_host(p, r), flatten_page_host(p, r, 64)) for p, r in zip(pages, radii)]


class Layout(object):
    """pages in one buffer, GAP guard bytes before, between and after them: offsets of every alignment"""

    def __init__(self, eng, pages):
        self.eng, self.pages = eng, pages
        self.sizes = np.asarray([p.size for p in pages], np.int64)
        self.offs = np.concatenate([[0], np.cumsum(self.sizes + GAP)[:-1]]).astype(np.int64) + GAP
        self.nbytes = int(self.offs[-1] + self.sizes[-1]) + GAP
        self.heights, self.widths = [p.shape[0] for p in pages], [p.shape[1] for p in pages]
        host = np.full(self.nbytes, GUARD, np.uint8)
        for o, p in zip(self.offs, pages):
            host[o:o + p.size] = p.ravel()
        self.buf = eng.alloc(self.nbytes).upload(host)

    def _split(self, flat):
        rest = np.ones(self.nbytes, bool)
        outs = []
        for o, p in zip(self.offs, self.pages):
            outs.append(flat[o:o + p.size].reshape(p.shape))
            rest[o:o + p.size] = False
        assert rest.sum() == GAP * (len(self.pages) + 1) and np.all(flat[rest] == GUARD)      # no byte outside a page
        return outs

    def flatten(self, radii, floor=64, background=True):
        """-> (flattened pages, backgrounds or None); asserts that every other byte of both buffers kept the guard"""
        guard = np.full(self.nbytes, GUARD, np.uint8)
        out = self.eng.alloc(self.nbytes).upload(guard)
        bg = self.eng.alloc(self.nbytes).upload(guard) if background else None
        try:
            self.eng.flatten_pages_dev(self.buf.ptr, self.nbytes, self.offs, self.heights, self.widths, radii, out.ptr,
                                       self.nbytes, floor, bg.ptr if background else None)
            outs = self._split(out.download((self.nbytes,), np.uint8))
            bgs = self._split(bg.download((self.nbytes,), np.uint8)) if background else None
        finally:
            out.free()
            if background:
                bg.free()
        return outs, bgs

    def free(self):
        self.buf.free()


def _same(got, want, what):
    assert np.array_equal(got, want), (what, got.shape, np.argwhere(got != want)[:4].tolist())


def test_a_mixed_batch_equals_the_host(eng, mixed):
    pages, radii, want = mixed
    lay = Layout(eng, pages)
    try:
        assert {int(o) % 4 for o in lay.offs} == {0, 1, 2, 3}
        outs, bgs = lay.flatten(radii)
        for i, (page, r) in enumerate(zip(pages, radii)):
            _same(bgs[i], want[i][0], ("background", r))
            _same(outs[i], want[i][1], ("flattened", r))
        # 17 x 9 at radius 127: every window covers the page, yet B is not the page maximum - a window that reaches the
        # page over a corner holds that corner alone, so the closing keeps the four corners (and B >= P everywhere)
        corners = ([0, 0, -1, -1], [0, -1, 0, -1])
        assert radii[3] == 127 and np.array_equal(bgs[3][corners], pages[3][corners]) and np.all(bgs[3] >= pages[3])
        alone, none = lay.flatten(radii, background=False)            # background_dev = NULL: the same pages
        assert none is None
        for a, b in zip(alone, outs):
            _same(a, b, "without the background")
    finally:
        lay.free()


def test_a_batch_in_chunks_gives_the_same(eng, mixed, monkeypatch):
    """D of a page is (h + 2r) x (w + 2r) bytes - 71 KB for 17 x 9 at radius 127, 101 KB for 64 x 64: the batch twelve
    times over is more than 4 MB of D, so a budget of 1 MB cuts it into five chunks or more"""
    pages, radii, want = mixed
    reps = 12
    assert sum((p.shape[0] + 2 * r) * (p.shape[1] + 2 * r) for p, r in zip(pages, radii)) * reps > 4 << 20
    lay = Layout(eng, pages * reps)
    try:
        monkeypatch.setenv("ASR_OMR_BUDGET_MB", "1")
        outs, bgs = lay.flatten(radii * reps)
        monkeypatch.delenv("ASR_OMR_BUDGET_MB")
        for i in range(len(pages) * reps):
            _same(bgs[i], want[i % len(pages)][0], ("background", i))
            _same(outs[i], want[i % len(pages)][1], ("flattened", i))
    finally:
        lay.free()


def _content_pages():
    h, w = 70, 90
    y, x = np.mgrid[0:h, 0:w]
    dot = np.full((h, w), 255, np.uint8)
    dot[33, 64] = 7
    hole = np.zeros((h, w), np.uint8)
    hole[0, w - 1] = 255
    ramp = shaded(np.full((h, w), 255, np.uint8))
    level = np.full((h, w), 100, np.uint8)
    level[10:12, 20:40] = 31
    return [np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), dot, hole,
            (((y + x) % 2) * 255).astype(np.uint8), (((y // 3 + x // 5) % 2) * 200 + 20).astype(np.uint8),
            ramp, np.ascontiguousarray(ramp[::-1]), np.ascontiguousarray(ramp[:, ::-1]),
            np.ascontiguousarray(ramp[::-1, ::-1]), level]


@pytest.mark.parametrize("floor", [0, 64, 100, 101, 255])
def test_contents_and_floors_equal_the_host(eng, floor):
    """blank, one pixel, checkerboards, the four border ramps, a page whose background is 100 everywhere (divided at
    floor 100, left alone at 101), each at the radii 1, 2 and 13"""
    from audio_sheet_retrieval_amd.sheet_utils.omr import flatten_page_host, page_background_host
    pages = _content_pages()
    lay = Layout(eng, pages * 3)
    radii = [1] * len(pages) + [2] * len(pages) + [13] * len(pages)
    try:
        outs, bgs = lay.flatten(radii, floor)
        for i, r in enumerate(radii):
            page = pages[i % len(pages)]
            _same(bgs[i], page_background_host(page, r), ("background", i, r))
            _same(outs[i], flatten_page_host(page, r, floor), ("flattened", i, r, floor))
        ramps = [outs[2 * len(pages) + j] for j in (6, 7, 8, 9)]
        level = outs[len(pages) - 1]
    finally:
        lay.free()
    if floor <= 64:
        assert all(np.all(r == 255) for r in ramps)                 # a shadow is gone up to every border
    if floor == 100:
        assert level[0, 0] == 255 and level[10, 20] == (510 * 31 + 100) // 200
    if floor == 101:
        _same(level, pages[-1], "B == floor - 1")


def test_a_300_dpi_page_equals_the_host(eng):
    from audio_sheet_retrieval_amd.sheet_utils.omr import flatten_page_host, flatten_radius, page_background_host
    page = np.random.default_rng(300).integers(0, 256, (3508, 2480), dtype=np.uint8)
    page[500:3000, 300:2200] |= 0xC0                                 # a lighter field: the division takes many values
    assert flatten_radius(2480) == 39
    lay = Layout(eng, [page])
    try:
        outs, bgs = lay.flatten([39])
        _same(bgs[0], page_background_host(page, 39), "background")
        _same(outs[0], flatten_page_host(page), "flattened")
    finally:
        lay.free()


def test_invalid_arguments_launch_nothing(eng):
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils.omr import flatten_page_host, page_background_host
    page = np.random.default_rng(3).integers(0, 256, (40, 30), dtype=np.uint8)
    guard = np.full(1200, GUARD, np.uint8)
    d_in = eng.alloc(1200).upload(page)
    d_out = eng.alloc(1200).upload(guard)
    d_bg = eng.alloc(1200).upload(guard)

    def flatten(pages_bytes=1200, off=0, h=40, w=30, r=3, floor=64, out_bytes=1200, out=None, bg=None):
        eng.flatten_pages_dev(d_in.ptr, pages_bytes, [off], [h], [w], [r], d_out.ptr if out is None else out, out_bytes,
                              floor, d_bg.ptr if bg is None else bg)

    try:
        for kwargs, message in ((dict(off=1), "outside the 1200-byte buffer"), (dict(off=-1), "outside the 1200-byte"),
                                (dict(pages_bytes=1199), "outside the 1199-byte"), (dict(out_bytes=1199), "outside the 1199"),
                                (dict(h=0), r"\[1, 16384\]"), (dict(w=0), r"\[1, 16384\]"), (dict(h=-3), r"\[1, 16384\]"),
                                (dict(h=16385, w=1), r"\[1, 16384\]"), (dict(h=1, w=16385), r"\[1, 16384\]"),
                                (dict(r=0), r"radius 0 outside \[1, 127\]"), (dict(r=128), "radius 128"),
                                (dict(r=-1), "radius -1"), (dict(floor=256), "floor 256"), (dict(floor=-1), "floor -1"),
                                (dict(out=d_in.ptr + 600, out_bytes=600, h=20), "output buffer overlaps the pages"),
                                (dict(bg=d_in.ptr + 600, out_bytes=600, h=20), "background buffer overlaps the pages"),
                                (dict(bg=d_out.ptr + 300, out_bytes=600, h=20), "background buffer overlaps the output")):
            with pytest.raises(_lib.AsrError, match=r"^asr error \d+: flatten_pages: .*" + message) as info:
                flatten(**kwargs)
            assert info.value.code == _lib.ASR_ERR_INVALID, kwargs
        assert np.all(d_out.download((1200,), np.uint8) == GUARD) and np.all(d_bg.download((1200,), np.uint8) == GUARD)
        assert np.array_equal(d_in.download((40, 30), np.uint8), page)
        flatten()                                                # the same call with nothing wrong writes its 1200 bytes
        assert np.array_equal(d_out.download((40, 30), np.uint8), flatten_page_host(page, 3))
        assert np.array_equal(d_bg.download((40, 30), np.uint8), page_background_host(page, 3))
        # nothing to do is not an error, and writes nothing
        d_out.upload(guard)
        d_bg.upload(guard)
        eng.flatten_pages_dev(d_in.ptr, 1200, [], [], [], [], d_out.ptr, 1200, 64, d_bg.ptr)
        assert np.all(d_out.download((1200,), np.uint8) == GUARD) and np.all(d_bg.download((1200,), np.uint8) == GUARD)
    finally:
        d_in.free()
        d_out.free()
        d_bg.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tutorial():
    page = np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]
    assert page.shape == (1181, 835)
    return page


@pytest.fixture(scope="module")
def dark(tutorial):
    """the tutorial page under a spine shadow on the left and a gradient of 20 % from top to bottom"""
    return shaded(tutorial)


def test_device_pages_flattened_brings_the_systems_of_the_shaded_page_back(recognizer, tutorial, dark):  # noqa: F811
    from audio_sheet_retrieval_amd.sheet_utils.omr import (IN_U8_RAW, DevicePages, flatten_page_host, flatten_pages_dev)
    eng = recognizer.system_detector.engine
    raw = DevicePages(eng, [dark])
    try:
        flat = raw.flattened()
        try:
            assert flat.engine is eng and len(flat) == 1 and flat.radii.tolist() == [13] and flat.radii.dtype == np.int32
            assert flat.heights.tolist() == [1181] and flat.widths.tolist() == [835]
            assert flat.offsets.tolist() == [0] and flat.nbytes == 1181 * 835
            page = flat.download_page(0)
            _same(page, flatten_page_host(dark), "flattened()")
            results = recognizer.detect_systems_pages([page], in_mode=IN_U8_RAW, dev_pages=flat)[0]
        finally:
            flat.free()
        _same(raw.download_page(0), dark, "the source stays valid")
        given = raw.flattened(radius=6, floor=0)
        try:
            assert given.radii.tolist() == [6]
            _same(given.download_page(0), flatten_page_host(dark, 6, 0), "flattened(6, 0)")
        finally:
            given.free()
        shaded_systems = recognizer.detect_systems_pages([dark], in_mode=IN_U8_RAW, dev_pages=raw)[0]
    finally:
        raw.free()
    clean = DevicePages(eng, [tutorial])
    try:
        clean_systems = recognizer.detect_systems_pages([tutorial], in_mode=IN_U8_RAW, dev_pages=clean)[0]
    finally:
        clean.free()
    if isinstance(shaded_systems, Exception):
        print("the shaded page without the stage: %r" % (shaded_systems,))
    else:
        print("the shaded page without the stage: %d systems %s" % (
            len(shaded_systems), [np.asarray(s).astype(int).tolist() for s in shaded_systems]))
    assert not isinstance(results, Exception) and not isinstance(clean_systems, Exception)
    assert len(clean_systems) == 6 and len(results) == 6
    diffs = [np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() for a, b in zip(results, clean_systems)]
    print("systems of the flattened page against the clean page, largest coordinate difference per system: %s" % diffs)
    assert max(diffs) <= 2
    from_host = flatten_pages_dev(eng, [dark])
    try:
        assert from_host.radii.tolist() == [13]
        _same(from_host.download_page(0), page, "flatten_pages_dev")
    finally:
        from_host.free()


def _scan_directory(tmp_path, name, page):
    from PIL import Image
    d = tmp_path / name / "a_piece" / "sheet"
    d.mkdir(parents=True)
    Image.fromarray(page).save(str(d / "01.png"))
    return str(tmp_path / name)


def test_load_umc_scans_reads_a_shaded_tilted_page_at_twice_the_resolution(recognizer, tutorial, dark, tmp_path):  # noqa: F811
    from audio_sheet_retrieval_amd.sheet_utils.omr import IN_U8_RAW, DevicePages, shear_page_host, unwrap_systems
    from audio_sheet_retrieval_amd.sheet_utils.umc import load_umc_scans
    twice = lambda page: np.repeat(np.repeat(shear_page_host(page, 30), 2, axis=0), 2, axis=1)
    big, big_clean = twice(dark), twice(tutorial)
    assert big.shape == (2362, 1670)
    scans, clean_scans = _scan_directory(tmp_path, "scans", big), _scan_directory(tmp_path, "clean", big_clean)
    eng = recognizer.system_detector.engine

    def strip_of(upload, stages):
        """the strip of unwrap_systems on the page that the stages make of the upload"""
        pages = DevicePages(eng, [upload])
        try:
            for stage in stages:
                following = stage(pages)
                pages.free()
                pages = following
            page = pages.download_page(0)
            systems = recognizer.detect_systems_pages([page], in_mode=IN_U8_RAW, dev_pages=pages)[0]
        finally:
            pages.free()
        assert page.shape == (1181, 835) and not isinstance(systems, Exception) and len(systems) == 6
        return unwrap_systems(page, systems, 160)

    def flattened_26(pages):
        flat = pages.flattened()
        assert flat.radii.tolist() == [26]
        return flat

    want = strip_of(big, [flattened_26, lambda p: p.deskewed(), lambda p: p.resized(835)])
    for return_device in (False, True):
        res = load_umc_scans(scans, omr=recognizer, return_device=return_device, device_post=return_device, flatten=True)
        assert res[0] == ["a_piece"] and len(res[2]) == 1
        assert res[2][0].dtype == np.uint8 and np.array_equal(res[2][0], want)
        if return_device:
            res[3].buf.free()
    # without the deskew the stage stands between the upload and the resize; radius and floor are handed on
    only = load_umc_scans(scans, omr=recognizer, flatten=True, deskew=False, flatten_radius=30, flatten_floor=32)
    assert len(only[2]) == 1
    assert np.array_equal(only[2][0], strip_of(big, [lambda p: p.flattened(30, 32), lambda p: p.resized(835)]))
    # flatten=False, the default, is the route as it was: upload, deskew, resize (on white paper, where that route works)
    parent = strip_of(big_clean, [lambda p: p.deskewed(), lambda p: p.resized(835)])
    for kwargs in (dict(flatten=False), dict()):
        plain = load_umc_scans(clean_scans, omr=recognizer, **kwargs)
        assert len(plain[2]) == 1 and np.array_equal(plain[2][0], parent)
