"""GPU: the scanner borders of scanned pages (asr_crop_estimate_dev / asr_crop_pages_dev, csrc/page_crop_kernels.hip) - the
counts, the rects, the statuses and the cropped bytes against the host restatements sheet_utils/omr.crop_counts_host /
crop_rect_host / crop_page_host (tests/test_page_crop_host.py holds those against the definition), the bytes between the
output pages through a guard pattern, the argument checks, and DevicePages.cropped / load_umc_scans end to end on the
framed tutorial page."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
from test_gpu_page_deskew import recognizer  # noqa: E402,F401  (the real weights from tests/golden)
from test_page_crop_host import framed  # noqa: E402

MODEL = "mutopia_ccal_cont"
GUARD = 0xA5
GAP = 5
# (floor, share); at (128, 512) and (127, 500) a row of noise is a border row or not by chance: short runs at every edge
SETTINGS = [(64, 512), (128, 512), (127, 500), (128, 300), (200, 1000), (0, 512), (255, 1), (1, 1024)]


@pytest.fixture(scope="module")
def eng():
    from audio_sheet_retrieval_amd import _lib
    engine = _lib.Engine(MODEL, device=0)
    yield engine
    engine.close()


def _pages():
    """-> (pages, margins).  Shapes that are no multiple of 4, of 64 or of the tiles (64 rows x 1024 columns, 256 per wave; 8 rows of a
    copy), more than one tile along each axis, the longest row and the longest column; frames on one, two and four
    sides, one exactly a quarter of the page wide, a count exactly at the limit and one below, all dark, all white,
    noise"""
    rng = np.random.default_rng(31)
    paper = lambda h, w: (255 - (rng.random((h, w)) < 0.04) * rng.integers(128, 256, (h, w))).astype(np.uint8)
    noise = lambda h, w: rng.integers(0, 256, (h, w), dtype=np.uint8)
    at_limit = np.full((40, 40), 255, np.uint8)
    at_limit[0, 10:20] = 0                                          # 10 of 20: a border row at share 512
    below_limit = at_limit.copy()
    below_limit[0, 19] = 255
    quarter = framed(paper(48, 60), (16, 0, 20, 0))                 # 64 x 80: the top and the left quarter
    assert quarter.shape == (64, 80)
    pages = [np.zeros((1, 1), np.uint8), noise(3, 5), framed(paper(60, 120), (2, 5, 6, 3)), framed(paper(255, 250), (0, 0, 7, 0)),
             framed(paper(290, 1000), (10, 0, 0, 25)), framed(paper(4, 16000), (0, 0, 384, 0)), framed(paper(16380, 3), (4, 0, 0, 0)),
             quarter, at_limit, below_limit, np.zeros((50, 70), np.uint8), np.full((33, 65), 255, np.uint8),
             noise(67, 129), noise(130, 515), framed(noise(70, 300) | 0x80, (3, 3, 3, 3), value=9)]
    assert [p.shape for p in pages[2:7]] == [(67, 129), (255, 257), (300, 1025), (4, 16384), (16384, 3)]
    margins = [0, 1, 2, 0, 13, 1, 0, 0, 0, 0, 3, 3, 1, 0, 40]
    assert len(margins) == len(pages)
    return pages, margins


@pytest.fixture(scope="module")
def batch():
    """the pages, their margins and, computed once per (floor, share), what the host gives: (rect, status) per page, the
    counts per page and the cropped pages"""
    from audio_sheet_retrieval_amd.sheet_utils.omr import crop_counts_host, crop_rect_host
    pages, margins = _pages()
    want = {}
    for floor, share in SETTINGS:
        rects = [crop_rect_host(p, floor, share, m) for p, m in zip(pages, margins)]
        want[floor, share] = (rects, [crop_counts_host(p, floor) for p in pages],
                              [np.ascontiguousarray(p[r0:r1, c0:c1]) for p, ((r0, r1, c0, c1), _) in zip(pages, rects)])
    rects = want[64, 512][0]
    assert [rects[i] for i in (0, 2, 7, 8, 9, 10, 11)] == [
        ((0, 1, 0, 1), 1), ((4, 60, 8, 124), 0), ((16, 64, 20, 80), 0), ((1, 40, 0, 40), 0), ((0, 40, 0, 40), 0),
        ((0, 50, 0, 70), 1), ((0, 33, 0, 65), 0)]
    assert rects[14] == ((0, 76, 0, 306), 1)                        # a margin larger than the paper
    return pages, margins, want


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

    def estimate(self, margins, floor, share):
        """-> (rects (n, 4), status (n,), row counts per page, column counts per page)"""
        rects, status, rows, cols = self.eng.crop_estimate_dev(self.buf.ptr, self.nbytes, self.offs, self.heights,
                                                               self.widths, margins, floor, share, return_counts=True)
        assert rects.dtype == np.int32 and status.dtype == np.int32 and rows.dtype == np.int32 and cols.dtype == np.int32
        assert rows.size == sum(self.heights) and cols.size == sum(self.widths)
        alone = self.eng.crop_estimate_dev(self.buf.ptr, self.nbytes, self.offs, self.heights, self.widths, margins, floor,
                                           share)                   # without the counts: the same rects
        assert np.array_equal(alone[0], rects) and np.array_equal(alone[1], status)
        return rects, status, np.split(rows, np.cumsum(self.heights)[:-1]), np.split(cols, np.cumsum(self.widths)[:-1])

    def crop(self, rects):
        """-> the cropped pages; asserts that every other byte of the output buffer kept the guard"""
        rects = np.asarray(rects, np.int32).reshape(-1, 4)
        shapes = [(int(r1 - r0), int(c1 - c0)) for r0, r1, c0, c1 in rects]
        sizes = np.asarray([h * w for h, w in shapes], np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes + GAP)[:-1]]).astype(np.int64) + GAP
        nbytes = int(offs[-1] + sizes[-1]) + GAP
        out = self.eng.alloc(nbytes).upload(np.full(nbytes, GUARD, np.uint8))
        try:
            self.eng.crop_pages_dev(self.buf.ptr, self.nbytes, self.offs, self.heights, self.widths, rects, offs, out.ptr,
                                    nbytes)
            flat = out.download((nbytes,), np.uint8)
        finally:
            out.free()
        rest = np.ones(nbytes, bool)
        outs = []
        for o, s, shape in zip(offs, sizes, shapes):
            outs.append(flat[o:o + s].reshape(shape))
            rest[o:o + s] = False
        assert rest.sum() == GAP * (len(shapes) + 1) and np.all(flat[rest] == GUARD)          # no byte outside a page
        return outs, {int(o) % 4 for o in offs}

    def free(self):
        self.buf.free()


def _same(got, want, what):
    assert np.array_equal(got, want), (what, got.shape, np.argwhere(np.asarray(got) != np.asarray(want))[:4].tolist())


@pytest.fixture(scope="module")
def layout(eng, batch):
    lay = Layout(eng, batch[0])
    assert {int(o) % 4 for o in lay.offs} == {0, 1, 2, 3}
    yield lay
    lay.free()


@pytest.mark.parametrize("floor,share", SETTINGS)
def test_a_mixed_batch_equals_the_host(layout, batch, floor, share):
    pages, margins, want = batch
    want_rects, want_counts, want_pages = want[floor, share]
    rects, status, rows, cols = layout.estimate(margins, floor, share)
    for i in range(len(pages)):
        _same(rows[i], want_counts[i][0], ("row counts", i, pages[i].shape))
        _same(cols[i], want_counts[i][1], ("column counts", i, pages[i].shape))
        assert (tuple(rects[i].tolist()), int(status[i])) == want_rects[i], (i, pages[i].shape)
    if floor == 0:
        assert not status.any() and all(tuple(r) == (0, p.shape[0], 0, p.shape[1]) for r, p in zip(rects.tolist(), pages))
    outs, alignments = layout.crop(rects)
    assert alignments == {0, 1, 2, 3}
    for i in range(len(pages)):
        _same(outs[i], want_pages[i], ("cropped", i, pages[i].shape))


def test_no_pages_is_not_an_error(eng):
    guard = np.full(64, GUARD, np.uint8)
    d_in, d_out = eng.alloc(64).upload(guard), eng.alloc(64).upload(guard)
    try:
        rects, status, rows, cols = eng.crop_estimate_dev(d_in.ptr, 64, [], [], [], [], return_counts=True)
        assert rects.shape == (0, 4) and status.shape == (0,) and rows.size == 0 and cols.size == 0
        eng.crop_pages_dev(d_in.ptr, 64, [], [], [], np.zeros((0, 4), np.int32), [], d_out.ptr, 64)
        assert np.all(d_out.download((64,), np.uint8) == GUARD)
    finally:
        d_in.free()
        d_out.free()


def test_given_rects_are_applied_as_they_are(layout, batch):
    pages = batch[0]
    rng = np.random.default_rng(5)
    rects = []
    for p in pages:
        h, w = p.shape
        r0, c0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        rects.append((r0, int(rng.integers(r0 + 1, h + 1)), c0, int(rng.integers(c0 + 1, w + 1))))
    rects[4] = (3, 300, 1, 1024)                                     # rows of 1023 bytes: every alignment on both sides
    rects[5] = (1, 4, 5, 16384)
    rects[6] = (0, 16384, 1, 2)                                      # a single column
    outs, _ = layout.crop(rects)
    for i, (p, (r0, r1, c0, c1)) in enumerate(zip(pages, rects)):
        _same(outs[i], p[r0:r1, c0:c1], ("rect", i, rects[i]))


def test_a_page_does_not_depend_on_the_others(eng, batch):
    pages, margins, want = batch
    want_rects, want_counts, want_pages = want[64, 512]
    for order in (list(range(len(pages)))[::-1], [12, 2, 7], [4]):
        lay = Layout(eng, [pages[i] for i in order])
        try:
            rects, status, rows, cols = lay.estimate([margins[i] for i in order], 64, 512)
            outs, _ = lay.crop(rects)
        finally:
            lay.free()
        for j, i in enumerate(order):
            assert (tuple(rects[j].tolist()), int(status[j])) == want_rects[i], (order, i)
            _same(rows[j], want_counts[i][0], ("row counts", order, i))
            _same(cols[j], want_counts[i][1], ("column counts", order, i))
            _same(outs[j], want_pages[i], ("cropped", order, i))


def test_invalid_arguments_launch_nothing(eng):
    from audio_sheet_retrieval_amd import _lib
    page = framed(np.full((34, 24), 255, np.uint8), (3, 3, 3, 3))
    assert page.shape == (40, 30)
    guard = np.full(1200, GUARD, np.uint8)
    d_in = eng.alloc(1200).upload(page)
    d_out = eng.alloc(1200).upload(guard)

    def estimate(pages_bytes=1200, off=0, h=40, w=30, floor=64, share=512, margin=0):
        return eng.crop_estimate_dev(d_in.ptr, pages_bytes, [off], [h], [w], [margin], floor, share)

    def crop(pages_bytes=1200, off=0, h=40, w=30, rect=(3, 37, 3, 27), out_off=0, out_bytes=1200, out=None):
        eng.crop_pages_dev(d_in.ptr, pages_bytes, [off], [h], [w], [rect], [out_off], d_out.ptr if out is None else out,
                           out_bytes)

    page_checks = ((dict(off=1), "outside the 1200-byte buffer"), (dict(off=-1), "outside the 1200-byte"),
                   (dict(pages_bytes=1199), "outside the 1199-byte"), (dict(h=0), r"\[1, 16384\]"),
                   (dict(w=0), r"\[1, 16384\]"), (dict(h=-3), r"\[1, 16384\]"), (dict(h=16385, w=1), r"\[1, 16384\]"),
                   (dict(h=1, w=16385), r"\[1, 16384\]"))
    try:
        for call, checks in ((estimate, page_checks + (
                (dict(floor=256), "floor 256"), (dict(floor=-1), "floor -1"), (dict(share=0), r"share 0 outside \[1, 1024\]"),
                (dict(share=1025), "share 1025"), (dict(margin=-1), "margin -1 is negative"))), (crop, page_checks + (
                (dict(rect=(-1, 37, 3, 27)), "rect rows"), (dict(rect=(37, 37, 3, 27)), "rect rows"),
                (dict(rect=(3, 41, 3, 27)), "rect rows"), (dict(rect=(3, 37, -1, 27)), "rect rows"),
                (dict(rect=(3, 37, 27, 27)), "rect rows"), (dict(rect=(3, 37, 3, 31)), "rect rows"),
                (dict(rect=(38, 37, 3, 27)), "rect rows"), (dict(out_bytes=34 * 24 - 1), "outside the 815-byte buffer"),
                (dict(out_off=1200 - 34 * 24 + 1), "outside the 1200-byte buffer"), (dict(out_off=-1), "outside the 1200-byte"),
                (dict(out=d_in.ptr + 600, out_bytes=600, h=20, rect=(0, 20, 0, 30)), "output buffer overlaps the pages")))):
            for kwargs, message in checks:
                with pytest.raises(_lib.AsrError, match=r"^asr error \d+: crop_pages: .*" + message) as info:
                    call(**kwargs)
                assert info.value.code == _lib.ASR_ERR_INVALID, kwargs
        assert np.all(d_out.download((1200,), np.uint8) == GUARD)
        assert np.array_equal(d_in.download((40, 30), np.uint8), page)
        rects, status = estimate()                                  # the same calls with nothing wrong
        assert rects.tolist() == [[3, 37, 3, 27]] and status.tolist() == [0]
        crop()
        flat = d_out.download((1200,), np.uint8)
        assert np.all(flat[:34 * 24] == 255) and np.all(flat[34 * 24:] == GUARD)
    finally:
        d_in.free()
        d_out.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tutorial():
    page = np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]
    assert page.shape == (1181, 835)
    return page


def test_device_pages_cropped_gives_the_tutorial_page_back(eng, tutorial):
    from audio_sheet_retrieval_amd.sheet_utils.omr import DevicePages, crop_page_host, crop_pages_dev
    scan = framed(tutorial)
    other = framed(tutorial[:190, :300], (0, 9, 0, 0))       # (row 199 is a staff line: it would join the frame)
    raw = DevicePages(eng, [scan, other, tutorial])
    try:
        cut = raw.cropped(margin=0)
        try:
            assert cut.engine is eng and len(cut) == 3 and cut.rects.dtype == np.int32 and cut.crop_status.dtype == np.int32
            assert cut.rects.tolist() == [[37, 1218, 41, 876], [0, 190, 0, 300], [0, 1181, 0, 835]]
            assert cut.crop_status.tolist() == [0, 0, 0]
            assert cut.heights.tolist() == [1181, 190, 1181] and cut.widths.tolist() == [835, 300, 835]
            assert cut.offsets.tolist() == [0, 1181 * 835, 1181 * 835 + 57000] and cut.nbytes == 2 * 1181 * 835 + 57000
            _same(cut.download_page(0), tutorial, "cropped(margin=0)")
            pages = cut.download()
            _same(pages[1], tutorial[:190, :300], "a frame on one side")
            _same(pages[2], tutorial, "no frame")
        finally:
            cut.free()
        _same(raw.download_page(0), scan, "the source stays valid")
        default = raw.cropped()                                      # crop_margin per page: 14, 5, 13 - where a border is
        try:
            assert default.rects.tolist() == [[51, 1204, 55, 862], [0, 185, 0, 300], [0, 1181, 0, 835]]
            _same(default.download_page(0), crop_page_host(scan), "cropped()")
        finally:
            default.free()
        each = raw.cropped(floor=1, share=1024, margin=[2, 0, 7])
        try:
            assert each.rects.tolist() == [[39, 1216, 43, 874], [0, 190, 0, 300], [0, 1181, 0, 835]]
        finally:
            each.free()
        given = raw.cropped(rects=[[1, 3, 5, 8], [0, 199, 0, 300], [1180, 1181, 0, 835]])
        try:
            assert given.crop_status.tolist() == [0, 0, 0] and given.heights.tolist() == [2, 199, 1]
            _same(given.download_page(0), scan[1:3, 5:8], "rects=")
            _same(given.download_page(1), other, "rects=")
            _same(given.download_page(2), tutorial[1180:], "rects=")
        finally:
            given.free()
        with pytest.raises(ValueError):
            raw.cropped(margin=[1, 2])
        with pytest.raises(ValueError):
            raw.cropped(rects=[[0, 1, 0, 1]])
    finally:
        raw.free()
    from_host = crop_pages_dev(eng, [scan], margin=0)
    try:
        assert from_host.rects.tolist() == [[37, 1218, 41, 876]]
        _same(from_host.download_page(0), tutorial, "crop_pages_dev")
    finally:
        from_host.free()


def _scan_directory(tmp_path, name, page):
    from PIL import Image
    d = tmp_path / name / "a_piece" / "sheet"
    d.mkdir(parents=True)
    Image.fromarray(page).save(str(d / "01.png"))
    return str(tmp_path / name)


def test_load_umc_scans_reads_a_framed_page(recognizer, tutorial, tmp_path):  # noqa: F811
    from audio_sheet_retrieval_amd.sheet_utils.umc import load_umc_scans
    scans = _scan_directory(tmp_path, "scans", framed(tutorial))
    clean_scans = _scan_directory(tmp_path, "clean", tutorial)
    clean = load_umc_scans(clean_scans, omr=recognizer, deskew=False, page_width=None, return_device=True)
    clean[3].buf.free()
    assert clean[0] == ["a_piece"] and len(clean[2]) == 1 and clean[2][0].shape[0] == 160
    assert not hasattr(clean[3], "crop_rects")
    res = load_umc_scans(scans, omr=recognizer, crop=True, crop_margin=0, deskew=False, page_width=None, return_device=True)
    try:
        assert res[0] == ["a_piece"] and len(res) == 4 and len(res[3]) == 3
        assert res[3].crop_rects.tolist() == [[37, 1218, 41, 876]] and res[3].crop_status.tolist() == [0]
        assert len(res[2]) == 1 and res[2][0].dtype == np.uint8
        _same(res[2][0], clean[2][0], "the strips of the framed page")
    finally:
        res[3].buf.free()
    host = load_umc_scans(scans, omr=recognizer, crop=True, crop_margin=0, deskew=False, page_width=None)
    assert len(host) == 3
    _same(host[2][0], clean[2][0], "the strips of the framed page on the host route")


def test_load_umc_scans_crops_first_and_only_when_asked(recognizer, tutorial, tmp_path):  # noqa: F811
    from audio_sheet_retrieval_amd.sheet_utils.umc import load_umc_scans
    scans = _scan_directory(tmp_path, "scans", framed(tutorial))
    clean_scans = _scan_directory(tmp_path, "clean", tutorial)
    # the whole route at the defaults of the other stages: the crop comes first, so the paper is scaled to the width
    full = load_umc_scans(scans, omr=recognizer, crop=True, crop_floor=32, crop_share=600, crop_margin=0)
    want = load_umc_scans(clean_scans, omr=recognizer)
    _same(full[2][0], want[2][0], "crop, deskew, resize")
    # crop=False, the default, is the route as it was
    plain = load_umc_scans(scans, omr=recognizer, deskew=False, page_width=None)
    off = load_umc_scans(scans, omr=recognizer, deskew=False, page_width=None, crop=False)
    assert len(plain[2]) == len(off[2]) and all(np.array_equal(a, b) for a, b in zip(plain[2], off[2]))
    assert plain[0] == off[0]
