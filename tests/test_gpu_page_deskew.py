"""GPU: the skew of scanned pages (asr_skew_estimate_dev, asr_deskew_pages_dev, csrc/page_deskew_kernels.hip) - the device
against the numpy restatements sheet_utils/omr.skew_scores_host / pick_slope / shear_page_host, integer for integer and
byte for byte (tests/test_page_deskew_host.py holds those against independent derivations), the chunking, the argument
checks, and DevicePages.deskewed / load_umc_scans end to end on the tutorial page sheared by 30 / 1024."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import omr_ref  # noqa: E402

MODEL = "mutopia_ccal_cont"
GUARD = 0xA5
GAP = 5
# (h, w).  The estimate's tiles are 32 rows x 448 columns: the last two shapes have a second column tile of one column
# and three column tiles; 129, 300, 64 + 1 rows end a row tile early.
MIXED = [(1, 1), (1, 7), (7, 1), (2, 2), (37, 53), (64, 129), (129, 200), (300, 17), (33, 449), (40, 1000)]
SLOPES = [0, 1, -1, 128, -128, 37, -77, 2, 128, -128]


@pytest.fixture(scope="module")
def eng():
    from audio_sheet_retrieval_amd import _lib
    engine = _lib.Engine(MODEL, device=0)
    yield engine
    engine.close()


@pytest.fixture(scope="module")
def mixed():
    """the pages and, computed once, their scores at max_slope 128 (the score of a slope does not depend on max_slope:
    those of 64 are the middle of these)"""
    from audio_sheet_retrieval_amd.sheet_utils.omr import skew_scores_host
    rng = np.random.default_rng(23)
    pages = [rng.integers(0, 256, s, dtype=np.uint8) for s in MIXED]
    pages[6][:] = 255 - (rng.random(MIXED[6]) < 0.02) * rng.integers(0, 256, MIXED[6])        # mostly paper
    return pages, [skew_scores_host(p, 128) for p in pages]


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

    def estimate(self, K):
        return self.eng.skew_estimate_dev(self.buf.ptr, self.nbytes, self.offs, self.heights, self.widths, K,
                                          return_scores=True)

    def shear(self, slopes, fill):
        """-> (outputs per page, every other byte of the output buffer)"""
        out = self.eng.alloc(self.nbytes).upload(np.full(self.nbytes, GUARD, np.uint8))
        try:
            self.eng.deskew_pages_dev(self.buf.ptr, self.nbytes, self.offs, self.heights, self.widths, slopes, out.ptr,
                                      self.nbytes, fill)
            flat = out.download((self.nbytes,), np.uint8)
        finally:
            out.free()
        rest = np.ones(self.nbytes, bool)
        outs = []
        for o, p in zip(self.offs, self.pages):
            outs.append(flat[o:o + p.size].reshape(p.shape))
            rest[o:o + p.size] = False
        return outs, flat[rest]

    def free(self):
        self.buf.free()


def test_scores_and_slopes_of_a_mixed_batch_equal_the_host(eng, mixed):
    from audio_sheet_retrieval_amd.sheet_utils.omr import pick_slope
    pages, want = mixed
    lay = Layout(eng, pages)
    try:
        assert {int(o) % 4 for o in lay.offs} == {0, 1, 2, 3}
        for K in (64, 128):
            slopes, scores = lay.estimate(K)
            assert slopes.dtype == np.int32 and scores.dtype == np.int64 and scores.shape == (len(pages), 2 * K + 1)
            for i, page in enumerate(pages):
                host = want[i][128 - K:128 + K + 1]
                assert np.array_equal(scores[i], host), (K, page.shape, np.flatnonzero(scores[i] != host)[:4].tolist())
                assert slopes[i] == pick_slope(host), (K, page.shape)
        slopes, scores = lay.estimate(0)
        assert np.all(slopes == 0) and scores[:, 0].tolist() == [int(w[128]) for w in want]
        assert np.array_equal(eng.skew_estimate_dev(lay.buf.ptr, lay.nbytes, lay.offs, lay.heights, lay.widths, 64),
                              lay.estimate(64)[0])                               # scores = NULL
    finally:
        lay.free()


@pytest.mark.parametrize("fill", [0, 255])
def test_sheared_bytes_of_a_mixed_batch_equal_the_host(eng, mixed, fill):
    from audio_sheet_retrieval_amd.sheet_utils.omr import shear_page_host
    pages, _ = mixed
    lay = Layout(eng, pages)
    try:
        for slopes in (SLOPES, SLOPES[::-1]):
            outs, rest = lay.shear(slopes, fill)
            for page, got, k in zip(pages, outs, slopes):
                want = shear_page_host(page, k, fill)
                assert np.array_equal(got, want), (page.shape, k, fill, np.argwhere(got != want)[:4].tolist())
            assert rest.size == GAP * (len(pages) + 1) and np.all(rest == GUARD)
    finally:
        lay.free()


def test_a_300_dpi_page_equals_the_host(eng):
    from audio_sheet_retrieval_amd.sheet_utils.omr import pick_slope, shear_page_host, skew_scores_host
    page = np.random.default_rng(300).integers(0, 256, (3508, 2480), dtype=np.uint8)
    lay = Layout(eng, [page])
    try:
        slopes, scores = lay.estimate(64)
        want = skew_scores_host(page, 64)
        assert np.array_equal(scores[0], want) and slopes[0] == pick_slope(want)
        outs, rest = lay.shear([-23], 255)
        assert np.array_equal(outs[0], shear_page_host(page, -23)) and np.all(rest == GUARD)
    finally:
        lay.free()


def test_a_batch_in_chunks_gives_the_same(eng, mixed, monkeypatch):
    """at max_slope 128 the profiles of 300 x 17 take 257 x 302 x 4 bytes = 0.3 MB, those of 40 x 1000 257 x 290 x 4: a
    budget of 1 MB holds three such pages"""
    pages, want = mixed
    order = [7, 9, 7, 7, 6, 9, 7, 0, 7, 9, 8, 7]
    lay = Layout(eng, [pages[i] for i in order])
    try:
        whole = lay.estimate(128)
        monkeypatch.setenv("ASR_OMR_BUDGET_MB", "1")
        chunked = lay.estimate(128)
        monkeypatch.delenv("ASR_OMR_BUDGET_MB")
        assert np.array_equal(whole[0], chunked[0]) and np.array_equal(whole[1], chunked[1])
        assert np.array_equal(chunked[1], np.stack([want[i] for i in order]))
    finally:
        lay.free()


def test_invalid_arguments_launch_nothing(eng):
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils.omr import shear_page_host
    page = np.random.default_rng(3).integers(0, 256, (40, 30), dtype=np.uint8)
    d_in = eng.alloc(1200).upload(page)
    d_out = eng.alloc(1200).upload(np.full(1200, GUARD, np.uint8))

    def shear(pages_bytes=1200, off=0, h=40, w=30, k=5, fill=255, out_bytes=1200, out=None):
        eng.deskew_pages_dev(d_in.ptr, pages_bytes, [off], [h], [w], [k], d_out.ptr if out is None else out, out_bytes, fill)

    def estimate(pages_bytes=1200, off=0, h=40, w=30, K=64):
        return eng.skew_estimate_dev(d_in.ptr, pages_bytes, [off], [h], [w], K)

    try:
        for kwargs, message in ((dict(off=1), "outside the 1200-byte buffer"), (dict(off=-1), "outside the 1200-byte"),
                                (dict(pages_bytes=1199), "outside the 1199-byte"), (dict(out_bytes=1199), "outside the 1199"),
                                (dict(h=0), r"\[1, 16384\]"), (dict(w=0), r"\[1, 16384\]"), (dict(h=-3), r"\[1, 16384\]"),
                                (dict(h=16385, w=1), r"\[1, 16384\]"), (dict(h=1, w=16385), r"\[1, 16384\]"),
                                (dict(k=129), "slope 129"), (dict(k=-129), "slope -129"), (dict(fill=256), "fill 256"),
                                (dict(fill=-1), "fill -1"), (dict(out=d_in.ptr + 600, out_bytes=600, h=20), "overlaps")):
            with pytest.raises(_lib.AsrError, match=message) as info:
                shear(**kwargs)
            assert info.value.code == _lib.ASR_ERR_INVALID, kwargs
        for kwargs, message in ((dict(off=1), "outside the 1200-byte buffer"), (dict(pages_bytes=1199), "outside the 1199"),
                                (dict(h=0), r"\[1, 16384\]"), (dict(w=16385, h=1), r"\[1, 16384\]"),
                                (dict(K=129), "max_slope 129"), (dict(K=-1), "max_slope -1")):
            with pytest.raises(_lib.AsrError, match=message) as info:
                estimate(**kwargs)
            assert info.value.code == _lib.ASR_ERR_INVALID, kwargs
        assert np.all(d_out.download((1200,), np.uint8) == GUARD)
        assert np.array_equal(d_in.download((40, 30), np.uint8), page)
        shear()                                                  # the same call with nothing wrong writes its 1200 bytes
        assert np.array_equal(d_out.download((40, 30), np.uint8), shear_page_host(page, 5))
        assert estimate().shape == (1,)
        # nothing to do is not an error, and writes nothing
        d_out.upload(np.full(1200, GUARD, np.uint8))
        eng.deskew_pages_dev(d_in.ptr, 1200, [], [], [], [], d_out.ptr, 1200)
        assert eng.skew_estimate_dev(d_in.ptr, 1200, [], [], []).shape == (0,)
        assert np.all(d_out.download((1200,), np.uint8) == GUARD)
    finally:
        d_in.free()
        d_out.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheared():
    """the tutorial page sheared by 30 / 1024 on the host: a staff drifts 24 pixels across the page"""
    from audio_sheet_retrieval_amd.sheet_utils.omr import shear_page_host
    page = np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]
    assert page.shape == (1181, 835)
    return shear_page_host(page, 30)


@pytest.fixture(scope="module")
def recognizer():
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    real = lambda name: omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_%s_params.npz" % name))
    return build_recognizer(real("system"), real("bar"))


def _edge_spreads(systems):
    """max - min of the left and of the right edges over systems 2 .. 6 (the first system is indented)"""
    left, right = [s[0, 1] for s in systems[1:]], [s[1, 1] for s in systems[1:]]
    return max(left) - min(left), max(right) - min(right)


def test_device_pages_deskewed_straightens_the_tutorial_page(recognizer, sheared):
    from audio_sheet_retrieval_amd.sheet_utils.omr import IN_U8_RAW, DevicePages, deskew_pages_dev, shear_page_host
    eng = recognizer.system_detector.engine
    raw = DevicePages(eng, [sheared])
    try:
        straight = raw.deskewed()
        try:
            assert straight.engine is eng and len(straight) == 1 and straight.slopes.tolist() == [-30]
            assert straight.heights.tolist() == [1181] and straight.widths.tolist() == [835]
            assert straight.offsets.tolist() == [0] and straight.nbytes == 1181 * 835
            page = straight.download_page(0)
            assert np.array_equal(page, shear_page_host(sheared, -30))
            results = recognizer.detect_systems_pages([page], in_mode=IN_U8_RAW, dev_pages=straight)
        finally:
            straight.free()
        assert np.array_equal(raw.download_page(0), sheared)                        # the source stays valid
        given = raw.deskewed(slopes=[7], fill=0)                                    # no estimate
        try:
            assert given.slopes.tolist() == [7]
            assert np.array_equal(given.download_page(0), shear_page_host(sheared, 7, 0))
        finally:
            given.free()
        tilted = recognizer.detect_systems_pages([sheared], in_mode=IN_U8_RAW, dev_pages=raw)
    finally:
        raw.free()
    assert len(results[0]) == 6 and len(tilted[0]) == 6
    (left, right), (left_tilted, right_tilted) = _edge_spreads(results[0]), _edge_spreads(tilted[0])
    print("edge spreads of systems 2..6: deskewed %s / %s, sheared %s / %s" % (left, right, left_tilted, right_tilted))
    assert 2 * left <= left_tilted and 2 * right <= right_tilted
    from_host = deskew_pages_dev(eng, [sheared])
    try:
        assert from_host.slopes.tolist() == [-30] and np.array_equal(from_host.download_page(0), page)
    finally:
        from_host.free()


def test_load_umc_scans_reads_a_tilted_page_at_twice_the_resolution(recognizer, sheared, tmp_path):
    from PIL import Image
    from audio_sheet_retrieval_amd.sheet_utils.omr import IN_U8_RAW, DevicePages, unwrap_systems
    from audio_sheet_retrieval_amd.sheet_utils.umc import load_umc_scans
    big = np.repeat(np.repeat(sheared, 2, axis=0), 2, axis=1)
    assert big.shape == (2362, 1670)
    d = tmp_path / "scans" / "a_piece" / "sheet"
    d.mkdir(parents=True)
    Image.fromarray(big).save(str(d / "01.png"))
    eng = recognizer.system_detector.engine
    raw = DevicePages(eng, [big])
    try:
        straight = raw.deskewed()
        try:
            assert straight.slopes.tolist() == [-30]
            small = straight.resized(835)
        finally:
            straight.free()
        try:
            page = small.download_page(0)
            systems = recognizer.detect_systems_pages([page], in_mode=IN_U8_RAW, dev_pages=small)[0]
        finally:
            small.free()
    finally:
        raw.free()
    assert page.shape == (1181, 835) and len(systems) == 6
    want = unwrap_systems(page, systems, 160)
    for return_device in (False, True):
        res = load_umc_scans(str(tmp_path / "scans"), omr=recognizer, return_device=return_device, device_post=return_device)
        assert res[0] == ["a_piece"] and len(res[2]) == 1
        assert res[2][0].dtype == np.uint8 and np.array_equal(res[2][0], want)
        if return_device:
            res[3].buf.free()
    # without the deskew the route is load_umc_sheets(page_width=835): the strip of the tilted page
    tilted = load_umc_scans(str(tmp_path / "scans"), omr=recognizer, deskew=False)
    assert len(tilted[2]) == 1 and not np.array_equal(tilted[2][0], want)
