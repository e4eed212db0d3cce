"""GPU: score pages at any resolution (asr_resize_pages_dev, csrc/page_resize_kernels.hip) - the device against the numpy
restatement sheet_utils/omr.resize_page_host byte for byte (tests/test_page_resize_host.py holds that one against an
independent derivation), the argument checks, and load_umc_sheets(page_width=835) end to end."""
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

# (h_in, w_in, h_out, w_out).  The kernel's tiles are 16 rows x 64 columns of the output.
MIXED = [
    # the shapes of the host test
    (7, 5, 3, 4), (13, 17, 5, 6), (5, 4, 11, 9), (9, 9, 9, 9), (64, 97, 21, 33), (1, 40, 1, 7), (40, 1, 7, 1),
    (3, 836, 2, 835),
    # output widths and heights on either side of the tile borders; odd input sizes, so that rows - and, back to back,
    # pages - start at every alignment
    (31, 131, 15, 63), (33, 129, 16, 64), (35, 135, 17, 65), (67, 259, 33, 129), (41, 150, 31, 127),
    # both ends of the supported range: 16 : 1 in both axes (a tile row of 1024 bytes + alignment: two 16-byte pieces
    # per lane, seven rows per chunk) and 1 : 4
    (272, 2080, 17, 130), (9, 17, 36, 68), (16, 1, 1, 4),
    # mixed: down along one axis, up along the other
    (50, 21, 13, 70),
]


@pytest.fixture(scope="module")
def eng():
    from audio_sheet_retrieval_amd import _lib
    engine = _lib.Engine(MODEL, device=0)
    yield engine
    engine.close()


def _run(eng, pages, shapes, gap=5):
    """one resize_pages_dev call: the pages back to back, each output `gap` guard bytes after the one before ->
    (outputs per page, every other byte of the output buffer)"""
    sizes = np.asarray([p.size for p in pages], np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    out_sizes = np.asarray([h * w for h, w in shapes], np.int64)
    out_offs = np.concatenate([[0], np.cumsum(out_sizes + gap)[:-1]]).astype(np.int64) + gap
    out_bytes = int(out_offs[-1] + out_sizes[-1]) + gap
    d_in = eng.alloc(int(sizes.sum())).upload(np.concatenate([p.ravel() for p in pages]))
    d_out = eng.alloc(out_bytes).upload(np.full(out_bytes, GUARD, np.uint8))
    try:
        eng.resize_pages_dev(d_in.ptr, int(sizes.sum()), offs, [p.shape[0] for p in pages], [p.shape[1] for p in pages],
                             out_offs, [h for h, _ in shapes], [w for _, w in shapes], d_out.ptr, out_bytes)
        flat = d_out.download((out_bytes,), np.uint8)
    finally:
        d_in.free()
        d_out.free()
    rest = np.ones(out_bytes, bool)
    outs = []
    for o, n, (h, w) in zip(out_offs, out_sizes, shapes):
        outs.append(flat[o:o + n].reshape(h, w))
        rest[o:o + n] = False
    return outs, flat[rest]


def test_a_mixed_batch_equals_the_host_byte_for_byte(eng):
    from audio_sheet_retrieval_amd.sheet_utils.omr import resize_page_host
    rng = np.random.default_rng(17)
    pages = [rng.integers(0, 256, (h, w), dtype=np.uint8) for h, w, _, _ in MIXED]
    offsets = np.cumsum([0] + [p.size for p in pages[:-1]])
    assert {int(o) % 4 for o in offsets} == {0, 1, 2, 3}
    outs, rest = _run(eng, pages, [(ho, wo) for _, _, ho, wo in MIXED])
    for page, got, (h, w, ho, wo) in zip(pages, outs, MIXED):
        want = resize_page_host(page, ho, wo)
        assert np.array_equal(got, want), ((h, w, ho, wo), np.argwhere(got != want)[:4].tolist())
    assert rest.size == 5 * (len(MIXED) + 1) and np.all(rest == GUARD)      # before, between and after the outputs


def test_invalid_arguments_launch_nothing(eng):
    from audio_sheet_retrieval_amd import _lib
    page = np.random.default_rng(3).integers(0, 256, (40, 30), dtype=np.uint8)
    d_in = eng.alloc(page.size).upload(page)
    d_out = eng.alloc(300).upload(np.full(300, GUARD, np.uint8))

    def call(pages_bytes=1200, off=0, h=40, w=30, out_off=0, ho=20, wo=15, out_bytes=300):
        eng.resize_pages_dev(d_in.ptr, pages_bytes, [off], [h], [w], [out_off], [ho], [wo], d_out.ptr, out_bytes)

    try:
        for kwargs, message in ((dict(off=1), "outside the 1200-byte buffer"), (dict(off=1201), "outside the 1200-byte"),
                                (dict(off=-1), "outside the 1200-byte"), (dict(pages_bytes=1199), "outside the 1199-byte"),
                                (dict(out_off=1), "outside the 300-byte buffer"), (dict(out_bytes=299), "outside the 299"),
                                (dict(h=0), "at least 1"), (dict(w=0), "at least 1"), (dict(ho=0), "at least 1"),
                                (dict(wo=0), "at least 1"), (dict(h=-3), "at least 1"),
                                (dict(ho=2, out_bytes=30), "ratio"),          # 40 rows -> 2: 20 : 1
                                (dict(wo=1, out_bytes=20), "ratio"),          # 30 columns -> 1: 30 : 1
                                (dict(h=2, w=3, pages_bytes=6, ho=9, wo=12), "ratio"),       # 2 rows -> 9: 1 : 4.5
                                (dict(h=2, w=3, pages_bytes=6, ho=8, wo=13), "ratio")):
            with pytest.raises(_lib.AsrError, match=message) as info:
                call(**kwargs)
            assert info.value.code == _lib.ASR_ERR_INVALID, kwargs
        assert np.all(d_out.download((300,), np.uint8) == GUARD)
        call()                                                   # the same call with nothing wrong writes its 300 bytes
        from audio_sheet_retrieval_amd.sheet_utils.omr import resize_page_host
        assert np.array_equal(d_out.download((20, 15), np.uint8), resize_page_host(page, 20, 15))
        # nothing to do is not an error, and writes nothing
        d_out.upload(np.full(300, GUARD, np.uint8))
        eng.resize_pages_dev(d_in.ptr, 1200, [], [], [], [], [], [], d_out.ptr, 300)
        assert np.all(d_out.download((300,), np.uint8) == GUARD)
    finally:
        d_in.free()
        d_out.free()


def test_a_300_dpi_page_equals_the_host(eng):
    from audio_sheet_retrieval_amd.sheet_utils.omr import resize_page_host, resized_shape
    page = np.random.default_rng(300).integers(0, 256, (3508, 2480), dtype=np.uint8)
    shape = resized_shape(*page.shape)
    assert shape == (1181, 835)
    outs, rest = _run(eng, [page], [shape])
    assert np.array_equal(outs[0], resize_page_host(page, *shape)) and np.all(rest == GUARD)


def test_a_600_dpi_white_page_stays_white(eng):
    """S = 255 * 7016 * 4961 passes 2^32: the sum and the final division are 64-bit"""
    page = np.full((7016, 4961), 255, np.uint8)
    assert 255 * page.size > 2 ** 32
    outs, rest = _run(eng, [page], [(1181, 835)])
    assert np.all(outs[0] == 255) and np.all(rest == GUARD)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _tutorial():
    return np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]


@pytest.fixture(scope="module")
def recognizer():
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    real = lambda name: omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_%s_params.npz" % name))
    return build_recognizer(real("system"), real("bar"))


def _one_piece_dir(root, name, page):
    from PIL import Image
    d = root / name / "a_piece" / "sheet"
    d.mkdir(parents=True)
    Image.fromarray(page).save(str(d / "01.png"))
    return str(root / name)


def test_device_pages_resized_returns_the_tutorial_page(recognizer):
    from audio_sheet_retrieval_amd.sheet_utils.omr import DevicePages, resize_pages_dev
    page = _tutorial()
    assert page.shape == (1181, 835)
    big = np.repeat(np.repeat(page, 2, axis=0), 2, axis=1)
    eng = recognizer.system_detector.engine
    raw = DevicePages(eng, [big, page])
    try:
        small = raw.resized(835)
        try:
            assert small.engine is eng and len(small) == 2
            assert small.heights.tolist() == [1181, 1181] and small.widths.tolist() == [835, 835]
            assert small.offsets.tolist() == [0, 1181 * 835] and small.nbytes == 2 * 1181 * 835
            got = small.download()
            assert np.array_equal(got[0], page) and np.array_equal(got[1], page)     # reduced; copied
            assert np.array_equal(small.download_page(1), page)
        finally:
            small.free()
        assert np.array_equal(raw.download_page(0), big)                             # the source stays valid
    finally:
        raw.free()
    from_host = resize_pages_dev(eng, [big], 835)
    try:
        assert np.array_equal(from_host.download_page(0), page)
    finally:
        from_host.free()


def test_load_umc_sheets_reads_a_page_at_twice_the_resolution(recognizer, tmp_path):
    from audio_sheet_retrieval_amd.sheet_utils.umc import load_umc_sheets
    page = _tutorial()
    big = np.repeat(np.repeat(page, 2, axis=0), 2, axis=1)
    assert big.shape == (2362, 1670)
    plain_dir = _one_piece_dir(tmp_path, "plain", page)
    big_dir = _one_piece_dir(tmp_path, "big", big)
    names, paths, sheets = load_umc_sheets(plain_dir, omr=recognizer)
    assert names == ["a_piece"] and sheets[0].shape[0] == 160 and sheets[0].shape[1] > 1000
    for return_device in (False, True):
        for device_post in (False, True):
            res = load_umc_sheets(big_dir, omr=recognizer, return_device=return_device, device_post=device_post,
                                  page_width=835)
            assert res[0] == names and [os.path.basename(p) for p in res[1]] == ["a_piece"]
            assert len(res[2]) == 1 and res[2][0].dtype == np.uint8 and np.array_equal(res[2][0], sheets[0])
            if return_device:
                dev = res[3]
                try:
                    assert dev.shapes == [sheets[0].shape]
                    strip = dev.buf.download(sheets[0].shape, np.float32)
                    assert np.array_equal(strip, sheets[0].astype(np.float32))
                finally:
                    dev.buf.free()
            else:
                assert len(res) == 3
