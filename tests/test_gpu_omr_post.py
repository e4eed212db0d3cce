"""GPU: systems_from_maps on the device (asr_systems_from_maps_dev, OpticalMusicRecognizer.detect_systems_pages_dev,
load_umc_sheets(device_post=True)) against the host path, sheet_utils/omr.py systems_from_maps, on the same arrays.
The yardstick is equality of the integers.  A page the device does not decide (status 3) is not an error, but the
share of such pages is capped, and so is the share of cases on which the host itself finds nothing.

The real-network test also passes pages whose *network maps* - not the post-processing - are what the first version of
this feature had never seen (all-white, all-zero, flipped pages): whatever the maps are, the two paths must agree."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import omr_post_cases as cases  # noqa: E402
import omr_ref  # noqa: E402


def _engine():
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    return O._engine(0)


def _host(case):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    try:
        return O.systems_from_maps(O.prepare_image(case["page"]), case["system"], case["bar"])
    except Exception as e:
        return e


def _device(eng, batch, with_bar):
    """one asr_systems_from_maps_dev call on a list of cases (all with, or all without, a bar map)"""
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    pages = O.DevicePages(eng, [c["page"] for c in batch])
    sys_buf = eng.alloc(pages.nbytes * 8).upload(np.concatenate([c["system"].ravel() for c in batch]))
    bar_buf = eng.alloc(pages.nbytes * 8).upload(np.concatenate([c["bar"].ravel() for c in batch])) if with_bar else None
    try:
        res, passes = O.systems_from_maps_dev(eng, pages.buf.ptr, O.IN_U8_RAW, pages.offsets, pages.heights,
                                              pages.widths, sys_buf.ptr, bar_buf.ptr if with_bar else None)
    finally:
        pages.free()
        sys_buf.free()
        if bar_buf is not None:
            bar_buf.free()
    assert passes >= 1
    return res


def _agree(dev, host, what):
    """a wrong answer fails; -> 'ok' (status 0 with a system), 'empty', 'raised' or 'fallback'"""
    st, corners = dev
    if st == 3:
        return "fallback"
    if st == 1:
        assert isinstance(host, IndexError), (what, host)
        return "raised"
    if st == 2:
        assert isinstance(host, ValueError), (what, host)
        return "raised"
    assert st == 0 and not isinstance(host, Exception), (what, st, host)
    assert corners.dtype == host.dtype and corners.shape == host.shape, (what, corners.shape, host.shape)
    assert np.array_equal(corners, host), (what, corners, host)
    return "ok" if len(host) else "empty"


def test_crafted_maps_match_the_host(monkeypatch):
    eng = _engine()
    all_cases = [cases.make_case(s) for s in range(cases.N_CASES)]
    assert {c["scenario"] for c in all_cases} == set(cases.SCENARIOS)
    host = [_host(c) for c in all_cases]
    host_ok = sum(1 for r in host if not isinstance(r, Exception) and len(r) > 0)
    print("host finds a system on %d of %d cases" % (host_ok, len(all_cases)))
    assert host_ok >= 0.9 * len(all_cases)                                   # the comparison is not vacuous
    # the exact-area case: the 50000-pixel blob is kept, the 49999-pixel one is not
    for s in (4, 24):                                                        # (the two without a bar map)
        assert all_cases[s]["scenario"] == "area_edge" and all_cases[s]["bar"] is None and len(host[s]) == 2, (s, host[s])

    tally = {"ok": 0, "empty": 0, "raised": 0, "fallback": 0}
    together = {}
    for with_bar in (False, True):
        idx = [i for i, c in enumerate(all_cases) if (c["bar"] is not None) == with_bar]
        res = _device(eng, [all_cases[i] for i in idx], with_bar)               # pages of different shapes, one call
        for i, r in zip(idx, res):
            together[i] = r
            kind = _agree(r, host[i], (i, all_cases[i]["scenario"]))
            print(i, all_cases[i]["scenario"], all_cases[i]["page"].shape, "bar" if with_bar else "no bar", r[0], kind)
            tally[kind] += 1
    print(tally)
    assert tally["ok"] >= 0.9 * len(all_cases), tally
    assert tally["fallback"] <= 0.1 * len(all_cases), tally

    # every page alone gives what it gave in the batch (one of each scenario, with and without the bar map), and so
    # does the batch cut into one-page chunks
    for i in range(2 * len(cases.SCENARIOS)):
        c = all_cases[i]
        alone = _device(eng, [c], c["bar"] is not None)[0]
        assert alone[0] == together[i][0], (i, alone[0], together[i][0])
        if alone[0] == 0:
            assert np.array_equal(alone[1], together[i][1]), i
    monkeypatch.setenv("ASR_OMR_BUDGET_MB", "16")
    idx = [i for i in range(cases.N_CASES) if all_cases[i]["bar"] is None][:6]
    for i, r in zip(idx, _device(eng, [all_cases[i] for i in idx], False)):
        assert r[0] == together[i][0] and (r[0] != 0 or np.array_equal(r[1], together[i][1])), i


def test_capacity_is_checked_by_the_library():
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    eng = _engine()
    c = cases.make_case(0)
    h, w = c["page"].shape
    pages = O.DevicePages(eng, [c["page"]])
    maps = eng.alloc(h * w * 8).upload(c["system"])
    status, counts = np.zeros(1, np.int32), np.zeros(1, np.int32)
    systems = np.zeros((1, 64, 4), np.int32)
    try:
        rc = eng.lib.asr_systems_from_maps_dev(eng.ctx, pages.buf.ptr, 2, pages.offsets.ctypes.data,
                                               pages.heights.ctypes.data, pages.widths.ctypes.data, 1, maps.ptr, None,
                                               None, None, h * w // 50000 - 1, status.ctypes.data, counts.ctypes.data,
                                               systems.ctypes.data, None)
        assert rc == _lib.ASR_ERR_INVALID
    finally:
        pages.free()
        maps.free()


def test_more_pages_than_one_launch_grid_holds():
    """70000 pages of 3 x 8 pixels (the smallest the device decides) are far below the workspace budget but more than
    the y dimension of a launch grid (65535): the call cuts them into chunks, and every copy of the page gives what
    the page gives alone"""
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    eng = _engine()
    rng = np.random.default_rng(5)
    n, h, w = 70000, 3, 8
    case = dict(page=rng.integers(0, 256, size=(h, w)).astype(np.uint8), system=rng.random((h, w)), bar=None)
    pages = O.DevicePages(eng, [case["page"]])
    maps = eng.alloc(n * h * w * 8).upload(np.tile(case["system"].ravel(), n))
    try:
        args = (eng, pages.buf.ptr, O.IN_U8_RAW)
        (alone,), _ = O.systems_from_maps_dev(*args, pages.offsets, pages.heights, pages.widths, maps.ptr)
        res, _ = O.systems_from_maps_dev(*args, np.repeat(pages.offsets, n), np.repeat(pages.heights, n),
                                         np.repeat(pages.widths, n), maps.ptr)
    finally:
        pages.free()
        maps.free()
    _agree(alone, _host(case), "3 x 8")
    assert len(res) == n
    assert {r[0] for r in res} == {alone[0]}
    if alone[0] == 0:
        assert all(np.array_equal(r[1], alone[1]) for r in res)


def _real(name):
    return omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_%s_params.npz" % name))


def _tutorial():
    return np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]


def _omr():
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    return build_recognizer(_real("system"), _real("bar"))


def _synthetic_page(seed, h, w):
    """a seeded score-like page: white, dark horizontal line groups and blobs, uint8"""
    rng = np.random.default_rng(seed)
    p = np.full((h, w), 255, np.uint8)
    for top in range(20 + int(rng.integers(0, 20)), h - 60, 120):
        for k in range(5):
            p[top + 8 * k, 10:w - 10] = 0
        for x in rng.integers(20, max(21, w - 20), size=max(1, w // 40)):
            y = top + int(rng.integers(0, 32))
            p[y:y + 6, x:x + 8] = 30
    return np.clip(p.astype(int) + rng.integers(-8, 8, size=p.shape), 0, 255).astype(np.uint8)


def _same(a, b, what):
    if isinstance(b, Exception):
        assert type(a) is type(b), (what, a, b)
    else:
        assert not isinstance(a, Exception), (what, a)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, a, b)


def test_real_networks_match_detect_systems_pages():
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    page = _tutorial()
    canvas = np.full((1300, 900), 255, np.uint8)
    r0, c0 = (1300 - page.shape[0]) // 2, (900 - page.shape[1]) // 2
    canvas[r0:r0 + page.shape[0], c0:c0 + page.shape[1]] = page
    pages = [page, np.ascontiguousarray(page[:, ::-1]), np.ascontiguousarray(page[::-1]), canvas,
             np.ascontiguousarray(page[:600]), np.full_like(page, 255), np.zeros_like(page),
             _synthetic_page(11, 900, 700), _synthetic_page(12, 512, 512)]
    rec = _omr()
    host = rec.detect_systems_pages(pages, in_mode=O.IN_U8_RAW)
    dev = rec.detect_systems_pages_dev(pages, in_mode=O.IN_U8_RAW)
    print("fallback pages", rec.last_fallback_pages, "labelling passes", rec.last_label_passes)
    assert len(dev) == len(host) == len(pages)
    for i, (a, b) in enumerate(zip(dev, host)):
        print(i, pages[i].shape, type(b).__name__ if isinstance(b, Exception) else len(b))
        _same(a, b, i)
    assert len(host[0]) == 6 and len(host[1]) == 6
    assert 8 in rec.last_fallback_pages
    assert 0 not in rec.last_fallback_pages and 1 not in rec.last_fallback_pages
    # the pages already on the device
    dp = O.DevicePages(rec.system_detector.engine, pages)
    try:
        again = rec.detect_systems_pages_dev(pages, in_mode=O.IN_U8_RAW, dev_pages=dp)
    finally:
        dp.free()
    for i, (a, b) in enumerate(zip(again, dev)):
        _same(a, b, i)
    # prepared float32 pages (in_mode 0)
    prep = [O.prepare_image(p) for p in pages[:2]]
    for i, (a, b) in enumerate(zip(rec.detect_systems_pages_dev(prep, in_mode=O.IN_F32_PREPARED), host[:2])):
        _same(a, b, i)


@pytest.mark.parametrize("return_device", [False, True])
def test_load_umc_sheets_device_post(tmp_path, capsys, return_device):
    from PIL import Image
    from audio_sheet_retrieval_amd.sheet_utils.umc import load_umc_sheets
    page = _tutorial()
    for name, pages in [("a_piece", [page, page]), ("b_blank", [np.zeros_like(page)]), ("c_nosheet", None)]:
        d = tmp_path / name
        d.mkdir()
        if pages is None:
            continue
        (d / "sheet").mkdir()
        for i, p in enumerate(pages):
            Image.fromarray(p).save(str(d / "sheet" / ("%02d.png" % (i + 1))))
    rec = _omr()
    outs = []
    for device_post in (False, True):
        res = load_umc_sheets(str(tmp_path), omr=rec, return_device=return_device, device_post=device_post)
        outs.append((res, capsys.readouterr().out))
        if return_device:
            res[3].buf.free()
    (a, msg_a), (b, msg_b) = outs
    assert a[0] == b[0] == ["a_piece"] and a[1] == b[1]
    assert len(a[2]) == len(b[2]) == 1 and a[2][0].shape[1] > 0
    assert a[2][0].dtype == b[2][0].dtype and np.array_equal(a[2][0], b[2][0])
    assert msg_a == msg_b and "Problem in system detection!!!" in msg_a
    if return_device:
        assert a[3].offsets == b[3].offsets and a[3].shapes == b[3].shapes
