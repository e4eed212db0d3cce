"""GPU: the UMC piece-identification path (umc_a2s_server / umc_s2a_server) - every batched device call against the
per-item path it replaces, bit for bit: the unrolled strips against unwrap_systems + hstack, the batched spectrograms
against process(), the data bases against a host loop over the reference's windows, and both drivers against
detect_score / detect_performance per piece.

Fixture pages are derived from the tutorial page; each derived page was run through the CPU restatement
(tests/omr_ref.py + omr.systems_from_maps, as test_omr_host.test_page_anchor_six_systems does) before it was relied on:
the page and the page with systems painted white yield systems, the page cropped 14 rows above the end of its last
system's 160-row band (1145 rows) yields that system edge-padded by 14 rows (a crop of 10 rows moves the detected
system so that it is skipped instead), the black page raises (the "problem" page).  Retrieval quality is
not asserted: the model weights are synthetic."""
import os
import pickle
import sys

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import omr_ref  # noqa: E402

SPLIT, CONFIG = "splits/all_split.yaml", "exp_configs/mutopia_full_aug.yaml"
TAG = "all_split_mutopia_full_aug"
MODEL = "mutopia_ccal_cont"
SR = 22050


def _real(name):
    return omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_%s_params.npz" % name))


def _tutorial():
    return np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]


def _omr():
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    return build_recognizer(_real("system"), _real("bar"))


def _engine():
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    eng = _lib.Engine(MODEL, device=0)
    eng.set_params(synth_data.synth_params(param_shapes(MODEL), seed=1, trained_like=True))
    return eng


def _download(dev):
    total = sum(r * c for r, c in dev.shapes)
    flat = dev.buf.download((total,), np.float32) if total else np.zeros(0, np.float32)
    return [flat[o:o + r * c].reshape(r, c) for o, (r, c) in zip(dev.offsets, dev.shapes)]


def _white(page, systems, which):
    q = page.copy()
    for k in which:
        q[max(0, int(systems[k][0, 0]) - 25):int(systems[k][2, 0]) + 25] = 255
    return q


def _cropped(page, systems, missing=14):
    """the page cut `missing` rows above the end of the last system's 160-row band: that system needs edge padding"""
    last = systems[-1]
    return np.ascontiguousarray(page[:int(np.mean([last[0, 0], last[2, 0]])) + 80 - missing])


# ---- unroll ----------------------------------------------------------------------------------------------------------
def test_unroll_parity(capsys):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    page = _tutorial()
    rec = _omr()
    base = rec.detect_systems(O.prepare_image(page))
    crop = _cropped(page, base)
    # pieces: the page alone, two pages, a piece whose second page has a clipped last system
    pieces = [[page], [page, _white(page, base, [1, 3])], [page, crop]]
    pages = [p for piece in pieces for p in piece]
    piece_of_page = [i for i, piece in enumerate(pieces) for _ in piece]
    dev_pages = O.DevicePages(rec.system_detector.engine, pages)
    systems = rec.detect_systems_pages(pages, in_mode=O.IN_U8_RAW, dev_pages=dev_pages)
    assert not any(isinstance(s, Exception) for s in systems), systems
    # pages on the device give the networks the same input as uploaded pages
    again = rec.detect_systems_pages(pages, in_mode=O.IN_U8_RAW)
    assert all(np.array_equal(a, b) for a, b in zip(systems, again))
    rows = [O.unroll_rows(p.shape, s) for p, s in zip(pages, systems)]
    assert any(r[4] > 0 for r in rows[-1]), ("the cropped page has no edge-padded system", rows[-1])
    buf, offsets, shapes = O.unroll_systems_dev(dev_pages, rows, piece_of_page, len(pieces))
    dev_pages.free()
    from audio_sheet_retrieval_amd.piece_identification import DeviceArrays
    strips = _download(DeviceArrays(buf, offsets, shapes))
    buf.free()
    k = 0
    for piece, strip in zip(pieces, strips):
        want = np.hstack([O.unwrap_systems(p, systems[k + j]) for j, p in enumerate(piece)])
        k += len(piece)
        assert strip.dtype == np.float32 and strip.shape == want.shape and want.shape[1] > 4000
        assert np.array_equal(strip.astype(np.uint8), want) and np.array_equal(strip, want.astype(np.float32))


def test_unroll_hand_made_systems(capsys):
    """systems that no detection produced: clipped at the top, padded by 16 rows, skipped by 17, one column wide,
    columns beyond the page - against unwrap_systems"""
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import omr as O

    def system(top, bottom, left, right):
        s = np.zeros((4, 2))
        s[0], s[1], s[2], s[3] = (top, left), (top, right), (bottom, right), (bottom, left)
        return s
    rng = np.random.default_rng(9)
    pages = [rng.integers(0, 256, size=(600, 501)).astype(np.uint8), rng.integers(0, 256, size=(333, 257)).astype(np.uint8)]
    systems = [np.asarray([system(200, 300, 20, 480), system(60, 90, 30, 400), system(500, 572, 5, 333),
                           system(500, 574, 5, 333), system(300, 420, 250, 251), system(100, 200, 400, 900)]),
               np.asarray([system(250, 340, 0, 257), system(0, 20, 3, 200), system(100, 200, 17, 18.5)])]
    eng = _lib.Engine(MODEL, device=0)
    dev_pages = O.DevicePages(eng, pages)
    rows = [O.unroll_rows(p.shape, s) for p, s in zip(pages, systems)]
    capsys.readouterr()
    for piece_of_page, n_pieces in (([0, 1], 2), ([0, 0], 1), ([1, 0], 2)):
        buf, offsets, shapes = O.unroll_systems_dev(dev_pages, rows, piece_of_page, n_pieces)
        from audio_sheet_retrieval_amd.piece_identification import DeviceArrays
        strips = _download(DeviceArrays(buf, offsets, shapes))
        buf.free()
        for q in range(n_pieces):
            want = np.hstack([O.unwrap_systems(p, s) for p, s, owner in zip(pages, systems, piece_of_page) if owner == q])
            assert strips[q].shape == want.shape and np.array_equal(strips[q], want.astype(np.float32)), (piece_of_page, q)
    # a table that leaves the page or the strip is refused before anything runs
    bad = np.asarray([[0, 500, 660, 0, 10, 0, 0, 0]], np.int32)
    out = eng.alloc(160 * 10 * 4)
    with pytest.raises(_lib.AsrError, match="do not fit"):
        eng.unroll_systems_dev(dev_pages.buf.ptr, dev_pages.nbytes, dev_pages.offsets, dev_pages.heights, dev_pages.widths,
                               bad, 160, [0], [10], out.ptr, 1600)
    bad = np.asarray([[0, 100, 260, 0, 11, 0, 0, 0]], np.int32)
    with pytest.raises(_lib.AsrError, match="outside strip"):
        eng.unroll_systems_dev(dev_pages.buf.ptr, dev_pages.nbytes, dev_pages.offsets, dev_pages.heights, dev_pages.widths,
                               bad, 160, [0], [10], out.ptr, 1600)
    out.free()
    dev_pages.free()
    eng.close()


# ---- spectrograms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_scale", [1.0, 1.0 / 32767])
def test_spectrogram_batch_parity(window_scale):
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    rng = np.random.default_rng(4)
    amp = 1.0 if window_scale == 1.0 else 20000.0
    recs = []
    for n in (0, 1, 2047, 2048, 22050, 100003, 661500):
        t = np.arange(n) / float(SR)
        x = np.sin(2 * np.pi * 440.0 * t) + 0.5 * np.sin(2 * np.pi * 1234.5 * t) + 0.1 * rng.standard_normal(n)
        recs.append((amp * x).astype(np.float32))
    eng = _lib.Engine(MODEL, device=0)
    proc = SpectrogramProcessor(eng, window_scale=window_scale)
    got = proc.process_many(recs)
    assert len(got) == len(recs)
    for r, g in zip(recs, got):
        want = proc.process(r)
        assert g.shape == want.shape == (92, proc.num_frames(r.size)) and g.dtype == np.float32
        assert np.array_equal(g, want), r.size
    assert got[0].shape == (92, 0) and got[1].shape == (92, 1) and got[-1].shape == (92, 600)
    assert float(np.abs(got[-1]).max()) > 0.1
    # the scale per recording (what load_audio returns) gives each recording its own window
    other = 1.0 / 32767 if window_scale == 1.0 else 1.0
    mixed = proc.process_many(recs[3:6], [window_scale, other, window_scale])
    assert np.array_equal(mixed[0], got[3]) and np.array_equal(mixed[2], got[5])
    assert np.array_equal(mixed[1], SpectrogramProcessor(eng, window_scale=other).process(recs[4]))
    # nothing in, nothing out
    assert proc.process_many([]) == []
    empty = proc.process_many([recs[0], recs[0]])
    assert [e.shape for e in empty] == [(92, 0), (92, 0)]
    eng.close()


# ---- data bases ------------------------------------------------------------------------------------------------------
def _host_db(engine, arrays, view, win, max_windows):
    """the reference's loops (audio_sheet_server.py:413-443, :457-492) with the windows sliced on the host, embedded by
    the existing host entry points in chunks of max_windows"""
    h, w = win
    windows, ids = [], []
    for i, a in enumerate(arrays):
        indices = np.arange(0, a.shape[1] - w, w // 4)
        r0 = a.shape[0] // 2 - h // 2 if view == 1 else 0
        for c in indices:
            windows.append(np.asarray(a[r0:r0 + h, c:c + w], np.float32))
        ids += [i] * len(indices)
    windows = np.stack(windows)[:, None]
    chunk = min(len(windows), max_windows)
    codes = []
    for s in range(0, len(windows), chunk):
        x = windows[s:s + chunk]
        codes.append(engine.embed_view1(x, prepared=False) if view == 1 else engine.embed_view2(x))
    return np.concatenate(codes), np.asarray(ids, np.int32)


def _strips_and_specs(engine):
    rng = np.random.default_rng(21)
    strips = [rng.integers(0, 256, size=(160, W)).astype(np.uint8) for W in (1500, 200, 930, 150, 451)]
    specs = [rng.random((92, T)).astype(np.float32) for T in (300, 42, 95, 30, 43)]
    return strips, specs


@pytest.mark.parametrize("max_windows", [4096, 7])
def test_data_base_parity(tmp_path, max_windows):
    from audio_sheet_retrieval_amd.piece_identification import EmbeddingDB, _to_device
    eng = _engine()
    strips, specs = _strips_and_specs(eng)
    names = ["piece_%d" % i for i in range(5)]
    for view, arrays, build, win in ((1, strips, EmbeddingDB.from_images, (160, 200)),
                                     (2, specs, EmbeddingDB.from_specs, (92, 42))):
        db = build(eng, names, arrays, max_windows=max_windows)
        codes, ids = _host_db(eng, arrays, view, win, max_windows)
        assert db.codes.shape == codes.shape and np.array_equal(db.codes, codes), view
        assert np.array_equal(db.ids, ids) and set(ids) == {0, 2, 4}          # pieces 1 and 3: W <= w, no window
        assert db.id_to_name == dict(enumerate(names))
        assert db.snippets.shape == (0, win[0] // 2, win[1] // 2) and db.snippets.dtype == np.uint8
        # device-handle input
        dev, owned = _to_device(eng, arrays)
        assert owned
        db2 = build(eng, names, dev, max_windows=max_windows)
        dev.buf.free()
        assert np.array_equal(db2.codes, db.codes) and np.array_equal(db2.ids, db.ids)
        # save / load: the reference's pickle layout
        path = str(tmp_path / ("db%d_%d.pkl" % (view, max_windows)))
        db.save(path)
        with open(path, "rb") as fp:
            raw = pickle.load(fp)
        assert len(raw) == 4 and np.array_equal(raw[0], db.codes) and raw[2] == db.id_to_name
        db3 = EmbeddingDB.load(eng, path)
        assert np.array_equal(db3.codes, db.codes) and np.array_equal(db3.ids, db.ids) and db3.id_to_name == db.id_to_name
        for d in (db, db2, db3):
            d.close()
    with pytest.raises(ValueError, match="names"):
        EmbeddingDB.from_images(eng, names[:2], strips)
    eng.close()


def test_detect_batch_device_handle_equals_host_input():
    from audio_sheet_retrieval_amd.piece_identification import (EmbeddingDB, _to_device, detect_performances,
                                                                detect_scores)
    eng = _engine()
    strips, specs = _strips_and_specs(eng)
    strips, specs = [strips[i] for i in (0, 2, 4)], [specs[i] for i in (0, 2, 4)]
    names = ["a", "b", "c"]
    sheet_db = EmbeddingDB.from_images(eng, names, strips)
    audio_db = EmbeddingDB.from_specs(eng, names, specs)
    targets = np.arange(3, dtype=np.int32)
    for detect, db, arrays in ((detect_scores, sheet_db, specs), (detect_performances, audio_db, strips)):
        host = detect(eng, db, arrays, top_k=3, n_candidates=5, n_samples=20, targets=targets, max_windows=17)
        dev, _ = _to_device(eng, arrays)
        got = detect(eng, db, dev, top_k=3, n_candidates=5, n_samples=20, targets=targets, max_windows=17)
        dev.buf.free()
        assert np.array_equal(host[1], got[1]) and np.array_equal(host[2], got[2])
        for (n1, v1), (n2, v2) in zip(host[0], got[0]):
            assert n1 == n2 and np.array_equal(v1, v2)
    sheet_db.close()
    audio_db.close()
    eng.close()


# ---- the drivers -----------------------------------------------------------------------------------------------------
@pytest.fixture()
def exp_root(tmp_path, monkeypatch):
    from audio_sheet_retrieval_amd import audio2sheet_align
    from audio_sheet_retrieval_amd.config import settings
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    root = tmp_path / "exp"
    root.mkdir()
    for mod in (settings, audio2sheet_align):
        monkeypatch.setattr(mod, "EXP_ROOT", str(root))
    (root / MODEL).mkdir()
    with open(root / MODEL / ("params_%s.pkl" % TAG), "wb") as fp:
        pickle.dump(synth_data.synth_params(param_shapes(MODEL), seed=1, trained_like=True), fp, protocol=2)
    for name in ("system", "bar"):                   # the OMR parameters as the pickles the drivers are pointed at
        with open(root / ("%s_params.pkl" % name), "wb") as fp:
            pickle.dump(_real(name), fp, protocol=2)
    work = tmp_path / "work"
    work.mkdir()
    monkeypatch.chdir(work)
    return root


def _omr_flags(exp_root):
    return ["--system_params", str(exp_root / "system_params.pkl"), "--bar_params", str(exp_root / "bar_params.pkl")]


def _tone(seed, seconds, dtype):
    rng = np.random.default_rng(seed)
    n = int(seconds * SR)
    t = np.arange(n) / float(SR)
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in
            zip(rng.uniform(0.1, 0.4, 4), rng.uniform(80, 3000, 4), rng.uniform(0, 6, 4)))
    x = x / np.abs(x).max() * 0.8
    return (x * 32767).astype(np.int16) if dtype == np.int16 else x.astype(np.float32)


def _umc_dir(root):
    """eight folders: five pieces are kept, four of them have score_ppq.*"""
    from PIL import Image
    from scipy.io import wavfile
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    page = _tutorial()
    base = _omr().detect_systems(O.prepare_image(page))
    w13, w045 = _white(page, base, [1, 3]), _white(page, base, [0, 4, 5])
    layout = [
        # name, pages (None: no sheet folder), score_ppq (dtype, seconds, extension), performance
        ("p1_page", [page], (np.int16, 3.0, ".wav"), True),
        ("p2_two_pages", [w13, page], (np.float32, 4.0, ".wav"), True),
        ("p3_white", [w045], (np.int16, 2.5, ".npy"), True),
        ("p4_blank_page", [page, np.zeros_like(page)], (np.int16, 3.0, ".wav"), True),
        ("p5_no_sheet", None, (np.int16, 3.0, ".wav"), True),
        ("p6_no_performance", [page], (np.int16, 3.0, ".wav"), False),
        ("p7_no_score_ppq", [w13], None, True),
        ("p8_cropped", [_cropped(page, base), w045], (np.int16, 5.0, ".wav"), True),
    ]
    data = root / "umc_test"
    data.mkdir()
    for k, (name, pages, ppq, perf) in enumerate(layout):
        d = data / name
        d.mkdir()
        if pages is not None:
            (d / "sheet").mkdir()
            for i, p in enumerate(pages):
                Image.fromarray(p).save(str(d / "sheet" / ("%02d.png" % (i + 1))))
        if ppq is not None:
            dtype, seconds, ext = ppq
            x = _tone(100 + k, seconds, dtype)
            if ext == ".npy":
                np.save(str(d / "score_ppq.npy"), _tone(100 + k, seconds, np.float32))
            else:
                wavfile.write(str(d / ("score_ppq" + ext)), SR, x)
            (d / "score_ppq.flac").write_bytes(b"fLaC")                  # next to it, as in the reference's data
        if perf:
            wavfile.write(str(d / "01_performance.wav"), SR, _tone(200 + k, 2.2 + 0.3 * k, np.int16))
    return str(data)


KEPT = ["p1_page", "p2_two_pages", "p3_white", "p7_no_score_ppq", "p8_cropped"]


def _per_item(direction, data_dir, real_perf, n_candidates):
    """the per-item path on the same data: host strips (unwrap_systems + hstack), one process() per recording, the
    data base by the host loop, detect_score / detect_performance per piece, the reference's rank rule"""
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor, load_audio
    from audio_sheet_retrieval_amd.piece_identification import (EmbeddingDB, detect_performance, detect_score,
                                                                full_eval_rank)
    from audio_sheet_retrieval_amd.sheet_utils import umc
    names, paths, sheets = umc.load_umc_sheets(data_dir, require_performance=True, omr=_omr())
    eng = _engine()
    pattern = "01_performance" if real_perf else "score_ppq"
    specs = {}
    for name, path in zip(names, paths):
        try:
            samples, scale = load_audio(umc.get_performance_audio_path(path, pattern))
        except IndexError:
            continue
        specs[name] = SpectrogramProcessor(eng, window_scale=scale).process(samples)
    if direction == "A2S":
        codes, ids = _host_db(eng, sheets, 1, (160, 200), 4096)
        queried = [n for n in names if n in specs]
    else:
        codes, ids = _host_db(eng, [specs[n] for n in names], 2, (92, 42), 4096)
        queried = list(names)
    db = EmbeddingDB(eng, codes, ids, dict(enumerate(names)))
    ranks, ratios = [], []
    for name in queried:
        if direction == "A2S":
            res, votes = detect_score(eng, db, specs[name], top_k=len(names), n_candidates=n_candidates)
        else:
            res, votes = detect_performance(eng, db, sheets[names.index(name)], top_k=len(names),
                                            n_candidates=n_candidates)
        rank, ratio = full_eval_rank(res, votes, name)
        ranks.append(rank)
        ratios.append(ratio)
    db.close()
    eng.close()
    return names, queried, ranks, ratios, codes, ids


@pytest.mark.parametrize("direction,real_perf", [("A2S", False), ("S2A", True), ("A2S", True)])
def test_driver_parity(exp_root, tmp_path, monkeypatch, capsys, direction, real_perf):
    from audio_sheet_retrieval_amd import umc_a2s_server, umc_s2a_server
    from audio_sheet_retrieval_amd.piece_identification import EmbeddingDB
    data_dir = _umc_dir(tmp_path)
    main = umc_a2s_server.main if direction == "A2S" else umc_s2a_server.main
    flag, db_file = (("--init_sheet_db", "umc_sheet_db_file.pkl") if direction == "A2S" else
                     ("--init_audio_db", "umc_audio_db_file.pkl"))
    common = ["--model", "models/%s.py" % MODEL, "--data_dir", data_dir, "--train_split", SPLIT, "--config", CONFIG,
              "--n_candidates", "9", "--full_eval"] + _omr_flags(exp_root) + (["--real_perf"] if real_perf else [])
    capsys.readouterr()
    ranks = main(common + [flag, "--dump_results"])
    text = capsys.readouterr().out

    # the pieces kept and the pieces ranked: fixed numbers
    n_ranked = 4 if (direction == "A2S" and not real_perf) else 5
    assert len(ranks) == n_ranked
    assert "5 pieces covering 9 pages of sheet music." in text        # 1 + 2 + 1 + 2 (p4) + 1 + 2
    assert text.count("Problem in system detection!!!") == 1 and text.count("No sheet available!!!") == 1
    assert text.count("No performance found!") == 1 and text.count("Problem in system padding!!!") == 0
    assert "Processing piece 8 of 8 (p8_cropped)" in text and "Experimental Tag: %s" % TAG in text

    names, queried, want_ranks, want_ratios, codes, ids = _per_item(direction, data_dir, real_perf, 9)
    capsys.readouterr()
    assert names == KEPT and len(queried) == n_ranked
    assert ("p7_no_score_ppq" in queried) == (n_ranked == 5)
    assert ranks == [int(r) for r in want_ranks]
    for name, rank, ratio in zip(queried, want_ranks, want_ratios):
        assert "rank: %02d (%.2f) %s\n" % (rank, ratio, name) in text
    assert text.count("rank: ") == n_ranked
    for r in sorted(set(want_ranks)):
        assert "%d of %d retrieved scores ranked at position %d." % (want_ranks.count(r), n_ranked, r) in text

    # the saved data base holds the per-item codes; the dump is the reference's file
    assert os.path.exists(db_file)
    eng = _engine()
    db = EmbeddingDB.load(eng, db_file)
    assert np.array_equal(db.codes, codes) and np.array_equal(db.ids, ids) and db.id_to_name == dict(enumerate(KEPT))
    db.close()
    eng.close()
    res_file = exp_root / MODEL / ("umc_retrieval_%s_umc_test_%s%s.yaml" % (TAG, direction, "_real" if real_perf else ""))
    with open(res_file) as fp:
        assert yaml.safe_load(fp) == ranks

    # a second run without the flag loads the data base and gives the same ranks
    os.remove(res_file)
    again = main(common)
    text2 = capsys.readouterr().out
    assert again == ranks and not os.path.exists(res_file)
    assert [l for l in text2.splitlines() if l.startswith(("rank: ", "rank <", "rank >"))] == \
        [l for l in text.splitlines() if l.startswith(("rank: ", "rank <", "rank >"))]


def test_s2a_names_the_piece_without_a_recording(exp_root, tmp_path, monkeypatch):
    from audio_sheet_retrieval_amd import umc_s2a_server
    data_dir = _umc_dir(tmp_path)
    with pytest.raises(IOError, match="p7_no_score_ppq"):
        umc_s2a_server.main(["--model", "models/%s.py" % MODEL, "--data_dir", data_dir, "--train_split", SPLIT,
                             "--config", CONFIG, "--init_audio_db", "--full_eval"] + _omr_flags(exp_root))


def test_load_umc_sheets_device_strips_equal_host_strips(tmp_path, capsys):
    from audio_sheet_retrieval_amd.sheet_utils import umc
    data_dir = _umc_dir(tmp_path)
    capsys.readouterr()
    names, paths, sheets = umc.load_umc_sheets(data_dir, require_performance=True, omr=_omr())
    host_text = capsys.readouterr().out
    names2, paths2, sheets2, dev = umc.load_umc_sheets(data_dir, require_performance=True, omr=_omr(), return_device=True)
    dev_text = capsys.readouterr().out
    strips = _download(dev)
    dev.buf.free()
    assert names2 == names == KEPT and paths2 == paths and dev_text == host_text
    for a, b, c in zip(sheets, sheets2, strips):
        assert b.dtype == np.uint8 and np.array_equal(a, b) and np.array_equal(c, a.astype(np.float32))
