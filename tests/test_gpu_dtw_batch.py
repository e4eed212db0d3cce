"""GPU: batched alignment DTW (asr_dtw_batch_dev / Engine.dtw_batch / alignment.compute_alignments) and the
audio2sheet_align driver - bit for bit against the oracle, asr_dtw_dev and the per-piece host pipeline."""
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _codes(rng, n_sheet, n_spec, noise=0.3):
    base = rng.standard_normal((max(n_sheet, n_spec), 32))
    s = base[np.linspace(0, len(base) - 1, n_sheet).astype(int)]
    a = base[np.linspace(0, len(base) - 1, n_spec).astype(int)] + noise * rng.standard_normal((n_spec, 32))
    f = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return f(s), f(a)


def _tie_heavy(rng, n_sheet, n_spec, n_distinct=4):
    """codes drawn from a handful of rows: many exactly equal distances, so the first-minimum order decides"""
    rows = rng.standard_normal((n_distinct, 32)).astype(np.float32)
    return rows[rng.integers(0, n_distinct, n_sheet)], rows[rng.integers(0, n_distinct, n_spec)]


SHAPES = [(90, 40), (40, 90), (64, 64), (1, 9), (9, 1), (300, 700)]


@pytest.fixture(scope="module")
def engine():
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine("mutopia_ccal_cont")
    yield eng
    eng.close()


def _pairs():
    rng = np.random.default_rng(11)
    pairs = [_codes(rng, *s) for s in SHAPES]
    pairs.append(_tie_heavy(rng, 120, 80))
    pairs.append(_tie_heavy(rng, 50, 130, n_distinct=2))
    return pairs


def test_batch_matches_oracle_bit_for_bit(engine):
    from audio_sheet_retrieval_amd import alignment as al
    from oracle import alignment as oa, retrieval as oret
    pairs = _pairs()
    res = al.dtw_by_dist_codes_batch(engine, pairs, first=True)
    for (sheet, spec), (md, dists, path, first) in zip(pairs, res):
        ref_d = oret.cdist_cosine64(sheet, spec)
        assert np.array_equal(dists, ref_d), sheet.shape
        rmd, _, _, rpath = oa.dtw_by_dist(ref_d)
        assert md == rmd, sheet.shape
        assert np.array_equal(path[0], rpath[0]) and np.array_equal(path[1], rpath[1]), sheet.shape
        loop = [int(np.flatnonzero(rpath[0] == col)[0]) for col in range(ref_d.shape[1])]
        assert np.array_equal(first, np.asarray(rpath[1])[loop]), sheet.shape
        assert np.array_equal(first, oa.align_pydtw(ref_d)), sheet.shape


def test_batch_matches_asr_dtw_dev_including_global_ring(engine, monkeypatch):
    """both first-entry sides, dists, min_dist and paths equal asr_dtw_dev's; ASR_DTW_LDS_CAP=40 sends every pair
    with min(n_a, n_b) >= 40 to the global-ring wavefront"""
    from audio_sheet_retrieval_amd import alignment as al
    pairs = [(a, b) for a, b in _pairs()]
    for cap in (None, "40"):
        if cap:
            monkeypatch.setenv("ASR_DTW_LDS_CAP", cap)
        res_a = engine.dtw_batch(pairs, want_dists=True, first_of="a")
        res_b = engine.dtw_batch(pairs, first_of="b")
        for (a, b), (md, d, pa, pb, fa), (md2, d2, pa2, pb2, fb) in zip(pairs, res_a, res_b):
            rmd, rd, rpa, rpb = engine.dtw(a, b)
            assert md == rmd and md2 == rmd and d2 is None
            assert np.array_equal(d, rd)
            for x, y in ((pa, rpa), (pb, rpb), (pa2, rpa), (pb2, rpb)):
                assert np.array_equal(x, y), (a.shape, b.shape, cap)
            assert np.array_equal(fa, rpb[al.first_entries(rpa, len(a))])
            assert np.array_equal(fb, rpa[al.first_entries(rpb, len(b))])


def test_batch_above_the_lds_cap(engine):
    """a pair whose diagonals exceed one workgroup's LDS (min side 7000 > 6825 on gfx950) = asr_dtw_dev"""
    rng = np.random.default_rng(2)
    a, b = _codes(rng, 7000, 7200, noise=0.5)
    ((md, _, pa, pb),) = engine.dtw_batch([(a, b)])
    rmd, _, rpa, rpb = engine.dtw(a, b, want_dists=False)
    assert md == rmd and np.array_equal(pa, rpa) and np.array_equal(pb, rpb)


def test_pairs_are_independent_of_the_batch(engine, monkeypatch):
    pairs = _pairs()
    alone = [engine.dtw_batch([p], want_dists=True, first_of="b")[0] for p in pairs]
    together = engine.dtw_batch(pairs, want_dists=True, first_of="b")
    reverse = engine.dtw_batch(pairs[::-1], want_dists=True, first_of="b")[::-1]
    monkeypatch.setenv("ASR_DTW_BUDGET_MB", "1")          # one chunk per pair
    chunked = engine.dtw_batch(pairs, want_dists=True, first_of="b")
    for x, y, z, w in zip(alone, together, reverse, chunked):
        assert x[0] == y[0] == z[0] == w[0]
        for k in range(1, 5):
            assert np.array_equal(x[k], y[k]) and np.array_equal(x[k], z[k]) and np.array_equal(x[k], w[k])


def test_reference_golden_cases_through_compute_alignments(engine):
    from audio_sheet_retrieval_amd import alignment as al
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_golden.npz"), allow_pickle=True)
    cases = ("dtw_tall", "dtw_wide", "dtw_square")
    for by in ("baseline", "pydtw"):
        pieces = [(g[c + "/sheet"], g[c + "/spec"], g[c + "/sheet_idxs"], g[c + "/spec_idxs"]) for c in cases]
        for c, (m, res) in zip(cases, al.compute_alignments(engine, pieces, by)):
            key = "%s/%s/" % (c, by)
            assert np.array_equal(res["aligned_sheet_idxs"], g[key + "aligned_idxs"]), key
            assert np.array_equal(res["i_inter"], g[key + "i_inter"]), key
            assert np.array_equal(res["a2s_alignment"], g[key + "a2s"]), key
            err = al.estimate_alignment_error(g[key + "truth"], g[key + "onsets"], m)
            assert np.array_equal(err, g[key + "errors"]), key
            single = al.compute_alignment(engine, *pieces[cases.index(c)], by)[1]
            for k in ("dists", "aligned_sheet_idxs", "aligned_sheet_coords", "i_inter", "a2s_alignment"):
                assert np.array_equal(res[k], single[k]), (key, k)


def test_bad_sizes_are_rejected_with_a_message(engine):
    from audio_sheet_retrieval_amd import _lib
    ok = np.ones((5, 32), np.float32)
    bad = [[(np.ones((0, 32), np.float32), ok)], [(ok, np.ones((0, 32), np.float32))],
           [(np.ones((5, 65), np.float32), np.ones((5, 65), np.float32))],
           [(ok, ok), (np.ones((100001, 2), np.float32)[:, :1].repeat(32, 1), ok[:1])]]
    for pairs in bad[:3]:
        with pytest.raises(_lib.AsrError, match="dtw_batch"):
            engine.dtw_batch(pairs)
    with pytest.raises(_lib.AsrError, match="pair 1 has bad sizes"):
        engine.dtw_batch(bad[3])
    assert engine.dtw_batch([(ok, ok)])[0][0] == engine.dtw(ok, ok)[0]    # the context still works


# ---- the driver ---------------------------------------------------------------------------------------------------
SPLIT, CONFIG = "splits/all_split.yaml", "exp_configs/mutopia_full_aug.yaml"
TAG = "all_split_mutopia_full_aug"


def _host_pipeline(engine, images, specs, o2c_maps, align_by, sheet_step=10, spec_step=2):
    """the reference's loop (:80-172): host NumPy slicing, per-piece embedding, oracle alignment"""
    from audio_sheet_retrieval_amd import alignment as al
    from oracle import alignment as oa
    out = []
    for sheet, (spec,), (o2c,) in zip(images, specs, o2c_maps):
        n = spec.shape[1] // spec_step
        spec_idxs = np.linspace(21, spec.shape[1] - 21, n).astype(np.int32)
        n = sheet.shape[1] // sheet_step
        sheet_idxs = np.linspace(100, sheet.shape[1] - 100, n).astype(np.int32)
        r0 = sheet.shape[0] // 2 - 80
        sheet_slices = np.stack([sheet[r0:r0 + 160, x - 100:x + 100] for x in sheet_idxs])[:, None]
        spec_slices = np.stack([spec[:, o - 21:o + 21] for o in spec_idxs])[:, None]
        img_codes = engine.embed_view1(sheet_slices, prepared=False)
        spec_codes = engine.embed_view2(spec_slices)
        m, res = oa.compute_alignment(img_codes, spec_codes, sheet_idxs, spec_idxs, align_by)
        err = al.estimate_alignment_error(o2c[:, 1], o2c[:, 0], m)
        out.append((img_codes, spec_codes, sheet_idxs, spec_idxs, m, res, err))
    return out


@pytest.mark.parametrize("align_by", ["baseline", "pydtw"])
def test_driver_matches_the_per_piece_host_pipeline(tmp_path, monkeypatch, align_by):
    from audio_sheet_retrieval_amd import audio2sheet_align as drv, network
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.data_pools import AudioScoreRetrievalPool
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    monkeypatch.setattr(drv, "EXP_ROOT", str(tmp_path))
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        params = [z["p%02d" % i] for i in range(len(param_shapes("mutopia_ccal_cont")))]
    d = tmp_path / "mutopia_ccal_cont"
    d.mkdir()
    with open(d / ("params_%s.pkl" % TAG), "wb") as fp:
        pickle.dump(params, fp, protocol=2)
    res = drv.main(["--model", "models/mutopia_ccal_cont.py", "--data", "synthetic:3", "--align_by", align_by,
                    "--train_split", SPLIT, "--config", CONFIG])
    dumped = pickle.load(open(d / ("alignment_res_%s_%s.pkl" % (TAG, align_by)), "rb"))
    assert sorted(dumped) == ["synthetic_000", "synthetic_001", "synthetic_002"]

    # the same pieces through the host pipeline, on an engine holding the same parameters
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine("mutopia_ccal_cont")
    eng.set_params(params)
    images, specs, o2c_maps = synth_data.synth_pieces(3)
    ref = _host_pipeline(eng, images, specs, o2c_maps, align_by)
    pool = AudioScoreRetrievalPool(eng, images, specs, o2c_maps, shuffle=False)
    pieces, results, errors = drv.align_pieces(eng, pool, align_by)
    for k, (img, spc, si, sp, m, r, err) in enumerate(ref):
        name = "synthetic_%03d" % k
        assert np.array_equal(pieces[k]["img_codes"], img) and np.array_equal(pieces[k]["spec_codes"], spc), name
        assert np.array_equal(pieces[k]["sheet_idxs"], si) and np.array_equal(pieces[k]["spec_idxs"], sp), name
        for key in ("aligned_sheet_idxs", "aligned_sheet_coords", "i_inter", "a2s_alignment"):
            assert np.array_equal(results[k][1][key], r[key]), (name, key)
        assert results[k][0] == m
        assert np.array_equal(errors[k], err) and np.array_equal(dumped[name], err) and np.array_equal(res[name], err)
    eng.close()
