"""GPU: training on raw sheet batches (asr_*_in, prepare_view1_kernel) gives the prepared route's results bit for bit -
the update, the burn-in, the gradients and the validation loss; the device pool feeds train() without a host copy of
the batch; run_train.py takes the raw route."""
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 32


@pytest.fixture(autouse=True)
def _model_schedules(monkeypatch):
    """the model's schedule picks in every context: timed picks may differ between two contexts, and with them the
    float32 summation order - the comparisons below are bit for bit"""
    monkeypatch.setenv("ASR_AUTOTUNE", "0")


def _batch(model, seed):
    from audio_sheet_retrieval_amd.models import _common
    from audio_sheet_retrieval_amd.utils import synth_data
    sheet_u8, spec = synth_data.synth_pairs(np.arange(seed * B, (seed + 1) * B), seed=23)
    prepare = _common.prepare_rsz if model.endswith("_rsz") else _common.prepare_plain
    return sheet_u8, prepare(sheet_u8), spec


def _run(model, params, route, batches):
    """fresh context, 3 updates, then one burn-in, compute_gradients and valid_loss call, all on `route`"""
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine(model)
    try:
        eng.set_params(params)
        u8, prep, spec = batches[0]
        eng.set_input_size(1, u8.shape[2], u8.shape[3])
        eng.train_begin(B)
        out = dict(steps=[])

        def x1_of(b):
            u8, prep, _ = b
            return {"prepared": prep, "u8": u8, "f32": u8.astype(np.float32)}[route]
        kw = dict(prepared=route == "prepared")
        for b in batches[:3]:
            out["steps"].append(eng.train_step(x1_of(b), b[2], 0.002, **kw))
        out["params"] = eng.get_params()
        out["opt"] = eng.get_opt_state()
        b = batches[3]
        out["burn_in"] = eng.burn_in(x1_of(b), b[2], **kw)
        out["grads"] = eng.compute_gradients(x1_of(b), b[2], **kw)
        out["params_after"] = eng.get_params()
        eng.train_end()
        out["valid"] = eng.valid_loss(x1_of(b), b[2], **kw)
        return out
    finally:
        eng.close()


def _assert_same(a, b, what):
    for (la, ca), (lb, cb) in zip(a["steps"], b["steps"]):
        assert la == lb and np.array_equal(ca, cb), what + ": loss / corr"
    for key in ("params", "params_after"):
        assert all(np.array_equal(p, q) for p, q in zip(a[key], b[key])), what + ": " + key
    assert np.array_equal(a["opt"]["m"], b["opt"]["m"]) and np.array_equal(a["opt"]["v"], b["opt"]["v"]), what
    assert a["opt"]["t"] == b["opt"]["t"] == 3
    assert all(np.array_equal(p, q) for p, q in zip(a["burn_in"], b["burn_in"])), what + ": burn-in"
    assert np.array_equal(a["grads"][0], b["grads"][0]) and a["grads"][1] == b["grads"][1], what + ": gradients"
    assert a["valid"] == b["valid"], what + ": valid loss"


@pytest.mark.parametrize("model", ["mutopia_ccal_cont", "mutopia_ccal_cont_rsz"])
def test_raw_routes_are_bit_identical_to_the_prepared_route(model):
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    params = synth_data.synth_params(param_shapes(model), seed=1, trained_like=True)
    batches = [_batch(model, s) for s in range(4)]
    ref = _run(model, params, "prepared", batches)
    _assert_same(ref, _run(model, params, "prepared", batches), "prepared twice")     # the yardstick is deterministic
    assert np.isfinite(ref["steps"][-1][0])
    _assert_same(ref, _run(model, params, "u8", batches), "uint8 raw")
    _assert_same(ref, _run(model, params, "f32", batches), "float32 raw")


def test_raw_input_of_the_wrong_size_is_rejected():
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    model = "mutopia_ccal_cont"
    eng = _lib.Engine(model)
    try:
        eng.set_params(synth_data.synth_params(param_shapes(model), seed=1, trained_like=True))
        eng.train_begin(4)
        u8, _, spec = _batch(model, 0)
        with pytest.raises(ValueError):
            eng.train_step(u8[:4, :, :80], spec[:4], 0.002, prepared=False)
        with pytest.raises(_lib.AsrError):                       # an unknown input mode
            eng._check(eng.lib.asr_train_step_in(eng.ctx, u8.ctypes.data, 7, spec.ctypes.data, 4, 0.002, None, None))
    finally:
        eng.close()


def _fake_pieces(rng, n_pieces=3):
    images, specs, maps = [], [], []
    for p in range(n_pieces):
        W = int(rng.integers(1500, 2600))
        img = (rng.random((200, W)) * 255).astype(np.float32)
        T = int(rng.integers(500, 900))
        sp = [(3 * rng.random((92, T)) ** 2).astype(np.float32) for _ in range(1 + p % 2)]
        onsets = np.sort(rng.choice(np.arange(30, T - 30), size=40, replace=False))
        coords = np.linspace(450, W - 450, 40).astype(np.int64)
        images.append(img)
        specs.append(sp)
        maps.append([np.stack([onsets, coords], axis=1).astype(np.int64) for _ in sp])
    return images, specs, maps


def _train_one_subepoch(device_feed):
    """train() for one sub-epoch of 3 updates at batch 32 on an AudioScoreRetrievalPool with augmentation: with the
    model's prepare (-> batches assembled on the device) or a wrapper of it (-> the host-prepared pool[key] batches)"""
    from audio_sheet_retrieval_amd import _lib, network
    from audio_sheet_retrieval_amd.models import _common, mutopia_ccal_cont as m
    from audio_sheet_retrieval_amd.utils import synth_data, train_dcca_pool as tdp
    from audio_sheet_retrieval_amd.utils.batch_iterators import MultiviewPoolIteratorUnsupervised
    from audio_sheet_retrieval_amd.utils.data_pools import AudioScoreRetrievalPool
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    layers = m.build_model()
    net = layers[0].net
    network.set_all_param_values(layers, synth_data.synth_params(param_shapes(m.__name__.split(".")[-1]), seed=3,
                                                                 trained_like=True))
    np.random.seed(17)
    images, specs, maps = _fake_pieces(np.random.default_rng(4))
    aug = dict(system_translation=3, sheet_scaling=[0.95, 1.05], onset_translation=1, spec_padding=0, interpolate=-1)
    # the host route's pool lives on a context of its own: pool[key] runs on the batch producer thread
    pool_eng = net.engine if device_feed else _lib.Engine("mutopia_ccal_cont")
    pool = AudioScoreRetrievalPool(pool_eng, images, specs, maps, data_augmentation=aug, shuffle=True)
    data = dict(train=pool, valid=synth_data.SyntheticRetrievalPool(64, seed=9))
    prepare = _common.prepare_plain if device_feed else (lambda x, z: _common.prepare_plain(x, z))
    funcs = tdp.create_iter_functions(layers, m.objectives, m.compute_updates, 0.002, m.L2, None)
    before = dict(tdp.ROUTE_CALLS)
    it = MultiviewPoolIteratorUnsupervised(batch_size=B, prepare=prepare, k_samples=96)
    va = MultiviewPoolIteratorUnsupervised(batch_size=32, prepare=prepare, shuffle=False)
    epoch = next(tdp.train(funcs, data, it, va, fit_cca=False))
    calls = {k: tdp.ROUTE_CALLS[k] - before.get(k, 0) for k in tdp.ROUTE_CALLS}
    funcs.close()
    params = network.get_all_param_values(layers)
    rng_state = np.random.get_state()[1].copy()
    net.engine.close()
    if pool_eng is not net.engine:
        pool_eng.close()
    return params, epoch, calls, rng_state


def test_device_pool_feeds_train_like_the_downloaded_batches():
    p_dev, e_dev, c_dev, rng_dev = _train_one_subepoch(True)
    p_host, e_host, c_host, rng_host = _train_one_subepoch(False)
    assert c_dev.get("device") == 3 and not c_dev.get("prepared")
    assert c_host.get("prepared") == 3 and not c_host.get("device") and not c_host.get("raw")
    assert np.array_equal(rng_dev, rng_host)                   # the same augmentation draws, in the same order
    assert all(np.array_equal(a, b) for a, b in zip(p_dev, p_host))
    assert e_dev["train_loss"] == e_host["train_loss"] and e_dev["map_va"] == e_host["map_va"]


def test_run_train_synthetic_takes_the_raw_route(tmp_path, monkeypatch):
    """one epoch of run_train.py --data synthetic: the model's prepare -> every update, validation loss and
    embedding goes through the raw entry points; equal to the same run on host-prepared batches"""
    import audio_sheet_retrieval_amd.models.mutopia_ccal_cont as m
    import audio_sheet_retrieval_amd.run_train as rt
    import audio_sheet_retrieval_amd.utils.batch_iterators as bi
    from audio_sheet_retrieval_amd.utils import train_dcca_pool as tdp
    monkeypatch.setattr(rt, "EXP_ROOT", str(tmp_path))
    common = ["--model", "models/mutopia_ccal_cont.py", "--data", "synthetic:300:100:100", "--max_epochs", "1",
              "--train_split", "splits/all_split.yaml", "--config", "exp_configs/mutopia_full_aug.yaml"]
    out = {}
    for route, prepare in (("raw", m.prepare), ("prepared", lambda x, z: m.prepare(x, z))):
        monkeypatch.setattr(m, "train_batch_iterator", lambda batch_size=m.BATCH_SIZE, p=prepare:
                            bi.MultiviewPoolIteratorUnsupervised(batch_size=batch_size, prepare=p, k_samples=300))
        monkeypatch.setattr(m, "valid_batch_iterator", lambda p=prepare:
                            bi.MultiviewPoolIteratorUnsupervised(batch_size=m.BATCH_SIZE, prepare=p, shuffle=False))
        before = dict(tdp.ROUTE_CALLS)
        np.random.seed(7)                                         # the initial weights
        rt.main(common)
        out[route] = (pickle.load(open(tmp_path / "mutopia_ccal_cont" / "params_all_split_mutopia_full_aug.pkl", "rb")),
                      pickle.load(open(tmp_path / "mutopia_ccal_cont" / "results_all_split_mutopia_full_aug.pkl", "rb")),
                      {k: tdp.ROUTE_CALLS[k] - before.get(k, 0) for k in tdp.ROUTE_CALLS})
    calls_raw, calls_prep = out["raw"][2], out["prepared"][2]
    assert calls_raw.get("raw") == 3 + 1 and not calls_raw.get("prepared")       # 3 updates + 1 validation batch
    assert calls_prep.get("prepared") == 3 and not calls_prep.get("raw")
    assert all(np.array_equal(a, b) for a, b in zip(out["raw"][0], out["prepared"][0]))
    for key in ("pred_tr_err", "pred_val_err", "map_val"):
        assert np.array_equal(out["raw"][1][key], out["prepared"][1][key]), key
