"""GPU: one-pass validation (asr_valid_output_in / _in_dev): the loss of valid_loss and the latents of embed_both from
one forward, bit for bit, on every input route and objective; the device entry point queued over pool batches that reuse
the same window buffers; no training state moves; train()'s evaluation passes on a device pool give the host route's
epoch, and a replaced iter_funcs['valid'] still gets the reference's two calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 32


@pytest.fixture(autouse=True)
def _model_schedules(monkeypatch):
    """the model's schedule picks in every context: timed picks may differ between two contexts, and with them the
    float32 summation order - the comparisons below are bit for bit"""
    monkeypatch.setenv("ASR_AUTOTUNE", "0")


def _params(model, seed=1):
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    return synth_data.synth_params(param_shapes(model), seed=seed, trained_like=True)


def _batch(model, seed):
    from audio_sheet_retrieval_amd.models import _common
    from audio_sheet_retrieval_amd.utils import synth_data
    sheet_u8, spec = synth_data.synth_pairs(np.arange(seed * B, (seed + 1) * B), seed=23)
    prepare = _common.prepare_rsz if model.endswith("_rsz") else _common.prepare_plain
    return {"prepared": prepare(sheet_u8), "u8": sheet_u8, "f32": sheet_u8.astype(np.float32)}, spec


def _contrastive_loss(lv1, lv2, weight=1.0, gamma=0.7, symmetric=False):
    """get_contrastive_cos_loss (models/objectives.py:30-69) in float64 on the latents"""
    total = 0.0
    for a, b in ((lv1, lv2), (lv2, lv1))[:2 if symmetric else 1]:
        d = a.astype(np.float64) @ b.astype(np.float64).T
        L = np.clip(gamma - np.diag(d)[:, None] + d, 0.0, 1000.0)
        np.fill_diagonal(L, 0.0)
        total += L.sum()
    n = lv1.shape[0]
    return weight * total / (n * (n - 1.0))


@pytest.mark.parametrize("model", ["mutopia_ccal_cont", "mutopia_ccal_cont_rsz"])
def test_valid_output_equals_valid_loss_and_embed_both(model):
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine(model)
    try:
        eng.set_params(_params(model))
        x1s, spec = _batch(model, 0)
        u8_loss = {}
        for objective in (None, (0.5, 0.7, True), (2.0, 0.7, False)):
            if objective:
                eng.set_objective(*objective)
            for route, x1 in x1s.items():
                prepared = route == "prepared"
                want_loss = eng.valid_loss(x1, spec, prepared=prepared)
                want1, want2 = eng.embed_both(x1, spec, prepared=prepared)
                loss, lv1, lv2 = eng.valid_output(x1, spec, prepared=prepared)
                what = "%s %s %r" % (model, route, objective)
                assert np.isfinite(loss) and loss > 0, what
                assert loss == want_loss, what
                assert np.array_equal(lv1, want1) and np.array_equal(lv2, want2), what
                kw = dict(weight=objective[0], gamma=objective[1], symmetric=objective[2]) if objective else {}
                assert abs(loss - _contrastive_loss(lv1, lv2, **kw)) <= 1e-5 * max(1.0, loss), what
                if route == "u8":
                    u8_loss[objective] = loss
        assert u8_loss[(2.0, 0.7, False)] == 2 * u8_loss[None]        # the objective reached the call
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


def test_device_entry_point_queues_batches_through_reused_windows():
    """4 batches gathered into the SAME two window buffers and queued without a host synchronisation between them
    (the last one without latent buffers); one download; every batch equals the host route on its windows"""
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    model = "mutopia_ccal_cont"
    eng = _lib.Engine(model)
    try:
        eng.set_params(_params(model))
        eng.set_objective(1.0, 0.7, True)
        pool = AudioScoreRetrievalPool(eng, *_fake_pieces(np.random.default_rng(4)), data_augmentation=NO_AUGMENT,
                                       shuffle=False)
        eng.set_input_size(1, *pool.sheet_dim)
        eng.set_input_size(2, *pool.spec_dim)
        keys = [np.arange(k * B, (k + 1) * B) for k in range(3)] + [np.arange(7, 7 + B)]
        bufs = (eng.alloc(B * int(np.prod(pool.sheet_dim)) * 4), eng.alloc(B * int(np.prod(pool.spec_dim)) * 4))
        rows = 3 * B
        ws = eng.alloc(4 * (2 * rows * 32 + len(keys)))
        for k, idx in enumerate(keys):
            b1, b2, n = pool.get_device(idx, out=bufs)
            lv = (ws.offset(4 * k * B * 32), ws.offset(4 * (rows + k * B) * 32)) if k < 3 else (None, None)
            eng.valid_output_dev(b1.ptr, _lib.IN_F32_RAW, b2.ptr, n, ws.offset(4 * (2 * rows * 32 + k)), *lv)
        out = ws.download((2 * rows * 32 + len(keys),), np.float32)
        for b in (ws,) + bufs:
            b.free()
        lv1, lv2, losses = out[:rows * 32].reshape(rows, 32), out[rows * 32:2 * rows * 32].reshape(rows, 32), out[-4:]
        for k, idx in enumerate(keys):
            x1, x2 = pool[idx]                                  # no augmentation: the same windows again
            loss, want1, want2 = eng.valid_output(x1, x2, prepared=False)
            assert losses[k] == np.float32(loss), k
            assert loss == eng.valid_loss(x1, x2, prepared=False), k
            if k < 3:
                assert np.array_equal(lv1[k * B:(k + 1) * B], want1), k
                assert np.array_equal(lv2[k * B:(k + 1) * B], want2), k
        assert len(set(losses.tolist())) == 4
    finally:
        eng.close()


def _updates(with_valid):
    """fresh context, 3 updates (valid_output on the host and on device buffers after each when asked), then a 4th"""
    from audio_sheet_retrieval_amd import _lib
    model = "mutopia_ccal_cont"
    eng = _lib.Engine(model)
    try:
        eng.set_params(_params(model, seed=2))
        batches = [_batch(model, s) for s in range(5)]
        eng.set_input_size(1, 160, 200)
        eng.train_begin(B)
        x1v, specv = batches[4][0]["u8"], batches[4][1]
        d1 = eng.alloc(B * 160 * 200 * 4).upload(batches[4][0]["f32"])
        d2 = eng.alloc(specv.nbytes).upload(specv)
        dl = eng.alloc(4 * (1 + 2 * B * 32))
        seen = []
        for x1s, spec in batches[:3]:
            eng.train_step(x1s["u8"], spec, 0.002, prepared=False)
            if with_valid:
                seen.append(eng.valid_output(x1v, specv, prepared=False))
                eng.valid_output_dev(d1.ptr, _lib.IN_F32_RAW, d2.ptr, B, dl.offset(256 * B), dl.ptr, dl.offset(128 * B))
                dev = dl.download((2 * B * 32 + 1,), np.float32)
                assert dev[-1] == np.float32(seen[-1][0])
                assert np.array_equal(dev[:-1].reshape(2, B, 32)[0], seen[-1][1])
                assert np.array_equal(dev[:-1].reshape(2, B, 32)[1], seen[-1][2])
        params, opt = eng.get_params(), eng.get_opt_state()
        x1s, spec = batches[3]
        loss4 = eng.train_step(x1s["u8"], spec, 0.002, prepared=False)
        for b in (d1, d2, dl):
            b.free()
        eng.train_end()
        after_end = (eng.valid_loss(x1v, specv, prepared=False), eng.valid_output(x1v, specv, prepared=False))
        return params, opt, loss4, seen, after_end
    finally:
        eng.close()


def test_valid_output_moves_no_training_state():
    p_a, o_a, l_a, seen, end_a = _updates(True)
    p_b, o_b, l_b, _, end_b = _updates(False)
    assert len(seen) == 3 and seen[0][0] != seen[2][0]          # the updates changed what the validation saw
    assert all(np.array_equal(a, b) for a, b in zip(p_a, p_b))  # BatchNorm mean / inv_std, CCALayer U V means S*
    assert np.array_equal(o_a["m"], o_b["m"]) and np.array_equal(o_a["v"], o_b["v"]) and o_a["t"] == o_b["t"] == 3
    assert l_a[0] == l_b[0] and np.array_equal(l_a[1], l_b[1])
    # after train_end, as without a training state: the loss of valid_loss
    assert end_a[0] == end_a[1][0] == end_b[0] == end_b[1][0]


def _train_one_subepoch(device_feed, replace_valid=False):
    """train() for one sub-epoch of 3 updates at batch 32: an augmenting AudioScoreRetrievalPool for training and a
    NO_AUGMENT, unshuffled one (40 pairs) for validation.  The model's prepare -> both evaluation passes on the device
    route; a wrapper of it -> host-prepared batches from pools on a second context"""
    from audio_sheet_retrieval_amd import _lib, network
    from audio_sheet_retrieval_amd.models import _common, mutopia_ccal_cont as m
    from audio_sheet_retrieval_amd.utils import synth_data, train_dcca_pool as tdp
    from audio_sheet_retrieval_amd.utils.batch_iterators import MultiviewPoolIteratorUnsupervised
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    layers = m.build_model()
    net = layers[0].net
    network.set_all_param_values(layers, synth_data.synth_params(param_shapes("mutopia_ccal_cont"), seed=3,
                                                                 trained_like=True))
    np.random.seed(17)
    rng = np.random.default_rng(4)
    images, specs, maps = _fake_pieces(rng)
    aug = dict(system_translation=3, sheet_scaling=[0.95, 1.05], onset_translation=1, spec_padding=0, interpolate=-1)
    pool_eng = net.engine if device_feed else _lib.Engine("mutopia_ccal_cont")
    pool = AudioScoreRetrievalPool(pool_eng, images, specs, maps, data_augmentation=aug, shuffle=True)
    valid = AudioScoreRetrievalPool(pool_eng, *_fake_pieces(rng, n_pieces=1), data_augmentation=NO_AUGMENT,
                                    shuffle=False)
    data = dict(train=pool, valid=valid)
    prepare = _common.prepare_plain if device_feed else (lambda x, z: _common.prepare_plain(x, z))
    funcs = tdp.create_iter_functions(layers, m.objectives, m.compute_updates, 0.002, m.L2, None)
    wrapped = []
    if replace_valid:
        inner = funcs["valid"]
        funcs["valid"] = lambda X1, X2: wrapped.append(1) or inner(X1, X2)
    before = dict(tdp.ROUTE_CALLS)
    it = MultiviewPoolIteratorUnsupervised(batch_size=B, prepare=prepare, k_samples=96)
    va = MultiviewPoolIteratorUnsupervised(batch_size=B, prepare=prepare, shuffle=False)
    epoch = next(tdp.train(funcs, data, it, va, fit_cca=True))
    calls = {k: tdp.ROUTE_CALLS[k] - before.get(k, 0) for k in tdp.ROUTE_CALLS}
    calls["wrapped_valid"] = len(wrapped)
    funcs.close()
    params = network.get_all_param_values(layers)
    rng_state = np.random.get_state()[1].copy()
    net.engine.close()
    if pool_eng is not net.engine:
        pool_eng.close()
    return params, epoch, calls, rng_state, valid.shape[0]


def _assert_same_epoch(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        if a[key] is None or b[key] is None:
            assert a[key] is b[key], key
        elif isinstance(a[key], dict):
            assert a[key] == b[key], key
        else:
            assert np.array_equal(a[key], b[key]), (key, a[key], b[key])


def test_train_evaluates_a_device_pool_like_the_host_route():
    p_dev, e_dev, c_dev, rng_dev, n_valid = _train_one_subepoch(True)
    p_host, e_host, c_host, rng_host, _ = _train_one_subepoch(False)
    assert n_valid == 40                                         # n_valid_cca = 40: 2 of the 3 train batches embedded
    assert c_dev.get("device") == 3 and not c_dev.get("prepared")
    assert c_dev.get("eval_device") == 2 and c_dev.get("valid_device") == 2 and not c_dev.get("raw")
    assert c_host.get("prepared") == 3 and not c_host.get("raw")
    assert not c_host.get("device") and not c_host.get("eval_device") and not c_host.get("valid_device")
    assert np.array_equal(rng_dev, rng_host)        # the skipped train batch still drew its augmentation numbers
    assert all(np.array_equal(a, b) for a, b in zip(p_dev, p_host))
    _assert_same_epoch(e_dev, e_host)
    assert np.isfinite(e_dev["valid_loss"]) and e_dev["valid_loss"] > 0

    # the reference's composition: iter_funcs['valid'] replaced -> two calls per validation batch, the same epoch
    p_two, e_two, c_two, rng_two, _ = _train_one_subepoch(False, replace_valid=True)
    assert c_two["wrapped_valid"] == 2 and not c_two.get("valid_device")
    assert np.array_equal(rng_two, rng_host) and all(np.array_equal(a, b) for a, b in zip(p_two, p_host))
    _assert_same_epoch(e_two, e_host)
