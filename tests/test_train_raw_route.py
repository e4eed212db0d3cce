"""CPU: the raw training route (include/asr_hip.h asr_*_in): the new entry points are declared, bound and exported;
the batch iterator's raw view yields the prepared view's batches before model.prepare (same order, fill-up,
reshuffle); IterFunctions sizes the context from a raw batch at its own size."""
import ctypes
import os
import re

import numpy as np
import pytest

NEW_SYMBOLS = ["asr_train_step_in", "asr_train_step_in_dev", "asr_burn_in_in", "asr_compute_gradients_in",
               "asr_valid_loss_in"]


def test_raw_training_symbols_declared_bound_and_exported(repo_root):
    from audio_sheet_retrieval_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", "asr_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.EXPORTS, name
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libasr_hip.so does not export %s" % name


def _passes(prepare, n_pool, batch, k_samples, passes, view):
    from audio_sheet_retrieval_amd.utils.batch_iterators import MultiviewPoolIteratorUnsupervised
    from audio_sheet_retrieval_amd.utils.synth_data import SyntheticRetrievalPool
    pool = SyntheticRetrievalPool(n_pool, seed=5, shuffle=True)
    it = MultiviewPoolIteratorUnsupervised(batch_size=batch, prepare=prepare, k_samples=k_samples)
    out = []
    for _ in range(passes):
        it(pool)
        out.append(list(getattr(it, view)() if view else it))
    return out, pool


@pytest.mark.parametrize("prep_name", ["prepare_plain", "prepare_rsz"])
@pytest.mark.parametrize("k_samples", [None, 22])
def test_raw_view_is_the_prepared_view_before_prepare(prep_name, k_samples):
    """shuffle on, two passes, batch 8 of a 45-pair pool: k_samples None -> a short last batch filled up from the
    pool's start and a reshuffle after every pass; 22 -> two windows, the second one filled up, then a reshuffle"""
    from audio_sheet_retrieval_amd.models import _common
    prepare = getattr(_common, prep_name)
    prepared, pool_p = _passes(prepare, 45, 8, k_samples, 2, None)
    raw, pool_r = _passes(prepare, 45, 8, k_samples, 2, "raw")
    keys, _ = _passes(prepare, 45, 8, k_samples, 2, "keys")
    assert [len(p) for p in prepared] == [len(p) for p in raw] == [len(p) for p in keys]
    assert np.array_equal(pool_p.train_entities, pool_r.train_entities)
    saw_fill = False
    for epoch in range(2):
        for (xp, zp), (xr, zr) in zip(prepared[epoch], raw[epoch]):
            assert xr.dtype == np.uint8 and xr.shape[2:] == (160, 200)
            assert np.array_equal(prepare(xr), xp) and prepare(xr).dtype == xp.dtype == np.float32
            assert np.array_equal(zr, zp)
    # the key view names the same rows (checked on a pool in the same shuffle state)
    from audio_sheet_retrieval_amd.utils.synth_data import SyntheticRetrievalPool
    ref = SyntheticRetrievalPool(45, seed=5, shuffle=True)
    for epoch in range(2):
        if epoch and k_samples is None:
            ref.reset_batch_generator()
        for (xr, zr), idx in zip(raw[epoch], keys[epoch]):
            x, z = ref.get_u8(idx)
            assert np.array_equal(x, xr) and np.array_equal(z, zr)
            saw_fill |= bool(idx[-1] < idx[0])
    assert saw_fill
    # both views reshuffled the pool the same number of times
    assert not np.array_equal(pool_r.train_entities, np.arange(45)) and pool_r._epoch == pool_p._epoch >= 2


class _Cfg(object):
    h1, w1, h2, w2 = 120, 200, 92, 42


class _FakeEngine(object):
    """records what IterFunctions asks of the library"""

    def __init__(self, rsz):
        self.cfg, self.rsz, self.calls = _Cfg(), rsz, []
        self.net_h1, self.net_w1 = (60, 100) if rsz else (120, 200)

    def set_input_size(self, view, h, w):
        self.calls.append(("set_input_size", view, h, w))
        if view == 1:
            self.cfg.h1, self.cfg.w1 = h, w
            self.net_h1, self.net_w1 = (h // 2, w // 2) if self.rsz else (h, w)
        else:
            self.cfg.h2, self.cfg.w2 = h, w

    def comm_info(self):
        return 0, 1

    def train_begin(self, n):
        self.calls.append(("train_begin", n))

    def train_step(self, x1, x2, lr, prepared=True):
        self.calls.append(("train_step", x1.shape, prepared))
        return 1.0, np.zeros(32, np.float32)


class _Net(object):
    def __init__(self, name, engine):
        self.model_name, self.engine = name, engine


class _Layer(object):
    def __init__(self, net):
        self.net = net


@pytest.mark.parametrize("model", ["mutopia_ccal_cont", "mutopia_ccal_cont_rsz"])
def test_raw_batch_sets_the_raw_size_itself(model):
    from audio_sheet_retrieval_amd.utils.train_dcca_pool import IterFunctions, SharedScalar
    eng = _FakeEngine(model.endswith("_rsz"))
    funcs = IterFunctions([_Layer(_Net(model, eng))], SharedScalar(0.002))
    x1 = np.zeros((4, 1, 160, 200), np.uint8)
    x2 = np.zeros((4, 1, 92, 42), np.float32)
    funcs.train_raw(x1, x2)
    assert ("set_input_size", 1, 160, 200) in eng.calls           # not 320 x 400 for the rsz model
    assert (eng.cfg.h1, eng.cfg.w1) == (160, 200)
    assert eng.calls[-1] == ("train_step", (4, 1, 160, 200), False)
    n_sets = sum(c[0] == "set_input_size" for c in eng.calls)
    funcs.train_raw(x1, x2)                                        # same size: nothing re-sized
    assert sum(c[0] == "set_input_size" for c in eng.calls) == n_sets
