"""Probe (GPU box): what train()'s own loop (utils/train_dcca_pool.py) achieves in updates per second over one
k_samples = 10 000 sub-epoch, per feed, against the resident-input step (asr_train_step_dev) as the ceiling.

Feeds (one process, one context per run, the same batches):
  f32_prepared  host float32 prepared by the iterator (prepare wrapped, so the library is not told it is its own)
  u8_raw        the iterator's raw view: uint8 sheets, model.prepare on the device (asr_train_step_in)
  device_pool   AudioScoreRetrievalPool: batches assembled on the device (get_device + asr_train_step_in_dev)
Timing: one warm-up sub-epoch per feed (tuner, allocations), then `repeats` timed sub-epochs; a sub-epoch's time runs
from the start of train()'s generator to the return of its last update (every host entry point returns after the
device has finished).  Prints one JSON line.
    python tools/bench_fit.py [--batches 100,512] [--k-samples 10000] [--repeats 3]

--eval: the epoch's evaluation instead - the train-metric pass over the sub-epoch (n_valid_cca = 1000 rows embedded)
plus the validation pass over a pool of --n-valid pairs, both at the models' BATCH_SIZE (100), fit_cca off.  Its time
runs from the return of the epoch's last update to the return of train()'s yield.  Feeds:
  two_calls         the u8_raw feed with iter_funcs['valid'] wrapped in a lambda: the reference's two calls per batch
  two_calls_f32     the same on the f32_prepared feed;  two_calls_device  on the device_pool feed
  f32_prepared      one call per batch (asr_valid_output_in) on host float32 prepared batches
  u8_raw            one call per batch on the raw uint8 batches
  device_pool       AudioScoreRetrievalPool on the engine: get_device + asr_valid_output_in_dev, one download per pass
    python tools/bench_fit.py --eval [--k-samples 10000] [--n-valid 10000] [--repeats 2]"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL = "mutopia_ccal_cont"


def _device_pool_pieces(n_samples, seed=4):
    """strips with n_samples usable (piece, onset) entities: 10 pieces, one performance each"""
    rng = np.random.default_rng(seed)
    per = -(-n_samples // 10) + 2
    images, specs, maps = [], [], []
    for _ in range(10):
        W = 40 * per + 1000
        images.append((rng.random((200, W)) * 255).astype(np.float32))
        T = 4 * per + 200
        specs.append([(3 * rng.random((92, T)) ** 2).astype(np.float32)])
        onsets = 60 + 4 * np.arange(per)
        coords = 500 + 40 * np.arange(per)
        maps.append([np.stack([onsets, coords], axis=1).astype(np.int64)])
    return images, specs, maps


def _timed_updates(funcs):
    """wrap the instance's step callables: record the host time every update returns"""
    stamps = []

    def wrap(f):
        def g(*a):
            r = f(*a)
            stamps.append(time.perf_counter())
            return r
        return g
    funcs["train"] = wrap(funcs["train"])
    funcs.train_raw = wrap(funcs.train_raw)
    funcs.train_dev = wrap(funcs.train_dev)
    return stamps


def run_feed(feed, B, k_samples, repeats, pieces):
    from audio_sheet_retrieval_amd import network
    from audio_sheet_retrieval_amd.models import _common, mutopia_ccal_cont as m
    from audio_sheet_retrieval_amd.utils import synth_data, train_dcca_pool as tdp
    from audio_sheet_retrieval_amd.utils.batch_iterators import MultiviewPoolIteratorUnsupervised
    from audio_sheet_retrieval_amd.utils.data_pools import AudioScoreRetrievalPool
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    layers = m.build_model()
    eng = layers[0].net.engine
    network.set_all_param_values(layers, synth_data.synth_params(param_shapes(MODEL), seed=1, trained_like=False))
    np.random.seed(17)
    if feed == "device_pool":
        train_pool = AudioScoreRetrievalPool(eng, *pieces, shuffle=True)
    else:
        train_pool = synth_data.SyntheticRetrievalPool(k_samples, seed=23, shuffle=True)
    data = dict(train=train_pool, valid=synth_data.SyntheticRetrievalPool(100, seed=9, first_index=10 ** 6))
    prepare = (lambda x, z: _common.prepare_plain(x, z)) if feed == "f32_prepared" else _common.prepare_plain
    funcs = tdp.create_iter_functions(layers, m.objectives, m.compute_updates, m.INI_LEARNING_RATE, m.L2, None)
    stamps = _timed_updates(funcs)
    it = MultiviewPoolIteratorUnsupervised(batch_size=B, prepare=prepare, k_samples=k_samples)
    va = MultiviewPoolIteratorUnsupervised(batch_size=100, prepare=prepare, shuffle=False)
    before = dict(tdp.ROUTE_CALLS)
    epochs = tdp.train(funcs, data, it, va, fit_cca=False)
    times = []
    for rep in range(repeats + 1):
        del stamps[:]
        t0 = time.perf_counter()
        next(epochs)
        if rep:                                                   # (the first sub-epoch is the warm-up)
            times.append((stamps[-1] - t0) / len(stamps))
    n_updates = len(stamps)
    routes = {k: tdp.ROUTE_CALLS[k] - before.get(k, 0) for k in tdp.ROUTE_CALLS if tdp.ROUTE_CALLS[k] > before.get(k, 0)}
    epochs.close()
    funcs.close()
    eng.close()
    ms = np.array(times) * 1e3
    return dict(ms_per_update=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()),
                ups=float(1e3 / np.median(ms)), updates_per_subepoch=n_updates, routes=routes)


def run_eval_feed(feed, k_samples, n_valid, repeats, pieces, B=100):
    """one context per feed: warm-up epoch, then `repeats` epochs; per epoch the seconds from the last update's return
    to the epoch's yield (the train-metric and validation passes + the retrieval ranks of both)"""
    from audio_sheet_retrieval_amd import network
    from audio_sheet_retrieval_amd.models import _common, mutopia_ccal_cont as m
    from audio_sheet_retrieval_amd.utils import synth_data, train_dcca_pool as tdp
    from audio_sheet_retrieval_amd.utils.batch_iterators import MultiviewPoolIteratorUnsupervised
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    layers = m.build_model()
    eng = layers[0].net.engine
    network.set_all_param_values(layers, synth_data.synth_params(param_shapes(MODEL), seed=1, trained_like=False))
    np.random.seed(17)
    base = {"two_calls": "u8_raw", "two_calls_f32": "f32_prepared", "two_calls_device": "device_pool"}.get(feed, feed)
    if base == "device_pool":
        train_pool = AudioScoreRetrievalPool(eng, *pieces, shuffle=True)
        valid_pool = AudioScoreRetrievalPool(eng, *pieces, data_augmentation=dict(NO_AUGMENT), shuffle=False)
        valid_pool.train_entities = valid_pool.train_entities[:n_valid]        # the synthetic feeds' pool size
        valid_pool.shape = [valid_pool.train_entities.shape[0]]
    else:
        train_pool = synth_data.SyntheticRetrievalPool(k_samples, seed=23, shuffle=True)
        valid_pool = synth_data.SyntheticRetrievalPool(n_valid, seed=9, first_index=10 ** 6)
    n_valid = valid_pool.shape[0]
    data = dict(train=train_pool, valid=valid_pool)
    prepare = (lambda x, z: _common.prepare_plain(x, z)) if base == "f32_prepared" else _common.prepare_plain
    funcs = tdp.create_iter_functions(layers, m.objectives, m.compute_updates, m.INI_LEARNING_RATE, m.L2, None)
    if feed.startswith("two_calls"):
        inner = funcs["valid"]
        funcs["valid"] = lambda X1, X2: inner(X1, X2)
    stamps = _timed_updates(funcs)
    it = MultiviewPoolIteratorUnsupervised(batch_size=B, prepare=prepare, k_samples=k_samples)
    va = MultiviewPoolIteratorUnsupervised(batch_size=B, prepare=prepare, shuffle=False)
    epochs = tdp.train(funcs, data, it, va, fit_cca=False)
    times, before = [], None
    for rep in range(repeats + 1):
        if rep == 1:
            before = dict(tdp.ROUTE_CALLS)
        next(epochs)
        t1 = time.perf_counter()
        if rep:                                                   # (the first epoch is the warm-up)
            times.append(t1 - stamps[-1])
    routes = {k: (tdp.ROUTE_CALLS[k] - before.get(k, 0)) // repeats for k in tdp.ROUTE_CALLS
              if tdp.ROUTE_CALLS[k] > before.get(k, 0)}
    epochs.close()
    funcs.close()
    eng.close()
    s = np.array(times)
    pairs = -(-k_samples // B) * B + -(-n_valid // B) * B
    return dict(s_per_eval=float(np.median(s)), s_min=float(s.min()), s_max=float(s.max()),
                pairs_per_s=float(pairs / np.median(s)), pairs_walked=pairs, n_valid=n_valid, routes_per_epoch=routes)


def main_eval(args):
    pieces = _device_pool_pieces(max(args.k_samples, args.n_valid)) if "device" in args.feeds else None
    out = dict(tool="bench_fit", leg="eval", model=MODEL, batch=100, k_samples=args.k_samples, n_valid=args.n_valid,
               n_valid_cca=1000, repeats=args.repeats, results={})
    for feed in args.feeds.split(","):
        with contextlib.redirect_stdout(sys.stderr):             # train()'s progress lines
            r = run_eval_feed(feed, args.k_samples, args.n_valid, args.repeats, pieces)
        out["results"][feed] = r
        print("eval %-16s %.3f s (%.3f-%.3f), %.0f pairs/s, routes %s" % (
            feed, r["s_per_eval"], r["s_min"], r["s_max"], r["pairs_per_s"], r["routes_per_epoch"]),
            file=sys.stderr, flush=True)
    print(json.dumps(out))


def ceiling(B, repeats, steps=20):
    """asr_train_step_dev on prepared inputs resident in HBM, the step bench.py's training leg times"""
    from ctypes import byref, c_float
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.models import _common
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    eng = _lib.Engine(MODEL)
    eng.set_params(synth_data.synth_params(param_shapes(MODEL), seed=1, trained_like=False))
    sheet, spec = synth_data.synth_pairs(np.arange(B), seed=23)
    x1 = _common.prepare_plain(sheet)
    d1, d2 = eng.alloc(x1.nbytes).upload(x1), eng.alloc(spec.nbytes).upload(spec)
    eng.train_begin(B)
    loss, corr = c_float(), np.empty(32, np.float32)

    def step():
        eng._check(eng.lib.asr_train_step_dev(eng.ctx, d1.ptr, d2.ptr, B, 1e-4, byref(loss), corr.ctypes.data))
    for _ in range(3):
        step()
    eng.sync()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        eng.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    eng.train_end()
    d1.free()
    d2.free()
    eng.close()
    ms = np.array(ms)
    return dict(ms_per_update=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()),
                ups=float(1e3 / np.median(ms)))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="100,512")
    p.add_argument("--k-samples", type=int, default=10000)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--feeds", default=None)
    p.add_argument("--eval", action="store_true", help="time the epoch's evaluation passes instead of the updates")
    p.add_argument("--n-valid", type=int, default=10000)
    args = p.parse_args(argv)
    if args.eval:
        if args.feeds is None:
            args.feeds = "two_calls_f32,f32_prepared,two_calls,u8_raw,two_calls_device,device_pool"
        return main_eval(args)
    if args.feeds is None:
        args.feeds = "f32_prepared,u8_raw,device_pool"
    pieces = _device_pool_pieces(args.k_samples) if "device_pool" in args.feeds else None
    out = dict(tool="bench_fit", model=MODEL, k_samples=args.k_samples, repeats=args.repeats, results={})
    for B in [int(b) for b in args.batches.split(",")]:
        res = dict(ceiling=ceiling(B, args.repeats))
        for feed in args.feeds.split(","):
            with contextlib.redirect_stdout(sys.stderr):         # train()'s progress lines
                r = run_feed(feed, B, args.k_samples, args.repeats, pieces)
            r["ratio_to_ceiling"] = res["ceiling"]["ms_per_update"] / r["ms_per_update"]
            res[feed] = r
            print("batch %d %-13s %.3f ms/update (%.3f-%.3f), %.1f ups, %.3f of the ceiling" % (
                B, feed, r["ms_per_update"], r["ms_min"], r["ms_max"], r["ups"], r["ratio_to_ceiling"]),
                file=sys.stderr, flush=True)
        out["results"][str(B)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
