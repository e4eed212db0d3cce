"""GPU: everything of the training step that is NOT a 3x3 convolution, each tower against float64 at ragged shapes.

The 3x3 convolutions have tests/test_gpu_train_candidates.py.  The rest of the step - conv1_raw_kernel (modes 0, 1, 2),
prepare_view1_kernel, bn_stats_* / colsum_*, bn_apply_elu_pool_kernel / pool_mask_kernel, bn_bwd_reduce_kernel<POOL> /
bn_bwd_final_kernel / bn_bwd_apply_kernel, bn_bwd_reduce_conv1_kernel, conv1_wgrad_kernel and its reduce,
conv1x1_raw_kernel, bn_gpool_kernel and the tail_bwd_* chain - reached the oracle only through whole-step gradients at
two even geometries whose pixel counts are multiples of 64.  Here:

Backward.  compute_gradients, then the device's own dH of each tower (asr_debug_train_tensor) and its pooling selection
go into oracle.train.tower_forward_train / tower_backward in float64; the 27 gradient tensors of each tower (L2 term
added, as compute_gradients reports them) are compared.  The CCALayer stage is an input, not part of the comparison
(its gradient divides by eigenvalue differences; batches near the rank limit eat the bar), but dH must be finite, the
loss within 2e-5 of oracle.train.loss_and_grads with the selection imposed, and the imposed selection the maximum up
to rounding (route_check gap <= ROUTE_GAP_BAR).

Forward, block by block, each from the device's own input (after burn_in: the backward pass overwrites block 9's z):
z_b against the float64 convolution of the device's x_b; stats_b against the float64 mean and 1/sqrt(var + 1e-4) of the
device's z_b; x_{b+1} (block 9: H) against float64 BatchNorm + ELU + floor pooling of the device's z_b with the device's
stats_b.  Block 1's z exists only under ASR_TRAIN_RECOMPUTE1=0 (or a switch that implies it); otherwise the float64
convolution of the device's x_1 stands in for it.  An error names its kernel.

Stale buffers.  A whole step cannot start from NaN-filled buffers, so every checked call follows the same entry point
on another batch (seed 12): an element the kernels leave unwritten holds the other batch's value and fails the
element-wise comparison.  Nothing may be NaN.

Geometries (mutopia_ccal_cont unless said; ASR_TRAIN_TUNE=0, ASR_AUTOTUNE=0; synth_params(seed=1, trained_like=True),
fresh CCALayer; rng = default_rng(11), x1 = rng.random, x2 = 2 rng.random, float32):
    odd      53x75 / 35x27, 41   sheet maps 53x75, 26x37, 13x18, 6x9, 3x4, spectrogram maps 35x27, 17x13, 8x6, 4x3, 2x1:
                                 every pool sees an odd height or width in one tower, the first both (the uncovered
                                 border of bn_bwd_apply_kernel); N H W mod 64 = 31 / 25 (ragged last wave of block 1 and
                                 of its two backward readers); npix 12 and 2
    tiny     17x19 / 16x21, 37   last maps 1x1: BatchNorm over 37 values in blocks 8 and 9, grids larger than the work,
                                 tail_bwd_* waves without rows, pixel lanes without pixels
    odd_rsz  mutopia_ccal_cont_rsz, raw 107x151 uint8 / 35x27, 41   raw routes u8 and f32 only; floor drops a raw row
                                 and a column; prepared W = 75 takes the VEC = 1 build of prepare_view1_kernel.  The raw
                                 batch is rng.integers(0, 256) of default_rng(11), the reference oracle.network.prepare
No geometry had to move: train_begin accepted all three.

Legs: the default form in-process on `odd` and `tiny` under both pooling rules; each of ASR_TRAIN_FUSE_BN1=0,
ASR_TRAIN_FUSE_STATS=0, ASR_TRAIN_RECOMPUTE1=0, ASR_TRAIN_ZSEL=0 (selection from pool_mask alone) and
ASR_TRAIN_FUSED_REDUCE=1 in a fresh child process (they are read once per process) that dumps the device tensors of
both geometries to an .npz; the raw routes on `odd` (u8 and f32 bit-identical with the prepared route:
compute_gradients, burn_in, parameters after one train_step) and on `odd_rsz` (the same among its routes + the checks
above).  The float64 references are cached per geometry and content of what they were computed from.

Bars (the project's existing ones): z, x, H within 1e-4 max(1, max|ref|); mu 1e-4 absolute; inv_std 1e-4 relative;
gradients 1e-4 of the tensor's maximum, floored at 1e-3 of the tower's largest gradient.  One
allowance, measured against the reference only: the float32 oracle is evaluated with the same selection and the same dH;
where its error e32 on a tensor exceeds 5e-5 that tensor's bar is 2 e32.  e32 is printed beside the device's error for
every tensor.  tests/test_train_glue_host.py asserts e32 <= 1e-4 (block 9's beta aside) for a centred random dH, so
that no bar exceeds 2e-4 there.  With the DEVICE's dH that does not hold for block 9's gamma, and the test prints it:
the CCALayer's output does not change when a channel of H is rescaled, so the exact gradient of block 9's gamma almost
vanishes (8e-4 .. 6e-3 of the tower's largest gradient) while the terms dH xhat it sums do not; the float32 forward
error in xhat (1e-5) then shows - e32 = 3.9e-4 .. 1.8e-3 on that tensor (bars 7.8e-4 .. 3.5e-3), and 1.0e-4 .. 5.3e-4
on block 8's and 9's beta / gamma of the sheet tower of `odd`.  The device, which sums these in float64, measures
7.1e-5 .. 2.0e-4 on block 9's gamma and <= 7e-6 on the others: inside 2e-4 everywhere but `tiny`'s spectrogram tower
(2.04e-4).

Measured on an MI355X, worst error over all legs as a fraction of its bar / the float32 oracle's figure beside it:
    geometry tower  block 1         statistics      apply/pool      BatchNorm bwd   tail            (3x3 conv, wgrad)
    odd      1      0.062 / 0.411   0.001 / 0.208   0.001 / 0.001   0.075 / 0.500   0.091 / 0.500   0.014 / 0.192
    odd      2      0.041 / 0.218   0.001 / 0.035   0.001 / 0.002   0.047 / 0.365   0.069 / 0.500   0.016 / 0.141
    tiny     1      0.026 / 0.119   0.001 / 0.013   0.001 / 0.001   0.057 / 0.178   0.078 / 0.500   0.014 / 0.051
    tiny     2      0.042 / 0.094   0.001 / 0.026   0.001 / 0.001   0.124 / 0.390   0.285 / 0.500   0.035 / 0.093
    odd_rsz  1      0.031 / 0.317   0.001 / 0.212   0.001 / 0.001   0.064 / 0.500   0.022 / 0.500   0.019 / 0.281
    odd_rsz  2      0.027 / 0.169   0.001 / 0.074   0.001 / 0.001   0.048 / 0.269   0.113 / 0.500   0.017 / 0.107
Groups: block 1 = its statistics, its output and its three gradients (with ASR_TRAIN_RECOMPUTE1=0 also z); statistics =
mu and inv_std of blocks 2..8; apply/pool = the outputs of blocks 2..8; BatchNorm backward = dbeta, dgamma of blocks
2..8; tail = block 9's z, statistics, H and three gradients; the last column is what the 3x3 kernels add (z of blocks
2..8 from the device's own input, dW of blocks 2..8).  0.500 is a tensor whose bar is 2 e32.  Every imposed selection
was the float64 maximum exactly (gap 0), no pooling ties; the loss agreed to 1e-7.

Deliberate breaks (not committed; arithmetic only, no address or bound changed), each with the tests it failed:
    `if (!has_win) continue;` in bn_bwd_apply_kernel (the uncovered border keeps the other batch's dz): every test but
        the bit-identity of the raw routes on `odd` - the gradients of blocks 1 and 2 of both geometries off by 0.2 .. 1.6
        of their maximum;
    the `live` test dropped from conv1_raw_kernel's statistics sums: test_default_form_against_float64 (all four),
        the odd_rsz test and every switch but stats_pass (ASR_TRAIN_FUSE_STATS=0 takes the sums from bn_stats_*) - block
        1's mu off by 1.7e-4 .. 5.1e-3, inv_std by 7e-4 .. 1.1e-2, named as such;
    the eighth pixel lane's term dropped in tail_bwd_partial_kernel (`q < 7`): every test that runs `odd` or `odd_rsz`
        against float64 (sheet tower, npix = 12: block 9's dgamma off by 7 floors, dW by 0.15, all earlier gradients by
        1 .. 5 %); `tiny` (npix = 1) and the spectrogram towers (npix = 2) have no pixel in that lane and pass.

Durations on an MI355X (pytest --durations), the whole file 12.2 s:
    2.22 s odd_rsz; 1.90 / 1.66 / 1.05 / 1.05 / 1.00 s the switches (block1_raw_tensor, stats_pass, bn1_apply_pass,
    bn_bwd_rereads_windows, one_launch_reductions; two geometries each); 1.52 / 0.82 s odd all / first; 0.19 / 0.13 s
    tiny; 0.20 s the raw routes on `odd`.
"""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_train_glue_host import (E32_LIMIT, FWD_BAR, GEOMETRIES, RAW_ODD_RSZ, float32_tower, glue_inputs,
                                        glue_params, gradient_bars, gradient_errors, tower_gradients)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOLED = (1, 3, 5, 7)
SWITCHES = {"bn1_apply_pass": dict(ASR_TRAIN_FUSE_BN1="0"), "stats_pass": dict(ASR_TRAIN_FUSE_STATS="0"),
            "block1_raw_tensor": dict(ASR_TRAIN_RECOMPUTE1="0"), "bn_bwd_rereads_windows": dict(ASR_TRAIN_ZSEL="0"),
            "one_launch_reductions": dict(ASR_TRAIN_FUSED_REDUCE="1")}
_RECORDS = []          # (geometry, tower, group, what, error / bar, float32 oracle's error / bar)


@pytest.fixture(scope="module", autouse=True)
def _environment():
    """model plans, no timing, in this process and in the children; the cached references go at the module's end"""
    mp = pytest.MonkeyPatch()
    mp.setenv("ASR_TRAIN_TUNE", "0")
    mp.setenv("ASR_AUTOTUNE", "0")
    mp.delenv("ASR_TUNE_CACHE", raising=False)
    mp.delenv("ASR_POOL_TIES", raising=False)
    for env in SWITCHES.values():
        for k in env:
            mp.delenv(k, raising=False)
    yield
    _block_reference.cache_clear()
    _ORACLES.clear()
    mp.undo()


# ---- the device side (runs in this process or in a child) ---------------------------------------------------------------
def _raw_batch(geometry, seed):
    """the uint8 sheet batch of the raw routes: at the network's size for `odd`, 107x151 for `odd_rsz`"""
    _model, hw1, _hw2, B = GEOMETRIES[geometry]
    hw = RAW_ODD_RSZ if geometry == "odd_rsz" else hw1
    return np.random.default_rng(seed).integers(0, 256, (B, 1) + hw, dtype=np.uint8)


def _batch(geometry, route, seed):
    """(x1 as `route` takes it, x1 as the network sees it, x2)"""
    from oracle import network as onet
    model = GEOMETRIES[geometry][0]
    x1, x2 = glue_inputs(geometry, seed)
    if route == "float":                               # the float32 batch of the issue, prepared route
        return x1, x1, x2
    u8 = _raw_batch(geometry, seed)
    prepared = onet.prepare(u8, model)
    return {"prepared": prepared, "u8": u8, "f32": u8.astype(np.float32)}[route], prepared, x2


def _engine(geometry, ties):
    from audio_sheet_retrieval_amd import _lib
    model, hw1, hw2, B = GEOMETRIES[geometry]
    raw = RAW_ODD_RSZ if geometry == "odd_rsz" else hw1
    eng = _lib.Engine(model, h1=raw[0], w1=raw[1], h2=hw2[0], w2=hw2[1], pool_ties=ties)
    assert (eng.net_h1, eng.net_w1) == hw1
    eng.set_params(glue_params(model))
    eng.train_begin(B)
    return eng


def device_tensors(geometry, ties=None, route="float", step=False):
    """Every exported tensor of a burn_in and of a compute_gradients call on the checked batch, each after the same
    call on another batch; step=True: also the parameters after one train_step."""
    from audio_sheet_retrieval_amd import _lib
    B = GEOMETRIES[geometry][3]
    kw = dict(prepared=route in ("float", "prepared"))
    stale, _, stale2 = _batch(geometry, route, 12)
    x1, _, x2 = _batch(geometry, route, 11)
    eng = _engine(geometry, ties)
    d = dict(ties=np.array(eng.pool_ties))
    try:
        def get(kind, t, b=0):
            return eng.debug_train_tensor(kind, view=t + 1, index=b, batch=B)
        eng.burn_in(stale, stale2, **kw)
        d["lv1"], d["lv2"] = eng.burn_in(x1, x2, **kw)
        for t in range(2):
            for b in range(9):
                d["x%d_%d" % (t, b)] = get("x", t, b)
                d["st%d_%d" % (t, b)] = get("stats", t, b)
                try:
                    d["z%d_%d" % (t, b)] = get("z", t, b)
                except _lib.AsrError:
                    assert b == 0                       # block 1's raw output: recomputed by its readers, never stored
            d["H%d" % t] = get("H", t)
        eng.compute_gradients(stale, stale2, **kw)
        d["grads"], loss = eng.compute_gradients(x1, x2, **kw)
        d["loss"] = np.array(loss)
        for t in range(2):
            d["dH%d" % t] = get("dH", t)
            for b in POOLED:
                d["bz%d_%d" % (t, b)] = get("z", t, b)
                d["mask%d_%d" % (t, b)] = get("pool_mask", t, b)
                try:
                    d["zsel%d_%d" % (t, b)] = get("zsel", t, b)
                except _lib.AsrError:
                    pass                                # ASR_TRAIN_ZSEL=0 keeps none
        if step:
            eng.train_step(stale, stale2, 0.002, **kw)
            for i, p in enumerate(eng.get_params()):
                d["p%d" % i] = p
    finally:
        eng.close()
    return d


def _child_main(out, *geometries):
    np.savez(out, **{g + "/" + k: v for g in geometries for k, v in device_tensors(g).items()})


def _run_child(tmp_path, tag, env, geometries):
    out = str(tmp_path / (tag + ".npz"))
    e = dict(os.environ, PYTHONPATH=ROOT, **env)
    r = subprocess.run([sys.executable, "-c", "import sys; from tests.test_gpu_train_glue import _child_main; "
                        "_child_main(*sys.argv[1:])", out] + list(geometries), env=e, cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    data = np.load(out)
    return {g: {k.split("/", 1)[1]: data[k] for k in data.files if k.startswith(g + "/")} for g in geometries}


# ---- the float64 side ---------------------------------------------------------------------------------------------------
def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


_BLOCK_INPUTS = {}


def _block_forward(x, z_dev, st_dev, W, beta, gamma, blk, dtype):
    """one block in `dtype`: z = conv(x); statistics of z_dev where the device exported it, of z otherwise; the block's
    output from the same z with the DEVICE's statistics (block 9: the global mean)"""
    from oracle import network as onet
    x, W, beta, gamma = (np.asarray(a, dtype) for a in (x, W, beta, gamma))
    z = onet.conv2d_flip_nhwc_f64(x, W) if dtype == np.float64 else onet.conv2d_flip_nhwc(x, W)
    src = z if z_dev is None else np.asarray(z_dev, dtype)
    C = src.shape[-1]
    zf = src.reshape(-1, C)
    mu = zf.mean(axis=0, dtype=dtype)
    istd = (1.0 / np.sqrt(((zf - mu) ** 2).mean(axis=0, dtype=dtype) + dtype(1e-4))).astype(dtype)
    mu_d, istd_d = np.asarray(st_dev[:C], dtype), np.asarray(st_dev[C:], dtype)
    y = (src - mu_d) * (gamma * istd_d) + beta
    if blk == 8:
        out = y.reshape(y.shape[0], -1, C).mean(axis=1, dtype=dtype)
    else:
        out = np.where(y > 0, y, np.expm1(np.minimum(y, 0))).astype(dtype)
        if blk in POOLED:
            out = onet.maxpool2_nhwc(out)
    return z, mu, istd, out


@functools.lru_cache(maxsize=64)
def _block_reference(key):
    """The float64 block of the inputs parked under `key` (their digest) against what the device exported of it, and
    the float32 block against the float64 one.  z and the statistics are part of the key, so their errors are kept as
    numbers; the block's output is not - its float64 reference is kept."""
    args = _BLOCK_INPUTS.pop(key)
    _x, z_dev, st, W = args[:4]
    C = W.shape[0]
    z64, mu64, istd64, out64 = _block_forward(*args, np.float64)
    z32, mu32, istd32, out32 = _block_forward(*args, np.float32)
    return dict(z=None if z_dev is None else (_rel(z_dev, z64), _rel(z32, z64)),
                mu=(float(np.abs(st[:C] - mu64).max()), float(np.abs(mu32 - mu64).max())),
                inv_std=(float(np.abs(st[C:] / istd64 - 1).max()), float(np.abs(istd32 / istd64 - 1).max())),
                out64=out64, out_e32=_rel(out32, out64))


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, float(np.abs(ref).max())))


def _record(geometry, tower, group, what, err, e32, bar, failures):
    _RECORDS.append((geometry, tower, group, what, err / bar, e32 / bar))
    print("  %-8s tower %d %-18s %-22s device %.2e  float32 oracle %.2e  bar %.1e" % (geometry, tower + 1, group, what, err,
                                                                                      e32, bar))
    if not err <= bar:
        failures.append((geometry, tower + 1, what, err, bar))


def check_forward(geometry, d, x_net, exact_input=True):
    """the block-by-block forward checks of the module docstring on the tensors `d` of one device run"""
    model, hw1, hw2, B = GEOMETRIES[geometry]
    params = glue_params(model)
    failures = []
    xs = (x_net, glue_inputs(geometry)[1])
    for k, v in d.items():
        assert not (v.dtype.kind == "f" and np.isnan(v).any()), k
    for t, (h, w) in enumerate((hw1, hw2)):
        x_in = np.ascontiguousarray(np.transpose(xs[t], (0, 2, 3, 1)))
        x0 = d["x%d_0" % t].reshape(x_in.shape)
        if exact_input or t == 1:
            assert np.array_equal(x0, x_in), "tower %d: block 1's input is not the batch" % (t + 1)
        else:                                           # prepare_view1_kernel against oracle.network.prepare
            _record(geometry, t, "block 1", "prepared input", _rel(x0, x_in.astype(np.float64)), 0.0, FWD_BAR, failures)
        for b in range(9):
            W, beta, gamma = params[45 * t + 5 * b:45 * t + 5 * b + 3]
            cout, cin = W.shape[:2]
            x = d["x%d_%d" % (t, b)].reshape(B, h, w, cin)
            z_dev = d.get("z%d_%d" % (t, b))
            z_dev = None if z_dev is None else z_dev.reshape(B, h, w, cout)
            st = d["st%d_%d" % (t, b)]
            key = _digest(x, st, W, beta, gamma, *([] if z_dev is None else [z_dev])) + ":%d" % b
            _BLOCK_INPUTS[key] = (x, z_dev, st, W, beta, gamma, b)
            ref = _block_reference(key)
            _BLOCK_INPUTS.pop(key, None)
            group = "block 1" if b == 0 else "tail" if b == 8 else None
            name = "block %d " % (b + 1)
            if z_dev is not None:
                _record(geometry, t, group or "conv3x3", name + "z", *ref["z"], FWD_BAR, failures)
            _record(geometry, t, group or "statistics", name + "mu", *ref["mu"], 1e-4, failures)
            _record(geometry, t, group or "statistics", name + "inv_std", *ref["inv_std"], 1e-4, failures)
            nxt = d["H%d" % t] if b == 8 else d["x%d_%d" % (t, b + 1)]
            _record(geometry, t, group or "apply/pool", name + ("H" if b == 8 else "output"),
                    _rel(nxt.reshape(ref["out64"].shape), ref["out64"]), ref["out_e32"], FWD_BAR, failures)
            if b in POOLED:
                h, w = h // 2, w // 2
    assert not failures, failures


_ORACLES = {}


def _tower_oracle(geometry, x_net, routing, ties):
    """the float64 evaluation with `routing` imposed (loss, caches of both towers, route_check), kept per selection"""
    from oracle import train as otrain
    key = (geometry, ties, _digest(x_net, *[routing[t][b] for t in range(2) for b in POOLED]))
    if key not in _ORACLES:
        for k in [k for k in _ORACLES if k[0] == geometry]:          # one selection per geometry at a time
            del _ORACLES[k]
        model = GEOMETRIES[geometry][0]
        p64 = [q.astype(np.float64) for q in glue_params(model)]
        keep, diag = {}, {}
        x2 = glue_inputs(geometry)[1]
        loss = otrain.loss_and_grads(x_net.astype(np.float64), x2.astype(np.float64), p64, routing=routing, ties=ties,
                                     diag=diag, keep=keep, towers_backward=False)[0]
        _ORACLES[key] = dict(loss=float(loss), keep=keep, diag=diag, grads={})
    return _ORACLES[key]


def check_backward(geometry, d, x_net):
    """the gradient checks of the module docstring on the tensors `d` of one device run"""
    from tests.test_gpu_train_routed import ROUTE_GAP_BAR, routing_from_exports
    model, hw1, hw2, B = GEOMETRIES[geometry]
    params = glue_params(model)
    ties = str(d["ties"])
    for t in range(2):
        assert np.isfinite(d["dH%d" % t]).all(), "dH of tower %d" % (t + 1)
    assert np.isfinite(d["grads"]).all() and np.isfinite(d["loss"])

    def export(kind, view, index):
        return d.get({"z": "bz", "zsel": "zsel", "pool_mask": "mask"}[kind] + "%d_%d" % (view - 1, index))
    routing = routing_from_exports(export, params, B, hw1, hw2, ties)
    o = _tower_oracle(geometry, x_net, routing, ties)
    gap = max(v[0] for v in o["diag"].values())
    print("  %s (%s): loss %.7f vs %.7f, imposed selection falls short of the float64 maximum by <= %.1e"
          % (geometry, ties, float(d["loss"]), o["loss"], gap))
    assert gap <= ROUTE_GAP_BAR, o["diag"]
    assert abs(float(d["loss"]) - o["loss"]) <= 2e-5
    offs = np.concatenate([[0], np.cumsum([int(np.prod(q.shape)) for q in params])])
    xs = (x_net, glue_inputs(geometry)[1])
    failures = []
    for t in range(2):
        tp = params[45 * t:45 * t + 45]
        dH = d["dH%d" % t].reshape(B, 32).astype(np.float64)
        dkey = (t, _digest(dH))
        if dkey not in o["grads"]:
            ref = tower_gradients(tp, o["keep"]["cache"][t], o["keep"]["last_shape"][t], dH, ties, np.float64)
            g32 = float32_tower(xs[t], tp, routing[t], dH, ties)[0]
            o["grads"] = {k: v for k, v in o["grads"].items() if k[0] != t}
            o["grads"][dkey] = (ref, gradient_errors(g32, ref))
        ref, e32 = o["grads"][dkey]
        got = [d["grads"][offs[45 * t + 5 * (i // 3) + i % 3]:offs[45 * t + 5 * (i // 3) + i % 3 + 1]].reshape(ref[i].shape)
               for i in range(27)]
        errs = gradient_errors(got, ref)
        for i, (e, f, bar) in enumerate(zip(errs, e32, gradient_bars(e32))):
            blk, what = i // 3, ("W", "beta", "gamma")[i % 3]
            group = "block 1" if blk == 0 else "tail" if blk == 8 else "BatchNorm backward" if i % 3 else "conv3x3"
            _record(geometry, t, group, "block %d d%s" % (blk + 1, what), e, f, bar, failures)
            if f > E32_LIMIT:
                print("  %-8s tower %d block %d d%s: the float32 oracle is off by %.1e with the device's dH - this bar is "
                      "above 2e-4" % (geometry, t + 1, blk + 1, what, f))
    assert not failures, failures


def _summary():
    """worst error per kernel group as a fraction of its bar, by geometry and tower, the float32 oracle's beside it"""
    rows = {}
    for g, t, group, _what, e, f in _RECORDS:
        k = (g, t, group)
        rows[k] = (max(rows.get(k, (0, 0))[0], e), max(rows.get(k, (0, 0))[1], f))
    for (g, t, group), (e, f) in sorted(rows.items()):
        print("  summary %-8s tower %d %-18s device %.3f of its bar, float32 oracle %.3f" % (g, t + 1, group, e, f))
    _RECORDS.clear()


# ---- the tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", ["all", "first"])
@pytest.mark.parametrize("geometry", ["odd", "tiny"])
def test_default_form_against_float64(geometry, ties):
    d = device_tensors(geometry, ties)
    x_net = glue_inputs(geometry)[0]
    try:
        check_forward(geometry, d, x_net)
        check_backward(geometry, d, x_net)
    finally:
        _summary()


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_older_form_against_float64(switch, tmp_path):
    runs = _run_child(tmp_path, switch, SWITCHES[switch], ("odd", "tiny"))
    try:
        for geometry, d in runs.items():
            assert ("zsel0_1" in d) == (switch != "bn_bwd_rereads_windows")
            assert ("z0_0" in d) == (switch in ("bn1_apply_pass", "stats_pass", "block1_raw_tensor"))
            x_net = glue_inputs(geometry)[0]
            check_forward(geometry, d, x_net)
            check_backward(geometry, d, x_net)
    finally:
        _summary()


def _assert_same_run(a, b, what):
    for k in ("grads", "loss", "lv1", "lv2"):
        assert np.array_equal(a[k], b[k]), what + ": " + k
    assert all(np.array_equal(a["p%d" % i], b["p%d" % i]) for i in range(97)), what + ": parameters after a step"


def test_raw_routes_on_odd_maps_are_bit_identical_to_the_prepared_route():
    ref = device_tensors("odd", route="prepared", step=True)
    assert np.isfinite(ref["grads"]).all() and np.abs(ref["grads"]).max() > 0
    assert any(not np.array_equal(ref["p%d" % i], glue_params()[i]) for i in (0, 45))
    for route in ("u8", "f32"):
        _assert_same_run(ref, device_tensors("odd", route=route, step=True), route)


def test_raw_routes_with_resize_on_an_odd_raw_size_against_float64():
    from oracle import network as onet
    model = GEOMETRIES["odd_rsz"][0]
    runs = {route: device_tensors("odd_rsz", route=route, step=True) for route in ("u8", "f32")}
    _assert_same_run(runs["u8"], runs["f32"], "u8 vs f32")
    x_net = onet.prepare(_raw_batch("odd_rsz", 11), model)
    assert x_net.shape[2:] == GEOMETRIES["odd_rsz"][1]
    try:
        check_forward("odd_rsz", runs["u8"], x_net, exact_input=False)
        check_backward("odd_rsz", runs["u8"], x_net)
    finally:
        _summary()
