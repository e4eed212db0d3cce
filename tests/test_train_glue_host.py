"""CPU: what tests/test_gpu_train_glue.py rests on, checked without a device.

Conditioning guard.  The GPU test compares each tower's 27 gradient tensors with float64 at 1e-4 of the tensor's maximum
(floored at 1e-3 of the tower's largest gradient) and allows a tensor 2 x e32 where the FLOAT32 oracle's own error e32
on it exceeds 5e-5.  That allowance is only honest while the inputs keep e32 small, so it is asserted here for the
geometries `odd` and `tiny` of that test, with a seeded, centred random dH in place of the device's: e32 <= 1e-4 on
every tensor but block 9's beta (its exact gradient is zero - the upstream gradient is centred - so both sides hold
rounding noise under the floor).  With such a dH no bar exceeds 2e-4, and a later change of inputs cannot loosen the
bars quietly.  (With the device's own dH the float32 oracle does worse on block 9's gamma, whose exact gradient nearly
vanishes as well - the GPU test prints and documents that.)  The forward figures (z, statistics, H of the float32 oracle against float64) have to stay under half the
forward bar of 1e-4: a device that rounds like the float32 oracle then still fits.

Index arithmetic.  The pooled BatchNorm kernels of the training step compute q / OW as (int)((q + 0.5f) * (1.0f / OW)).
The expression is emulated in NumPy float32 and must be exact for every divisor d <= 2048 and every row r < 2048 at
both ends of the row, r d and r d + d - 1 (the float32 product is monotone in q, so the row's interior lies between):
the domain of a pooled map of the largest input asr_set_input_size admits (4096 x 4096).  That is the domain fdivt
(train_fwd_kernels.hip) and fdivb (train_bwd_kernels.hip) are called on - cells of a pooled map or of its ceil(H/2) x
ceil(W/2) cover; the comment on the original in conv_kernels.hip proves n < 2^20 only.  Beyond it the expression does
miss: first at n = 4 201 469 with d = 4095, which no pooled map reaches.
"""
import functools

import numpy as np
import pytest

MODEL = "mutopia_ccal_cont"
# name: (model, sheet as the network sees it, spectrogram, batch)
GEOMETRIES = {"odd": (MODEL, (53, 75), (35, 27), 41),
              "tiny": (MODEL, (17, 19), (16, 21), 37),
              "odd_rsz": (MODEL + "_rsz", (53, 75), (35, 27), 41)}
RAW_ODD_RSZ = (107, 151)          # floor drops a raw row and a column; prepared W = 75 is no multiple of 4
E32_ALLOW_FROM, E32_LIMIT = 5e-5, 1e-4
FWD_BAR = 1e-4


@functools.lru_cache(maxsize=None)
def glue_params(model=MODEL):
    from audio_sheet_retrieval_amd.utils import synth_data
    from oracle import network as onet
    params = synth_data.synth_params(onet.param_shapes(model), seed=1, trained_like=True)
    for i in range(90, 97):
        params[i] = np.zeros_like(params[i])                 # fresh CCALayer
    return params


def glue_inputs(geometry, seed=11):
    """(x1 as the network sees it, x2), float32; seed 11 is the checked batch, any other a batch that leaves stale values"""
    _model, hw1, hw2, B = GEOMETRIES[geometry]
    rng = np.random.default_rng(seed)
    x1 = rng.random((B, 1) + hw1).astype(np.float32)
    x2 = (2 * rng.random((B, 1) + hw2)).astype(np.float32)
    return x1, x2


def gradient_errors(got, ref):
    """per tensor: max |got - ref| over max(max |ref|, 1e-3 of the largest gradient of the list) - BASELINE.md section 3"""
    gmax = max(float(np.abs(r).max()) for r in ref)
    return [float(np.abs(np.asarray(g, np.float64) - r).max() / max(1e-3 * gmax, float(np.abs(r).max()))) for g, r in zip(got, ref)]


def l2_terms(tparams, l2=1e-5):
    """the weight-decay term of the train loss on [W, beta, gamma] x 9 (train_dcca_pool.py:141-142)"""
    return [2.0 * l2 * tparams[5 * (i // 3) + i % 3].astype(np.float64) for i in range(27)]


def tower_gradients(tparams, cache, last_shape, dH, ties, dtype):
    """oracle.train.tower_backward + the L2 term, as compute_gradients reports them"""
    from oracle import train as otrain
    p = [q.astype(dtype) for q in tparams]
    g = otrain.tower_backward(p, cache, last_shape, np.asarray(dH, dtype), ties)
    return [a.astype(np.float64) + b for a, b in zip(g, l2_terms(tparams))]


def float32_tower(x_nchw, tparams, routing, dH, ties):
    """the float32 oracle of one tower with an imposed selection and a given dH: (gradients incl. L2, H, stats, cache)"""
    from oracle import train as otrain
    p32 = [q.astype(np.float32) for q in tparams]
    H, stats, cache, ls = otrain.tower_forward_train(x_nchw.astype(np.float32), p32, routing)
    return tower_gradients(tparams, cache, ls, dH, ties, np.float32), H, stats, cache


def gradient_bars(e32):
    """1e-4; where the float32 oracle's own error exceeds 5e-5, twice that error"""
    return [1e-4 if e <= E32_ALLOW_FROM else 2.0 * e for e in e32]


def free_selection(cache):
    """{block: the set of window elements equal to the maximum} of an evaluation's own activations"""
    from oracle import train as otrain
    out = {}
    for blk in (1, 3, 5, 7):
        win = otrain._windows(cache[blk]["a"])
        out[blk] = win == win.max(axis=-1, keepdims=True)
    return out


@pytest.mark.parametrize("geometry", ["odd", "tiny"])
def test_float32_oracle_stays_within_the_allowance(geometry):
    from oracle import train as otrain
    params = glue_params()
    xs = glue_inputs(geometry)
    B = xs[0].shape[0]
    for t, x in enumerate(xs):
        tp = params[45 * t:45 * t + 45]
        p64 = [q.astype(np.float64) for q in tp]
        H64, st64, c64, ls = otrain.tower_forward_train(x.astype(np.float64), p64)
        sel = free_selection(c64)
        assert all((s.sum(axis=-1) == 1).all() for s in sel.values()), "pooling ties in the float64 evaluation"
        dH = np.random.default_rng([12, t]).standard_normal((B, 32))
        dH -= dH.mean(axis=0, keepdims=True)
        ref = tower_gradients(tp, c64, ls, dH, "all", np.float64)
        g32, H32, st32, c32 = float32_tower(x, tp, sel, dH, "all")
        e32 = gradient_errors(g32, ref)
        fwd = [float(np.abs(H32 - H64).max() / max(1.0, np.abs(H64).max()))]
        for blk in range(9):
            z = c64[blk]["z"]
            fwd.append(float(np.abs(c32[blk]["z"] - z).max() / max(1.0, np.abs(z).max())))
            fwd.append(float(np.abs(st32[blk][0] - st64[blk][0]).max()))
            fwd.append(float(np.abs(st32[blk][1] / st64[blk][1] - 1).max()))
        worst = max(e for i, e in enumerate(e32) if i != 25)
        print("%s tower %d: e32 worst %.1e (tensor %d), block 9's beta %.1e, forward worst %.1e"
              % (geometry, t + 1, worst, max((i for i in range(27) if i != 25), key=lambda i: e32[i]), e32[25], max(fwd)))
        assert worst <= E32_LIMIT, e32
        assert max(gradient_bars([e for i, e in enumerate(e32) if i != 25])) <= 2e-4
        assert max(fwd) <= 0.5 * FWD_BAR, fwd


def test_reciprocal_row_index_is_exact_on_pooled_maps():
    d = np.arange(1, 2049, dtype=np.int64)[:, None]
    r = np.arange(2048, dtype=np.int64)[None, :]
    rcp = np.float32(1.0) / d.astype(np.float32)
    for n in (r * d, r * d + d - 1):
        assert n.max() < 2 ** 23                             # n and n + 0.5 are float32 values
        got = ((n.astype(np.float32) + np.float32(0.5)) * rcp).astype(np.int32)
        assert got.dtype == np.int32 and np.array_equal(got, np.broadcast_to(r, n.shape)), np.argwhere(got != r)[:4]
