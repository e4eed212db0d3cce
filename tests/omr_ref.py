"""Test restatement of the staff-system detector's networks (sheet_utils/system_detector.py, omr.py): the U-Net
forward in numpy (float64 by default) and SegmentationNetwork's sliding-window tiling, written from the reference's
graph and loop.  The host post-processing is the package's (sheet_utils/omr.py); tests/test_omr_host.py checks it
against brute-force versions of the library functions it restates.

Transposed-conv orientation.  Lasagne's TransposedConv2DLayer (flip_filters=False) computes the input gradient of a
Theano conv with filter_flip=True whose kernel is W (C_in, C_out, 2, 2) read as (out, in, kh, kw).  That forward conv
maps y (C_out channels) to x (C_in channels):

    x[ci, p, q] = sum_{co, u, v} y[co, 2p + u, 2q + v] * W[ci, co, 1 - u, 1 - v]        (filter_flip: true convolution)

Its adjoint (the input gradient), with stride 2 and a 2x2 kernel (no overlap), is

    y[co, 2i + a, 2j + b] = sum_ci x[ci, i, j] * W[ci, co, 1 - a, 1 - b]

which is `transposed_conv(..., flip=True)`.  flip=False (W[ci, co, a, b]) is the other reading, kept to measure how
strongly the page anchor separates the two.  tests/test_omr_host.py pins the rule with the adjoint identity
<strided_corr(y), x> == <y, transposed_conv(x)> against `strided_corr`, the forward conv written directly.
"""
import numpy as np

N_PARAMS = 99


def params_from_npz(path):
    z = np.load(path)
    return [z["p%02d" % i] for i in range(N_PARAMS)]


def conv3_same_flip(x, W, dtype=np.float64):
    """Conv2DLayer(flip_filters=True, pad='same', no bias).  x: (ci, H, W); W: (co, ci, 3, 3) -> (co, H, W).
    Evaluated by torch's CPU correlation on the flipped kernel, in `dtype`."""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype))[None]
    wt = torch.from_numpy(np.ascontiguousarray(np.asarray(W)[:, :, ::-1, ::-1], dtype))
    with torch.no_grad():
        return torch.nn.functional.conv2d(xt, wt, padding=1)[0].numpy()


def bn(x, p, dtype=np.float64):
    beta, gamma, mean, inv_std = [np.asarray(a, dtype)[:, None, None] for a in p]
    return (x - mean) * (gamma * inv_std) + beta


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def maxpool2(x):
    c, h, w = x.shape
    return x.reshape(c, h // 2, 2, w // 2, 2).max(axis=(2, 4))


def transposed_conv(x, W, flip=True, dtype=np.float64):
    """TransposedConv2DLayer(filter_size=2, stride=2, no bias).  x: (ci, h, w); W: (ci, co, 2, 2) -> (co, 2h, 2w)"""
    ci, h, w = x.shape
    co = W.shape[1]
    Wt = np.asarray(W, dtype)
    out = np.zeros((co, 2 * h, 2 * w), dtype)
    xf = x.reshape(ci, -1)
    for a in range(2):
        for b in range(2):
            k = Wt[:, :, 1 - a, 1 - b] if flip else Wt[:, :, a, b]
            out[:, a::2, b::2] = (k.T @ xf).reshape(co, h, w)
    return out


def strided_corr(y, W):
    """the forward conv whose input gradient the transposed conv is, written directly:
    x[ci, p, q] = sum_{co,u,v} y[co, 2p+u, 2q+v] * W[ci, co, 1-u, 1-v].  y: (co, 2h, 2w) -> (ci, h, w)"""
    co, H, Wd = y.shape
    ci = W.shape[0]
    x = np.zeros((ci, H // 2, Wd // 2))
    for c in range(ci):
        for o in range(co):
            for u in range(2):
                for v in range(2):
                    x[c] += y[o, u::2, v::2] * W[c, o, 1 - u, 1 - v]
    return x


def sigmoid_f32_theano(z):
    """theano's float32 scalar sigmoid: 0 below -88, 1 above 15"""
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-z))
    return np.where(z < -88.0, 0.0, np.where(z > 15.0, 1.0, s))


def unet_forward(x, params, flip=True, dtype=np.float64):
    """system_detector.build_model() in inference mode on one prepared tile x (H, W) -> (H, W) probabilities"""
    P = params
    h = np.asarray(x, dtype)[None]
    i = 0
    skips = []

    def conv_bn(h, i):
        return elu(bn(conv3_same_flip(h, P[i], dtype), P[i + 1:i + 5], dtype)), i + 5

    for lv in range(4):
        h, i = conv_bn(h, i)
        h, i = conv_bn(h, i)
        if lv < 3:
            skips.append(h)
            h = maxpool2(h)
    for lv in range(3):
        h = transposed_conv(h, P[i], flip, dtype)
        h = np.maximum(bn(h, P[i + 1:i + 5], dtype), 0)
        h = skips.pop() + h
        h = bn(h, P[i + 5:i + 9], dtype)
        i += 9
        h, i = conv_bn(h, i)
        h, i = conv_bn(h, i)
    z = np.tensordot(np.asarray(P[97], dtype)[0, :, 0, 0], h, axes=(0, 0)) + np.asarray(P[98], dtype)[0]
    assert i == 97
    return sigmoid_f32_theano(z)


def sliding_window(page, tile_shape, net, overlap=0.5):
    """SegmentationNetwork.predict_proba on one page (h, w): a tile-sized page goes through `net` directly, any other
    through the reference's padded, Hamming-weighted float64 sliding window.  net: tile (th, tw) -> (th, tw)."""
    th, tw = tile_shape
    h, w = page.shape
    if (h, w) == (th, tw):
        return np.asarray(net(page))
    missing_h = int(th * np.ceil(float(h) / th) - h)
    missing_w = int(tw * np.ceil(float(w) / tw) - w)
    pad_top, pad_left = missing_h // 2, missing_w // 2
    img = np.pad(page, ((pad_top, missing_h - pad_top), (pad_left, missing_w - pad_left)), mode="constant")
    row_0 = np.arange(0, img.shape[0] - th + 1, int(th * (1.0 - overlap)))
    col_0 = np.arange(0, img.shape[1] - tw + 1, int(tw * (1.0 - overlap)))
    ham2d = np.sqrt(np.outer(np.hamming(th), np.hamming(tw)))
    R = np.zeros(img.shape)
    V = np.zeros(img.shape)
    for r0 in row_0:
        for c0 in col_0:
            Pt = net(img[r0:r0 + th, c0:c0 + tw])
            R[r0:r0 + th, c0:c0 + tw] += Pt * ham2d
            V[r0:r0 + th, c0:c0 + tw] += ham2d
    R = R[pad_top:pad_top + h, pad_left:pad_left + w]
    V = V[pad_top:pad_top + h, pad_left:pad_left + w]
    with np.errstate(invalid="ignore"):
        return R / V


def tiles_of(page, tile_shape, overlap=0.5):
    """the tiles the sliding window feeds to the network, in its order (for stitching given tile outputs)"""
    th, tw = tile_shape
    out = []
    sliding_window(page, tile_shape, lambda t: out.append(np.array(t)) or np.zeros(tile_shape), overlap)
    return out


def stitch_given(page_shape, tile_shape, tile_outputs, overlap=0.5):
    """sliding_window with the network replaced by the given tile outputs, in tile order"""
    it = iter(tile_outputs)
    return sliding_window(np.zeros(page_shape, np.float32), tile_shape, lambda t: next(it), overlap)
