"""GPU: conv3x3_winog with the dense weight layout (csrc/wino_weight_layout.h) and the input transform that reads the
loaded patch in place.

Engine 128x96 / 64x48, five samples in one chunk, every block on the global-A Winograd kernels (ASR_TUNE_ONLY=winog):
blocks 3-4 of the sheet tower run at 64x48 (32x24 = 768 tiles per image: M-tiles whose 16 patches all lie inside the
image take the form without border selects, those along the edges the other), the spectrogram tower's at 32x24 (192
tiles) and blocks 5-8 at 16x12 / 8x6 and below, where 16 consecutive tiles straddle strips and images.  Block 4
(24 -> 24, two n-tiles) reads its weights in the dense form, block 3 (12 -> 24: a remainder k-step) and the
three-n-tile blocks in the row-major one.

Bars: those of test_gpu_winograd_tile_walk.py - activations within 1e-4 of the layer's largest magnitude, embeddings
within 5e-6 of the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL = "mutopia_ccal_cont"
N = 5
SHAPE1, SHAPE2 = (128, 96), (64, 48)


def _block_outputs(onet, x, tparams):
    _, _, cache = onet.tower_forward(x, tparams, True, return_cache=True)
    outs = []
    for blk in range(8):
        a = cache[blk]["a"]
        outs.append(onet.maxpool2_nhwc(a) if blk in (1, 3, 5, 7) else a)
    return outs


@pytest.fixture(scope="module")
def case():
    """Two different batches and the oracle's answer for the second one (computed once, read-only)."""
    from audio_sheet_retrieval_amd.utils import synth_data
    from oracle import network as onet
    params = synth_data.synth_params(onet.param_shapes(MODEL), seed=1, trained_like=True)
    batches = []
    for seed in (7, 8):
        rng = np.random.default_rng(seed)
        sheet = rng.integers(0, 256, size=(N, 1) + SHAPE1, dtype=np.uint8)
        spec = (3.0 * rng.random((N, 1) + SHAPE2) ** 2).astype(np.float32)
        batches.append((sheet, spec))
    sheet, spec = batches[1]
    x = onet.prepare(sheet, MODEL)
    ref = {"blocks": {1: _block_outputs(onet, x, params[0:45]), 2: _block_outputs(onet, spec, params[45:90])},
           "emb": onet.compute_output(x, spec, params)}
    for view in (1, 2):
        for a in ref["blocks"][view]:
            a.setflags(write=False)
    return params, batches, ref


def test_winog_blocks_match_the_oracle_on_a_second_batch(case, monkeypatch):
    from audio_sheet_retrieval_amd import _lib
    params, batches, ref = case
    monkeypatch.setenv("ASR_TUNE_ONLY", "winog")
    monkeypatch.setenv("ASR_FUSE1", "0")                # block 1 materialised: all eight activations can be read back
    monkeypatch.delenv("ASR_TUNE_CACHE", raising=False)
    eng = _lib.Engine(MODEL, h1=SHAPE1[0], w1=SHAPE1[1], h2=SHAPE2[0], w2=SHAPE2[1], max_chunk=N)
    eng.set_params(params)
    # a first, different batch leaves its activations in the buffers: a tile the second pass skipped would keep them
    eng.embed_view1(batches[0][0], prepared=False)
    eng.embed_view2(batches[0][1])
    lv1 = eng.embed_view1(batches[1][0], prepared=False)
    lv2 = eng.embed_view2(batches[1][1])
    for view in (1, 2):
        for blk in range(8):
            want = ref["blocks"][view][blk]
            got = eng.debug_activation(view, blk, N)
            assert got.shape == want.shape, (view, blk, got.shape, want.shape)
            scale = max(1.0, float(np.abs(want).max()))
            err = float(np.abs(got - want).max())
            print("view %d block %d: max err %.3g (scale %.3g)" % (view, blk + 1, err, scale))
            assert err <= 1e-4 * scale, "view %d block %d: max err %g (scale %g)" % (view, blk + 1, err, scale)
    e1, e2 = float(np.abs(lv1 - ref["emb"][0]).max()), float(np.abs(lv2 - ref["emb"][1]).max())
    print("embeddings: max err %.3g / %.3g" % (e1, e2))
    assert e1 <= 5e-6 and e2 <= 5e-6, (e1, e2)
    eng.close()
