"""GPU: conv3x3_wino (the LDS-patch Winograd kernel) with the dense weight layout (csrc/wino_lds_weight_layout.h): one
64-bit LDS read per pair of B operands, over runs of regions in which a workgroup reuses its two patch buffers.

Every block that has the family runs on it (ASR_TUNE_ONLY=wino, block 1 materialised).  Two engines: sheets 64x48 with
spectrograms 46x21, and sheets 50x38 with spectrograms 92x42 - the second sheet size has odd tile counts, so that the
last region row and column run the guarded border arm of the epilogue.

Five different samples per tower, against the oracle.  A workgroup reuses a patch buffer only from its third
consecutive region on, and the launch spreads the regions over every workgroup slot of the chip (up to three per
compute unit), so the five samples are repeated round-robin to a batch of 320 in ONE chunk: block 2 (12 -> 12, pooled;
6 to 18 regions of 32x8 pixels per sample at these sizes) then gives every workgroup a run of three to eight regions in
which neighbouring regions belong to different samples or different places.  A different batch runs first, so that a
stale patch buffer or a skipped tile shows.

Bars: those of test_gpu_winog_weight_layout.py - activations of blocks 2 and 3 of both towers within 1e-4 of the
layer's largest magnitude, embeddings within 5e-6 of the oracle's (measured: 1.5e-7 to 2.5e-7)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL = "mutopia_ccal_cont"
DISTINCT, REPEAT = 5, 64
N = DISTINCT * REPEAT


def _block_outputs(onet, x, tparams):
    _, _, cache = onet.tower_forward(x, tparams, True, return_cache=True)
    outs = {}
    for blk in (1, 2):                                   # blocks 2 and 3 (block 2 is followed by the pool)
        a = cache[blk]["a"]
        outs[blk] = onet.maxpool2_nhwc(a) if blk == 1 else a
    return outs


@pytest.fixture(scope="module", params=[((64, 48), (46, 21)), ((50, 38), (92, 42))],
                ids=["sheet64x48-spec46x21", "sheet50x38-spec92x42"])
def case(request):
    """Two different batches and the oracle's answer for the five samples of the second one (computed once, read-only)."""
    from audio_sheet_retrieval_amd.utils import synth_data
    from oracle import network as onet
    shape1, shape2 = request.param
    params = synth_data.synth_params(onet.param_shapes(MODEL), seed=1, trained_like=True)
    batches = []
    for seed in (7, 8):
        rng = np.random.default_rng(seed)
        sheet = rng.integers(0, 256, size=(DISTINCT, 1) + shape1, dtype=np.uint8)
        spec = (3.0 * rng.random((DISTINCT, 1) + shape2) ** 2).astype(np.float32)
        batches.append((sheet, spec))
    sheet, spec = batches[1]
    x = onet.prepare(sheet, MODEL)
    ref = {"blocks": {1: _block_outputs(onet, x, params[0:45]), 2: _block_outputs(onet, spec, params[45:90])},
           "emb": onet.compute_output(x, spec, params)}
    for view in (1, 2):
        for a in ref["blocks"][view].values():
            a.setflags(write=False)
    return shape1, shape2, params, batches, ref


def test_wino_blocks_match_the_oracle_over_runs_of_regions(case, monkeypatch):
    from audio_sheet_retrieval_amd import _lib
    shape1, shape2, params, batches, ref = case
    monkeypatch.setenv("ASR_TUNE_ONLY", "wino")
    monkeypatch.setenv("ASR_FUSE1", "0")                # block 1 materialised: the activations can be read back
    monkeypatch.delenv("ASR_TUNE_CACHE", raising=False)
    monkeypatch.setenv("ASR_HOST_GRANULE", str(N))      # host batches go through the towers whole: one launch per block
    monkeypatch.setenv("ASR_HOST_GRANULE_FIRST", str(N))
    eng = _lib.Engine(MODEL, h1=shape1[0], w1=shape1[1], h2=shape2[0], w2=shape2[1], max_chunk=N)
    eng.set_params(params)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (REPEAT,) + (1,) * (a.ndim - 1)))      # samples 0 1 2 3 4 0 1 ...
    eng.embed_view1(tile(batches[0][0]), prepared=False)
    eng.embed_view2(tile(batches[0][1]))
    lv1 = eng.embed_view1(tile(batches[1][0]), prepared=False)
    lv2 = eng.embed_view2(tile(batches[1][1]))
    for view in (1, 2):
        for blk in (1, 2):
            want = ref["blocks"][view][blk]
            got = eng.debug_activation(view, blk, N)
            assert got.shape == (N,) + want.shape[1:], (view, blk, got.shape, want.shape)
            scale = max(1.0, float(np.abs(want).max()))
            err = float(np.abs(got.reshape((REPEAT,) + want.shape) - want[None]).max())
            print("view %d block %d: max err %.3g (scale %.3g)" % (view, blk + 1, err, scale))
            assert err <= 1e-4 * scale, "view %d block %d: max err %g (scale %g)" % (view, blk + 1, err, scale)
    e1 = float(np.abs(lv1.reshape(REPEAT, DISTINCT, -1) - ref["emb"][0][None]).max())
    e2 = float(np.abs(lv2.reshape(REPEAT, DISTINCT, -1) - ref["emb"][1][None]).max())
    print("embeddings: max err %.3g / %.3g" % (e1, e2))
    assert e1 <= 5e-6 and e2 <= 5e-6, (e1, e2)
    eng.close()
