"""GPU: the two epilogues of conv3x3_wino4s - branch-free on rows-full M-tiles (per-column offsets or a sentinel that the
buffer store's range check drops; csrc/wino4_epilogue.h), guarded elsewhere - against the oracle and against each other.

Five samples in one chunk, F(4x4) forced where a block has it, block 1 materialised, a first different batch run
beforehand so that a store the second pass skipped would keep stale values.

"full": sheet 96x64, spectrogram 64x48.  Blocks 5-8 see 24x16 / 12x8 and 16x12 / 8x6: every tile is full, and
5 x 24 = 120 tiles are 7.5 M-tiles - the last M-tile has eight lanes past the end of the list, all sentinels.
"ragged": sheet 72x100, spectrogram 46x42.  The sheet's maps are 18x25 and 9x12: 7 tiles per row with a last tile one
pixel wide, five tile rows with a last one two rows high, so one launch holds rows-full M-tiles with ragged columns
(fast), M-tiles that touch the bottom tile row (guarded) and M-tiles that straddle images; the pooled lists
(2 OH = 18, 2 OW = 24) end in a one-row tile row; the spectrogram's 11x10 and 5x5 maps are ragged both ways.

Bars: those of test_gpu_embed_parity.py - activations of blocks 5-8 within 1e-4 of the layer's largest magnitude,
embeddings within 5e-6 of the oracle's - and bit equality of all eight activations and of the embeddings with a second
engine created under ASR_WINO4_EPI=0 (it takes the first engine's schedules from the tune cache that one wrote, so the
epilogue is the only difference)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL = "mutopia_ccal_cont"
N = 5
GEOMETRIES = {"full": ((96, 64), (64, 48)), "ragged": ((72, 100), (46, 42))}


def _block_outputs(onet, x, tparams):
    _, _, cache = onet.tower_forward(x, tparams, True, return_cache=True)
    outs = []
    for blk in range(8):
        a = cache[blk]["a"]
        outs.append(onet.maxpool2_nhwc(a) if blk in (1, 3, 5, 7) else a)
    return outs


@pytest.fixture(scope="module", params=sorted(GEOMETRIES))
def case(request):
    """Two different batches and the oracle's answer for the second one (computed once per geometry, read-only)."""
    from audio_sheet_retrieval_amd.utils import synth_data
    from oracle import network as onet
    shape1, shape2 = GEOMETRIES[request.param]
    params = synth_data.synth_params(onet.param_shapes(MODEL), seed=1, trained_like=True)
    batches = []
    for seed in (5, 6):
        rng = np.random.default_rng(seed)
        sheet = rng.integers(0, 256, size=(N, 1) + shape1, dtype=np.uint8)
        spec = (3.0 * rng.random((N, 1) + shape2) ** 2).astype(np.float32)
        batches.append((sheet, spec))
    sheet, spec = batches[1]
    x = onet.prepare(sheet, MODEL)
    ref = {"blocks": {1: _block_outputs(onet, x, params[0:45]), 2: _block_outputs(onet, spec, params[45:90])},
           "emb": onet.compute_output(x, spec, params)}
    for view in (1, 2):
        for a in ref["blocks"][view]:
            a.setflags(write=False)
    return (shape1, shape2), params, batches, ref


def _run(shapes, params, batches):
    """a fresh engine: first batch, then the second; the second batch's eight activations per tower and embeddings"""
    from audio_sheet_retrieval_amd import _lib
    (h1, w1), (h2, w2) = shapes
    eng = _lib.Engine(MODEL, h1=h1, w1=w1, h2=h2, w2=w2, max_chunk=N)
    eng.set_params(params)
    eng.embed_view1(batches[0][0], prepared=False)
    eng.embed_view2(batches[0][1])
    lv1 = eng.embed_view1(batches[1][0], prepared=False)
    lv2 = eng.embed_view2(batches[1][1])
    acts = {view: [eng.debug_activation(view, blk, N) for blk in range(8)] for view in (1, 2)}
    eng.close()
    return acts, (lv1, lv2)


def test_both_epilogues_match_the_oracle_and_each_other(case, monkeypatch, tmp_path):
    shapes, params, batches, ref = case
    monkeypatch.setenv("ASR_TUNE_ONLY", "wino4")
    monkeypatch.setenv("ASR_FUSE1", "0")                # block 1 materialised: all eight activations can be read back
    monkeypatch.setenv("ASR_TUNE_CACHE", str(tmp_path / "tune_cache.txt"))      # empty: the first engine times, the second follows
    monkeypatch.delenv("ASR_WINO4_EPI", raising=False)
    acts, emb = _run(shapes, params, batches)
    for view in (1, 2):
        for blk in range(4, 8):
            want, got = ref["blocks"][view][blk], acts[view][blk]
            assert got.shape == want.shape, (view, blk, got.shape, want.shape)
            scale = float(np.abs(want).max())
            err = float(np.abs(got - want).max())
            print("view %d block %d: max err %.3g (largest magnitude %.3g)" % (view, blk + 1, err, scale))
            assert err <= 1e-4 * scale, "view %d block %d: max err %g (largest magnitude %g)" % (view, blk + 1, err, scale)
    e1, e2 = float(np.abs(emb[0] - ref["emb"][0]).max()), float(np.abs(emb[1] - ref["emb"][1]).max())
    print("embeddings: max err %.3g / %.3g" % (e1, e2))
    assert e1 <= 5e-6 and e2 <= 5e-6, (e1, e2)

    monkeypatch.setenv("ASR_WINO4_EPI", "0")
    acts0, emb0 = _run(shapes, params, batches)
    for view in (1, 2):
        for blk in range(8):
            assert np.array_equal(acts[view][blk], acts0[view][blk]), "view %d block %d differs between the epilogues" % (view, blk + 1)
    assert np.array_equal(emb[0], emb0[0]) and np.array_equal(emb[1], emb0[1])
