"""GPU: the consumers of conv3x3_wino4s with their register classes swapped - accumulators in VGPRs, B operands loaded
straight into AGPRs, all 216 of a lane's weights resident at C_in = 24 - against the float64 oracle.  The MFMAs, the
weight loads and the waits between them are inline assembly there, so what the compiler would have counted and padded
is placed by hand; a wait that is one load short or a missing hazard pad shows as wrong values, not as a fault.

Blocks 5-8 of both towers are pinned to 4005 / 4006 / 4007 / 4006 (24 -> 48 resident, 48 -> 48 pooled, 48 -> 48, 48 -> 48
pooled; conv_wino4_kernels.hip, g_wino4) through the test's own tune cache, as tests/test_gpu_wino4_producer.py does,
and the test asserts from that cache that they ran.  A first, different batch runs beforehand.

"ragged": sheet 88x104, three samples.  Blocks 5/6 see 22x26 maps: 42 tiles per image, 126 in all - an M-tile that spans
    two images, 14 live lanes in the last one, bottom tile rows two pixels deep: the guarded epilogue, whose stores the
    next M-tile's first step drains before it reads its weights.
"bench": the benchmark's 160x200 / 92x42 with twelve samples: rows-full M-tiles, the branch-free epilogues with their
    static store counts (16 pooled, 64 un-pooled) that the counted wait of the next M-tile's first step leaves in flight.
"single": one sample of 16x16 in both towers.  Blocks 5/6 see 4x4 maps: one tile, fewer than one M-tile - the resident
    weights' prologue with a single pass through the M-tile loop, one workgroup, 15 lanes past the end of the list.

Bar: the project's - activations of blocks 5-8 and both embeddings within 1e-4 of the tensor's largest magnitude.

Training: the RAW builds keep the compiler-allocated path behind the template's RAW parameter.  One step's forward pass
with them forced, in a process of its own (the switch is read once per process), to show that they still run and still
agree with the oracle's raw outputs z at the same bar."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL = "mutopia_ccal_cont"
# name: (sheet size, spectrogram size, samples)
GEOMETRIES = {"ragged": ((88, 104), (92, 42), 3), "bench": ((160, 200), (92, 42), 12), "single": ((16, 16), (16, 16), 1)}
# blocks 5-8 (tuner index b = 4..7) -> the conv3x3_wino4s entry of the library's F(4x4) table, tile 4 x 64, NI 16
WINO4S = {4: 4005, 5: 4006, 6: 4007, 7: 4006}


def _block_outputs(onet, x, tparams):
    _, _, cache = onet.tower_forward(x, tparams, True, return_cache=True)
    return [onet.maxpool2_nhwc(cache[blk]["a"]) if blk in (5, 7) else cache[blk]["a"] for blk in range(4, 8)]


@pytest.fixture(scope="module", params=sorted(GEOMETRIES))
def case(request):
    """Two different batches and the oracle's blocks 5-8 and embeddings for the second (once per geometry, read-only)."""
    from audio_sheet_retrieval_amd.utils import synth_data
    from oracle import network as onet
    shape1, shape2, n = GEOMETRIES[request.param]
    params = synth_data.synth_params(onet.param_shapes(MODEL), seed=1, trained_like=True)
    batches = []
    for seed in (7, 8):
        rng = np.random.default_rng(seed)
        sheet = rng.integers(0, 256, size=(n, 1) + shape1, dtype=np.uint8)
        spec = (3.0 * rng.random((n, 1) + shape2) ** 2).astype(np.float32)
        batches.append((sheet, spec))
    sheet, spec = batches[1]
    x = onet.prepare(sheet, MODEL)
    ref = {1: _block_outputs(onet, x, params[0:45]), 2: _block_outputs(onet, spec, params[45:90]),
           "emb": [np.asarray(e) for e in onet.compute_output(x, spec, params)]}
    for a in ref[1] + ref[2] + ref["emb"]:
        a.setflags(write=False)
    return (shape1, shape2), n, params, batches, ref


def _tune_tag(lib):
    """the tag a tune-cache line must carry to be read by this build (asr_api.hip, tune_cache_tag)"""
    h = 2166136261
    for ch in lib.asr_version():
        h = ((h ^ ch) * 16777619) & 0xffffffff
    return h & 0x7fffffff


def _cache_lines(cache):
    """{(view, b): [variant, ...]} of the schedule lines of a tune cache"""
    picks = {}
    for ln in cache.read_text().splitlines():
        f = ln.split()
        if f and f[0] == "v2":
            picks.setdefault((int(f[3]), int(f[4])), []).append(int(f[8]))
    return picks


def test_swapped_register_classes_match_the_oracle(case, monkeypatch, tmp_path):
    from audio_sheet_retrieval_amd import _lib
    ((h1, w1), (h2, w2)), n, params, batches, ref = case
    cache = tmp_path / "tune_cache.txt"
    monkeypatch.setenv("ASR_TUNE_ONLY", "wino4")
    monkeypatch.setenv("ASR_FUSE1", "0")
    monkeypatch.setenv("ASR_TUNE_CACHE", str(cache))
    monkeypatch.delenv("ASR_WINO4_EPI", raising=False)  # the branch-free epilogues where the M-tiles admit them
    tag = _tune_tag(_lib.load_library())
    cache.write_text("".join("v2 %d 12 %d %d %d %d %d %d 4 64 16\n" % (tag, view, b, h >> (2 if b < 6 else 3), w >> (2 if b < 6 else 3), n, WINO4S[b])
                             for view, (h, w) in ((1, (h1, w1)), (2, (h2, w2))) for b in sorted(WINO4S)))
    eng = _lib.Engine(MODEL, h1=h1, w1=w1, h2=h2, w2=w2, max_chunk=n)
    eng.set_params(params)
    eng.embed_view1(batches[0][0], prepared=False)
    eng.embed_view2(batches[0][1])
    emb = [eng.embed_view1(batches[1][0], prepared=False), eng.embed_view2(batches[1][1])]
    acts = {view: [eng.debug_activation(view, blk, n) for blk in range(4, 8)] for view in (1, 2)}
    eng.close()
    picks = _cache_lines(cache)
    print("schedules (view, b): variant  " + "; ".join("(%d, %d): %s" % (k + (v,)) for k, v in sorted(picks.items())))
    for view in (1, 2):
        for b, variant in WINO4S.items():
            assert picks.get((view, b)) == [variant], "view %d block %d did not run conv3x3_wino4s: %s" % (view, b + 1, picks.get((view, b)))
    bad = []
    for view in (1, 2):
        for k, (want, got) in enumerate(zip(ref[view], acts[view])):
            assert got.shape == want.shape, (view, k + 5, got.shape, want.shape)
            scale = float(np.abs(want).max())
            err = float(np.abs(got - want).max())
            print("view %d block %d (%dx%d): max err %.3g (largest magnitude %.3g)" % (view, k + 5, want.shape[1], want.shape[2], err, scale))
            if not err <= 1e-4 * scale:
                bad.append((view, k + 5, err, scale))
        want, got = ref["emb"][view - 1], np.asarray(emb[view - 1])
        assert got.shape == want.shape, (view, got.shape, want.shape)
        scale = float(np.abs(want).max())
        err = float(np.abs(got - want).max())
        print("view %d embedding: max err %.3g (largest magnitude %.3g)" % (view, err, scale))
        if not err <= 1e-4 * scale:
            bad.append((view, "embedding", err, scale))
    assert not bad, bad


_TRAIN_SCRIPT = r"""
import sys, numpy as np
from audio_sheet_retrieval_amd import _lib
from audio_sheet_retrieval_amd.utils import synth_data
from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
model, B, hw1, hw2 = "mutopia_ccal_cont", 4, (48, 64), (32, 24)
rng = np.random.default_rng(11)
params = synth_data.synth_params(param_shapes(model), seed=1, trained_like=True)
for i in range(90, 97):
    params[i] = np.zeros_like(params[i])
x1 = rng.random((B, 1) + hw1).astype(np.float32)
x2 = (rng.random((B, 1) + hw2) * 2).astype(np.float32)
eng = _lib.Engine(model)
eng.set_input_size(1, *hw1)
eng.set_input_size(2, *hw2)
eng.set_params(params)
eng.train_begin(B)
eng.compute_gradients(x1, x2)
out = {"x1": x1, "x2": x2}
for view in (1, 2):
    for blk in range(4, 8):
        out["z%d_%d" % (view, blk)] = eng.debug_train_tensor("z", view=view, index=blk, batch=B)
np.savez(sys.argv[1], **out)
eng.close()
"""


def test_the_raw_builds_still_run_a_training_forward_pass(tmp_path):
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    from oracle import train as otrain
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "z.npz")
    # forward convolutions on the RAW F(4x4) builds wherever one exists, the planner's choice elsewhere, nothing timed
    env = dict(os.environ, PYTHONPATH=root, ASR_TRAIN_WINO4="3", ASR_TRAIN_TUNE="0")
    r = subprocess.run([sys.executable, "-c", _TRAIN_SCRIPT, out], env=env, cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    params = synth_data.synth_params(param_shapes(MODEL), seed=1, trained_like=True)
    p64 = [q.astype(np.float64) for q in params]
    bad = []
    for view, x, tp in ((1, got["x1"], p64[0:45]), (2, got["x2"], p64[45:90])):
        _, _, cache, _ = otrain.tower_forward_train(x.astype(np.float64), tp)
        for blk in range(4, 8):
            want = cache[blk]["z"]
            z = got["z%d_%d" % (view, blk)].reshape(want.shape)
            scale = float(np.abs(want).max())
            err = float(np.abs(z - want).max())
            print("view %d block %d (%dx%d): z max err %.3g (largest magnitude %.3g)" % (view, blk + 1, want.shape[1], want.shape[2], err, scale))
            if not err <= 1e-4 * scale:
                bad.append((view, blk + 1, err, scale))
    assert not bad, bad
