"""GPU: every path of the producer wave of conv3x3_wino4s - the M-tile's border masks ANDed onto the patch, the interior
M-tile that needs none, lanes past the end of the tile list, M-tiles that span two images - against the oracle.

F(4x4) forced where a block has it, block 1 materialised, a first different batch run beforehand (a V buffer slot the
second pass did not write would keep the first batch's values).  Blocks 5-8 of both towers are pinned to their
conv3x3_wino4s build through the test's own tune cache - under ASR_CONV_WINO4=1 the tuner could otherwise pick the
one-n-tile form conv3x3_wino4g on maps this small - and the test asserts from that cache that they ran it.  The sizes
are the smallest that reach each path:

"interior": sheet 112x304, two samples.  Blocks 5/6 see 28x76 maps: 7 x 19 tiles, and M-tile 6 = tiles 96..111 is tile
    row 5, columns 1..16 - no lane touches the image border, the only geometry here in which the producer takes the
    path without masks (it needs 18 tile columns; the models' own maps have 13 at most).  Blocks 7/8 see 14x38: border
    path, last tile row two pixels high, last tile column two pixels wide.
"ragged": sheet 88x104, three samples.  Blocks 5/6 see 22x26: 6 x 7 = 42 tiles per image, 126 in all - the last M-tile
    has 14 live lanes, tiles 32..47 span images 0 and 1, the last tile row and column are two pixels deep.  Blocks 7/8
    see 11x13.
"bench": the benchmark's 160x200 / 92x42 (40x50, 20x25 and 23x10, 11x5 maps), two samples.
The spectrogram keeps its default size in the first two.

Bar: that of tests/test_gpu_wino4_epilogue.py - activations of blocks 5-8 of both towers within 1e-4 of the layer's
largest magnitude.

Training: the RAW builds run the same producer.  One step's forward pass on four samples (48x64 / 32x24: blocks 5/6 on
12x16 maps, 48 tiles whose M-tiles span images; blocks 7/8 on 6x8) with the RAW F(4x4) builds forced for the forward
convolutions; the raw outputs z of blocks 5-8 of both towers, read as tests/test_gpu_train_routed.py reads them, within
1e-4 of the layer's largest magnitude of the float64 oracle's.  The switch that forces them is read once per process,
so that step runs in a process of its own.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL = "mutopia_ccal_cont"
# name: (sheet size, spectrogram size, samples)
GEOMETRIES = {"interior": ((112, 304), (92, 42), 2), "ragged": ((88, 104), (92, 42), 3), "bench": ((160, 200), (92, 42), 2)}


def _block_outputs(onet, x, tparams):
    _, _, cache = onet.tower_forward(x, tparams, True, return_cache=True)
    outs = []
    for blk in range(8):
        a = cache[blk]["a"]
        outs.append(onet.maxpool2_nhwc(a) if blk in (1, 3, 5, 7) else a)
    return outs


@pytest.fixture(scope="module", params=sorted(GEOMETRIES))
def case(request):
    """Two different batches and the oracle's blocks 5-8 for the second one (computed once per geometry, read-only)."""
    from audio_sheet_retrieval_amd.utils import synth_data
    from oracle import network as onet
    shape1, shape2, n = GEOMETRIES[request.param]
    params = synth_data.synth_params(onet.param_shapes(MODEL), seed=1, trained_like=True)
    batches = []
    for seed in (5, 6):
        rng = np.random.default_rng(seed)
        sheet = rng.integers(0, 256, size=(n, 1) + shape1, dtype=np.uint8)
        spec = (3.0 * rng.random((n, 1) + shape2) ** 2).astype(np.float32)
        batches.append((sheet, spec))
    sheet, spec = batches[1]
    x = onet.prepare(sheet, MODEL)
    ref = {1: _block_outputs(onet, x, params[0:45])[4:], 2: _block_outputs(onet, spec, params[45:90])[4:]}
    for view in (1, 2):
        for a in ref[view]:
            a.setflags(write=False)
    return (shape1, shape2), n, params, batches, ref


# blocks 5-8 (tuner index b = 4..7) -> the conv3x3_wino4s entry of the library's F(4x4) table for that block
# (conv_wino4_kernels.hip, g_wino4: 4005 = 24 -> 48, 4006 = 48 -> 48 pooled, 4007 = 48 -> 48), tile 4 x 64, NI 16
WINO4S = {4: 4005, 5: 4006, 6: 4007, 7: 4006}


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


def test_producer_paths_match_the_oracle(case, monkeypatch, tmp_path):
    from audio_sheet_retrieval_amd import _lib
    ((h1, w1), (h2, w2)), n, params, batches, ref = case
    cache = tmp_path / "tune_cache.txt"
    monkeypatch.setenv("ASR_TUNE_ONLY", "wino4")
    monkeypatch.setenv("ASR_CONV_WINO4", "1")
    monkeypatch.setenv("ASR_FUSE1", "0")                # block 1 materialised, as in the epilogue's test
    monkeypatch.setenv("ASR_TUNE_CACHE", str(cache))    # its own
    # With ASR_CONV_WINO4=1 the one-n-tile form conv3x3_wino4g is a candidate too, and on maps this small either could
    # win the tuner's timing.  So blocks 5-8 of both towers are not left to it: the cache names conv3x3_wino4s for
    # them beforehand (the tuner takes a line that matches build, geometry and chunk, and appends one where none
    # does); the earlier blocks it times as usual.
    tag = _tune_tag(_lib.load_library())
    cache.write_text("".join("v2 %d 12 %d %d %d %d %d %d 4 64 16\n" % (tag, view, b, h >> (2 if b < 6 else 3), w >> (2 if b < 6 else 3), n, WINO4S[b])
                             for view, (h, w) in ((1, (h1, w1)), (2, (h2, w2))) for b in sorted(WINO4S)))
    eng = _lib.Engine(MODEL, h1=h1, w1=w1, h2=h2, w2=w2, max_chunk=n)
    eng.set_params(params)
    eng.embed_view1(batches[0][0], prepared=False)
    eng.embed_view2(batches[0][1])
    eng.embed_view1(batches[1][0], prepared=False)
    eng.embed_view2(batches[1][1])
    acts = {view: [eng.debug_activation(view, blk, n) for blk in range(4, 8)] for view in (1, 2)}
    eng.close()
    # which schedules ran: for blocks 5-8 the cache must still hold the one conv3x3_wino4s line per (tower, block) -
    # a line the tuner did not accept would have made it time the block and append its own pick
    picks = _cache_lines(cache)
    print("schedules (view, b): variant  " + "; ".join("(%d, %d): %s" % (k + (v,)) for k, v in sorted(picks.items())))
    for view in (1, 2):
        for b, variant in WINO4S.items():
            assert picks.get((view, b)) == [variant], "view %d block %d did not run conv3x3_wino4s: %s" % (view, b + 1, picks.get((view, b)))
    worst = []
    for view in (1, 2):
        for k, (want, got) in enumerate(zip(ref[view], acts[view])):
            assert got.shape == want.shape, (view, k + 5, got.shape, want.shape)
            scale = float(np.abs(want).max())
            err = float(np.abs(got - want).max())
            print("view %d block %d (%dx%d): max err %.3g (largest magnitude %.3g)" % (view, k + 5, want.shape[1], want.shape[2], err, scale))
            worst.append((err <= 1e-4 * scale, view, k + 5, err, scale))
    assert all(w[0] for w in worst), [w[1:] for w in worst if not w[0]]


_TRAIN_SCRIPT = r"""
import sys, numpy as np
from audio_sheet_retrieval_amd import _lib
from audio_sheet_retrieval_amd.utils import synth_data
from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
model, B, hw1, hw2 = "mutopia_ccal_cont", 4, (48, 64), (32, 24)
rng = np.random.default_rng(9)
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


def test_training_forward_through_the_raw_builds(tmp_path):
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
