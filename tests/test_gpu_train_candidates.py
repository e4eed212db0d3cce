"""GPU: EVERY schedule the training step's tuner can pick (asr_train_begin, tune_train_plans), one at a time, against
float64 - not only the one that won the timing on the day.

asr_debug_train_candidate runs candidate `index` of the tuner's own list for a 3x3 block (forward convolution, data
gradient, weight gradient) alone, through the production launcher, from outputs, BatchNorm statistics table and partial
sums pre-filled with NaN.  The sweep below walks every block 1..7 of both towers, every kind and every index until the
list ends, and compares
    z          with oracle.network.conv2d_flip_nhwc_f64,
    dx, dW     with oracle.train.conv_bwd_nhwc on float64 arrays,
    mu/inv_std (the convolution's own statistics rows, finished as train_forward_block finishes them, eps 1e-4) with the
               float64 z.
Inputs have a non-zero mean so that sums do not cancel: x = elu(0.8 randn + 0.3), dz = 0.05 randn + 0.02; the weights
are synth_params(seed=1, trained_like=True).  On these inputs the FLOAT32 oracle stays within 2.5e-5 of the float64
one relative to each tensor's maximum (test_inputs_are_well_conditioned; measured worst 2.6e-6), so the bars measure
the kernels and not the inputs.

Geometries (sheet / spectrogram, batch):
    tiny  20x36 / 16x24, 2    the last blocks see 2x4 and 2x3 maps: a single M-tile, waves without work whose
                              statistics rows must still be written (zeros) - stats_rows > work items
    odd   106x74 / 54x38, 5   53x37, 27x19 and 13x9 maps: M-tiles straddle strips and images, ragged last M-tile, ragged
                              F(4x4) tile row and column; run again under the first-maximum pooling rule (forward only),
                              which brings the forward F(4x4) builds into the lists
    even  48x64 / 32x24, 3    every tile full; afterwards one train_step on this engine and one on a fresh engine
    long  64x48 / 46x21, 320  five samples repeated round-robin; only the blocks with an LDS-patch variant, that family
                              and the model plan: each workgroup runs three or more consecutive regions (its patch
                              buffers are reused), asserted as work items > 2 x workgroups

Bars (the project's existing ones): z and dx within 1e-4 max(1, max|ref|) (test_train_forward_and_side_effects_match_oracle),
dW within 1e-4 of the tensor's maximum (test_gpu_train_routed.py), mu within 1e-4 absolute,
inv_std within 1e-4 relative; nothing NaN.  Families: direct (kind 2: the direct-form weight gradients), winog (global-A
F(2x2)), wino (LDS-patch F(2x2); kind 2: the Winograd-domain weight gradient), wino4 (F(4x4)).

`long`: not every tiling can give a workgroup three regions at batch 320 - the largest regions cover a whole 32x24 or
23x10 map, one region per sample, 320 regions on 160 or 320 workgroups.  Those tilings run and are checked like the
others and are printed; asserted is that every list with LDS-patch candidates holds tilings with such runs and that
every LDS-patch kernel build gets them in one of the two towers.

Measured on an MI355X, worst error over all geometries and both towers as a fraction of its bar (the bars stay):
    family  kind   z / dx    mu       inv_std  dW
    winog   fwd    0.0031    0.0017   0.0030
    winog   dgrad  0.0012
    wino    fwd    0.0023    0.0003   0.0011
    wino    dgrad  0.00044
    wino4   fwd    0.072     0.0025   0.0045            (first-maximum rule only)
    wino4   dgrad  0.017
    direct  wgrad                              0.0019
    wino    wgrad                              0.0026
No launcher refused a candidate.  Float32 oracle against float64 on the same inputs: worst 2.6e-6 of a tensor's maximum.
Deliberate breaks (not committed) fail with NaN: the zero-row store of idle global-A waves skipped - mu and inv_std of
every global-A forward candidate of `tiny` and of the small maps of `odd`; the last M-tile dropped from the row-major
global-A walk - z and dx of every such candidate.
"""
import functools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL = "mutopia_ccal_cont"
KINDS = ("fwd", "dgrad", "wgrad")
# geometry: (sheet, spectrogram, distinct samples, repeats)
GEOMETRIES = {"tiny": ((20, 36), (16, 24), 2, 1), "odd": ((106, 74), (54, 38), 5, 1), "even": ((48, 64), (32, 24), 3, 1),
              "long": ((64, 48), (46, 21), 5, 64)}
_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _environment():
    """model plans, no timing (the lists do not depend on it); the engines of the module are closed at its end"""
    mp = pytest.MonkeyPatch()
    mp.setenv("ASR_TRAIN_TUNE", "0")
    mp.setenv("ASR_AUTOTUNE", "0")
    mp.delenv("ASR_TUNE_CACHE", raising=False)
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _sweep.cache_clear()
    _reference.cache_clear()
    mp.undo()


@functools.lru_cache(maxsize=None)
def _params():
    from audio_sheet_retrieval_amd.utils import synth_data
    from oracle import network as onet
    return synth_data.synth_params(onet.param_shapes(MODEL), seed=1, trained_like=True)


def _engine(geometry, rule="all"):
    from audio_sheet_retrieval_amd import _lib
    if (geometry, rule) not in _ENGINES:
        s1, s2, distinct, repeat = GEOMETRIES[geometry]
        eng = _lib.Engine(MODEL, h1=s1[0], w1=s1[1], h2=s2[0], w2=s2[1], pool_ties=rule)
        eng.set_params(_params())
        eng.train_begin(distinct * repeat)
        _ENGINES[(geometry, rule)] = eng
    return _ENGINES[(geometry, rule)]


def _inputs(geometry, view, block, shape):
    """x (distinct,H,W,cin) and dz (distinct,H,W,cout) of one block, float32, non-zero mean"""
    h, w, cin, cout = shape
    distinct = GEOMETRIES[geometry][2]
    rng = np.random.default_rng([sorted(GEOMETRIES).index(geometry), view, block])
    x = 0.8 * rng.standard_normal((distinct, h, w, cin)) + 0.3
    x = np.where(x > 0, x, np.expm1(np.minimum(x, 0))).astype(np.float32)
    dz = (0.05 * rng.standard_normal((distinct, h, w, cout)) + 0.02).astype(np.float32)
    return x, dz


@functools.lru_cache(maxsize=None)
def _reference(geometry, view, block, shape):
    """inputs and the float64 answers for the distinct samples of one block: computed once, read-only"""
    from oracle import network as onet, train as otrain
    x, dz = _inputs(geometry, view, block, shape)
    W = _params()[45 * (view - 1) + 5 * block].astype(np.float64)
    assert W.shape == (shape[3], shape[2], 3, 3)
    z = onet.conv2d_flip_nhwc_f64(x.astype(np.float64), W)
    dx, dW = otrain.conv_bwd_nhwc(x.astype(np.float64), W, dz.astype(np.float64))
    zf = z.reshape(-1, shape[3])
    mu = zf.mean(axis=0)
    inv_std = 1.0 / np.sqrt(zf.var(axis=0) + 1e-4)
    ref = dict(x=x, dz=dz, W=W, z=z, dx=dx, dW=dW, mu=mu, inv_std=inv_std)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _list_length(eng, view, block, kind, n):
    """the list ends where the aid says so: ASR_ERR_INVALID, "... has <length> candidates" """
    from audio_sheet_retrieval_amd import _lib
    with pytest.raises(_lib.AsrError) as ei:
        eng.debug_train_candidate(view, block, kind, 1 << 20, batch=n)
    assert ei.value.code == _lib.ASR_ERR_INVALID, ei.value
    m = re.search(r"has (\d+) candidates", str(ei.value))
    assert m, ei.value
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def _sweep(geometry, view, rule="all", kinds=(0, 1, 2)):
    """Every candidate of every list of one tower.  Returns (records, failures): a record per candidate that ran -
    dict(block, kind, index, family, tile, desc, launched, err: {quantity: error as a fraction of its bar}, ...)."""
    eng = _engine(geometry, rule)
    _, _, distinct, repeat = GEOMETRIES[geometry]
    n = distinct * repeat
    rep = lambda a: a if repeat == 1 else np.ascontiguousarray(np.tile(a, (repeat, 1, 1, 1)))   # samples 0 1 2 3 4 0 1 ...
    records, failures = [], []
    for block in range(1, 8):
        shape = eng.debug_train_candidate(view, block, 0, 0, batch=n)["shape"]
        lists = {kind: [eng.debug_train_candidate(view, block, kind, i, batch=n)
                        for i in range(_list_length(eng, view, block, kind, n))] for kind in kinds}
        # `long`: the LDS-patch family and the model's plan, on the blocks that have the family in either direction
        if geometry == "long" and not any(d["family"] == "wino" for kind in (0, 1) for d in lists[kind]):
            continue
        for kind in kinds:
            length = len(lists[kind])
            if geometry == "long":
                todo = [i for i, d in enumerate(lists[kind]) if i == 0 or (kind != 2 and d["family"] == "wino")]
            else:
                todo = list(range(length))
            ref = _reference(geometry, view, block, shape)
            x, dz = rep(ref["x"]), rep(ref["dz"])
            for i in todo:
                r = eng.debug_train_candidate(view, block, kind, i, x if kind != 1 else dz, dz if kind == 2 else None)
                rec = dict(block=block, kind=kind, index=i, list_length=length,
                           **{k: r[k] for k in ("family", "tile", "desc", "launched", "work_items", "workgroups", "variant")})
                tag = "%s view %d conv%d %s [%d/%d] %s" % (geometry, view, block + 1, KINDS[kind], i, length, r["desc"])
                records.append(rec)
                if not r["launched"]:
                    print(tag + ": REFUSED by its launcher (not counted)")
                    continue
                out = r["out"].astype(np.float64)
                err = {}
                if kind == 2:
                    want = ref["dW"] * repeat
                    err["dW"] = np.abs(out - want).max() / (1e-4 * np.abs(want).max())
                else:
                    want = ref["z"] if kind == 0 else ref["dx"]
                    d = np.abs(out.reshape((repeat,) + want.shape) - want[None]).max()
                    err["z" if kind == 0 else "dx"] = d / (1e-4 * max(1.0, np.abs(want).max()))
                if kind == 0:
                    rec["stats_rows"] = r["stats_rows"]
                    if r["stats_rows"] > 0:
                        err["mu"] = np.abs(r["mu"] - ref["mu"]).max() / 1e-4
                        err["inv_std"] = np.abs(r["inv_std"] / ref["inv_std"] - 1.0).max() / 1e-4
                rec["err"] = err
                print(tag + ": " + ", ".join("%s %.3g" % kv for kv in err.items()) +
                      (", %d rows / %d items / %d workgroups" % (r["stats_rows"], r["work_items"], r["workgroups"])
                       if kind == 0 else ""))
                for q, e in err.items():
                    if not e <= 1.0:                   # (NaN fails too: an element or a statistics row nobody wrote)
                        failures.append("%s: %s at %.3g of its bar" % (tag, q, e))
    return records, failures


def _checked(records):
    return [r for r in records if r["launched"] and "err" in r]


def _worst(records):
    worst = {}
    for r in _checked(records):
        for q, e in r["err"].items():
            key = (r["family"], KINDS[r["kind"]], q)
            worst[key] = max(worst.get(key, 0.0), e) if e == e else float("nan")
    return worst


def _assert_not_passing_on_nothing(geometry, view, records, kinds=(0, 1, 2)):
    checked = _checked(records)
    for block in range(1, 8):
        for kind in kinds:
            listed = [r for r in records if r["block"] == block and r["kind"] == kind]
            if geometry == "long" and not listed:
                continue                                  # (blocks without the LDS-patch family are not this geometry's)
            done = [r for r in checked if r["block"] == block and r["kind"] == kind]
            assert done, "view %d conv%d %s: no candidate was checked" % (view, block + 1, KINDS[kind])
            for fam in {r["family"] for r in listed}:
                assert any(r["family"] == fam for r in done), \
                    "view %d conv%d %s: no %s candidate launched" % (view, block + 1, KINDS[kind], fam)
    if geometry == "long":
        assert any(r["family"] == "wino" and r["kind"] == 0 for r in checked), "no LDS-patch forward candidate ran"


SWEEPS = [(g, v) for g in ("tiny", "odd", "even", "long") for v in (1, 2)]


@pytest.mark.parametrize("geometry,view", SWEEPS, ids=["%s-view%d" % gv for gv in SWEEPS])
def test_every_candidate_matches_float64(geometry, view):
    records, failures = _sweep(geometry, view)
    for key, e in sorted(_worst(records).items()):
        print("worst %s view %d  %-6s %-5s %-7s %.3g of its bar" % ((geometry, view) + key + (e,)))
    assert not failures, "\n".join(failures)
    _assert_not_passing_on_nothing(geometry, view, records)
    fwd = [r for r in _checked(records) if r["kind"] == 0]
    if geometry == "tiny":
        # waves (workgroups) without an M-tile or a region: their rows are in the table the launcher reported
        idle = [r["desc"] for r in fwd if r["stats_rows"] > r["work_items"]]
        assert idle, "view %d: no forward candidate with more statistics rows than work items" % view
    if geometry == "long":
        # Runs of three or more regions per workgroup (work items > 2 x workgroups).  Not every tiling can have them at
        # this geometry's batch: the largest regions cover a whole 32x24 or 23x10 map, one region per sample, 320 regions
        # on 160 or 320 workgroups.  Those tilings are printed; every list with LDS-patch candidates must hold tilings
        # that do get such runs, and every kernel BUILD must get them in one of the towers
        # (test_the_long_runs_reuse_the_patch_buffers_of_every_build).
        lds = [r for r in _checked(records) if r["family"] == "wino" and r["kind"] != 2]
        for r in lds:
            if not r["work_items"] > 2 * r["workgroups"]:
                print("long view %d conv%d %s %s: %d regions on %d workgroups - no run of three" % (
                    view, r["block"] + 1, KINDS[r["kind"]], r["desc"], r["work_items"], r["workgroups"]))
        for key in sorted({(r["block"], r["kind"]) for r in lds}):
            runs = [r for r in lds if (r["block"], r["kind"]) == key and r["work_items"] > 2 * r["workgroups"]]
            assert runs, "view %d conv%d %s: no LDS-patch tiling gives a workgroup three regions" % (
                view, key[0] + 1, KINDS[key[1]])


def test_the_long_runs_reuse_the_patch_buffers_of_every_build():
    """every LDS-patch kernel build that the `long` lists hold was checked, per direction, on at least one tiling
    whose workgroups run three or more consecutive regions"""
    lds = [r for view in (1, 2) for r in _checked(_sweep("long", view)[0]) if r["family"] == "wino" and r["kind"] != 2]
    builds = sorted({(r["kind"], r["variant"]) for r in lds})
    assert len(builds) >= 4, builds
    for kind, variant in builds:
        runs = [r for r in lds if (r["kind"], r["variant"]) == (kind, variant) and r["work_items"] > 2 * r["workgroups"]]
        print("wino#%d %s: %d tilings with runs of three or more regions" % (variant, KINDS[kind], len(runs)))
        assert runs, "wino#%d %s: no tiling gives a workgroup three regions" % (variant, KINDS[kind])


@pytest.mark.parametrize("view", [1, 2])
def test_forward_candidates_under_the_first_maximum_rule(view):
    """ASR_POOL_TIES_FIRST puts the RAW F(4x4) builds into the FORWARD lists"""
    records, failures = _sweep("odd", view, "first", (0,))
    for key, e in sorted(_worst(records).items()):
        print("worst odd(first) view %d  %-6s %-5s %-7s %.3g of its bar" % ((view,) + key + (e,)))
    assert not failures, "\n".join(failures)
    _assert_not_passing_on_nothing("odd", view, records, (0,))
    assert any(r["family"] == "wino4" for r in _checked(records)), "no forward F(4x4) candidate in view %d" % view


def test_the_odd_runs_cover_every_family_and_tile_order():
    records = []
    for view in (1, 2):
        records += _checked(_sweep("odd", view)[0]) + _checked(_sweep("odd", view, "first", (0,))[0])
    families = {r["family"] for r in records}
    assert families == {"direct", "winog", "wino", "wino4"}, families
    orders = {r["tile"][0] for r in records if r["family"] == "winog"}
    assert {1, 2} <= orders, "global-A tile orders checked: strips of %s tile rows" % sorted(orders)
    tilings = {}
    for r in records:
        if r["kind"] == 2:
            tilings.setdefault((r["block"], r["desc"].split(",")[0]), None)
    per_block = {}
    for block, _ in tilings:
        per_block[block] = per_block.get(block, 0) + 1
    assert max(per_block.values()) > 1, "every weight-gradient list holds one tiling only: %s" % per_block


def test_training_is_unaffected_by_the_aid():
    """one train_step after the sweeps of the `even` engine and one on an engine that never called the aid: same loss
    (2e-6, the first-step bar of test_training_schedule_switches_compute_the_same_step); gradient slots all zero"""
    from audio_sheet_retrieval_amd import _lib
    for view in (1, 2):
        _sweep("even", view)
    eng = _engine("even")
    s1, s2, n, _ = GEOMETRIES["even"]
    for i in range(90):
        g = eng.debug_train_tensor("grad", index=i)
        assert not g.any(), "gradient slot %d is not zero after the sweep" % i
    rng = np.random.default_rng(3)
    x1 = rng.random((n, 1) + s1).astype(np.float32)
    x2 = (2 * rng.random((n, 1) + s2)).astype(np.float32)
    loss, _ = eng.train_step(x1, x2, lr=0.002)
    fresh = _lib.Engine(MODEL, h1=s1[0], w1=s1[1], h2=s2[0], w2=s2[1])
    fresh.set_params(_params())
    fresh.train_begin(n)
    want, _ = fresh.train_step(x1, x2, lr=0.002)
    fresh.close()
    print("loss after the sweeps %.8g, on a fresh engine %.8g" % (loss, want))
    assert np.isfinite(want) and abs(loss - want) <= 2e-6, (loss, want)


def test_inputs_are_well_conditioned():
    """the float32 oracle on the same inputs stays within 2.5e-5 of the float64 one, relative to each tensor's maximum:
    the 1e-4 bars measure the kernels, not how the inputs condition the sums"""
    from oracle import network as onet, train as otrain
    worst = 0.0
    for geometry in GEOMETRIES:
        eng = _engine(geometry)
        n = GEOMETRIES[geometry][2] * GEOMETRIES[geometry][3]
        for view in (1, 2):
            for block in range(1, 8):
                shape = eng.debug_train_candidate(view, block, 0, 0, batch=n)["shape"]
                ref = _reference(geometry, view, block, shape)
                W32 = ref["W"].astype(np.float32)
                z = onet.conv2d_flip_nhwc(ref["x"], W32)
                dx, dW = otrain.conv_bwd_nhwc(ref["x"], W32, ref["dz"])
                for name, got in (("z", z), ("dx", dx), ("dW", dW)):
                    e = float(np.abs(got - ref[name]).max() / np.abs(ref[name]).max())
                    worst = max(worst, e)
                    assert e <= 2.5e-5, (geometry, view, block, name, e)
    print("float32 oracle against float64, worst over all blocks: %.3g of the tensor's maximum" % worst)
