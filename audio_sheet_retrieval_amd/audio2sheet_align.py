#!/usr/bin/env python
"""Audio-to-sheet alignment of whole test pieces (the paper's third experiment).  Command line of the reference's
audio2sheet_align.py (:27-40):

    python -m audio_sheet_retrieval_amd.audio2sheet_align --model models/mutopia_ccal_cont.py --data synthetic:16 \
        --train_split splits/all_split.yaml --config exp_configs/mutopia_full_aug.yaml \
        --estimate_UV --align_by pydtw [--step_sheet 10] [--step_spec 2]

Per piece (reference :80-172): sheet windows every --step_sheet pixels and spectrogram windows every --step_spec frames
at centred np.linspace positions; both towers embed them; the codes are aligned by a straight line (baseline) or DTW
(pydtw); the interpolated frame -> x mapping gives one pixel error per annotated onset.  The per-piece errors are dumped
to alignment_res_<tag>_<align_by>.pkl next to the parameters (:228-233).

Here the strips of all pieces stay resident on the device (AudioScoreRetrievalPool), the windows are cut there
(asr_slice_windows_dev), all windows of all pieces go through each tower in one call, and pydtw aligns every piece
in one asr_dtw_batch_dev call.  Plots (--plots) and audio decoding (--real_audio) are not part of this
implementation.
"""
import argparse
import os
import pickle

import numpy as np

from . import _lib, network
from .alignment import compute_alignments, estimate_alignment_error
from .config.settings import EXP_ROOT
from .retrieval_wrapper import load_params
from .run_train import compile_tag, select_model
from .utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool


def _arguments(argv):
    p = argparse.ArgumentParser(description="Align audio to sheet music for every test piece.")
    p.add_argument("--model", help="model definition, e.g. models/mutopia_ccal_cont.py",
                   default="models/mutopia_ccal_cont.py")
    p.add_argument("--data", type=str, default="synthetic", help="test pieces ('synthetic[:n_pieces]')")
    p.add_argument("--estimate_UV", action="store_true", help="use the parameters written by refine_cca")
    p.add_argument("--step_sheet", type=int, default=10, help="pixels between sheet windows")
    p.add_argument("--step_spec", type=int, default=2, help="frames between spectrogram windows")
    p.add_argument("--real_audio", action="store_true", help="(audio decoding is not part of this implementation)")
    p.add_argument("--align_by", type=str, default="baseline", choices=["baseline", "pydtw"])
    p.add_argument("--plots", action="store_true", help="(plots are not part of this implementation)")
    p.add_argument("--dump_alignment", action="store_true", help="(accepted; the errors are always dumped)")
    p.add_argument("--train_split", type=str, default=None)
    p.add_argument("--config", type=str, default=None)
    p.add_argument("--seed", type=int, default=23)
    return p.parse_args(argv)


def sample_points(length, win, step):
    """window centres every `step` along an axis of `length` (:112-120): np.linspace from win//2 to length - win//2,
    length // step of them -> (centres int32, half width); window k is [centres[k] - half, centres[k] + half)"""
    half = win // 2
    return np.linspace(half, length - half, length // step).astype(np.int32), half


def result_file(param_file, align_by):
    """the reference's dump name (:229-230)"""
    return param_file.replace("params_", "alignment_res_").replace(".pkl", "_%s.pkl") % align_by


def select_pieces(data_name, seed=23):
    """{'names', 'images', 'specs', 'o2c_maps'} of the test pieces.  'synthetic[:n]' (default 16): synthetic whole
    pieces (utils/synth_data.synth_pieces); MSMD (`mutopia`) needs the msmd package, which is not part of this
    implementation."""
    name = str(data_name)
    if not name.startswith("synthetic"):
        raise SystemExit("--data %s: only synthetic pieces are available here (MSMD loading is outside the accelerated "
                         "path); use --data synthetic[:n_pieces]" % name)
    from .utils import synth_data
    n = int(name.split(":")[1]) if ":" in name else 16
    images, specs, o2c_maps = synth_data.synth_pieces(n, seed)
    return dict(names=["synthetic_%03d" % i for i in range(n)], images=images, specs=specs, o2c_maps=o2c_maps)


def embed_pieces(engine, pool, sheet_step, spec_step):
    """Windows of every piece cut on the device and embedded with one call per tower -> one dict per piece with
    img_codes, spec_codes, sheet_idxs, spec_idxs (reference :110-147, which slices on the host and embeds one window
    per call)."""
    win_h, win_w = pool.sheet_dim
    bins, ctx = pool.spec_dim
    plan = []
    for i, sheet in enumerate(pool.images):
        spec = pool.specs[i][0]
        spec_idxs, o0 = sample_points(spec.shape[1], ctx, spec_step)
        sheet_idxs, c0 = sample_points(sheet.shape[1], win_w, sheet_step)
        r0 = sheet.shape[0] // 2 - win_h // 2
        plan.append((sheet_idxs, c0, r0, spec_idxs, o0))
    n1 = sum(len(p[0]) for p in plan)
    n2 = sum(len(p[3]) for p in plan)
    d_win1 = engine.alloc(n1 * win_h * win_w * 4)
    d_win2 = engine.alloc(n2 * bins * ctx * 4)
    d_codes1, d_codes2 = engine.alloc(n1 * 32 * 4), engine.alloc(n2 * 32 * 4)
    try:
        o1 = o2 = 0
        for i, (sheet_idxs, c0, r0, spec_idxs, o0) in enumerate(plan):
            rows, T = pool.images[i].shape
            engine.slice_windows_dev(pool._d_img.offset(pool._img_off[i] * 4), rows, T, r0, win_h, win_w,
                                     sheet_idxs - c0, d_win1.offset(o1 * win_h * win_w * 4))
            spec = pool.specs[i][0]
            engine.slice_windows_dev(pool._d_spec.offset(pool._spec_off[i][0] * 4), bins, spec.shape[1], 0, bins, ctx,
                                     spec_idxs - o0, d_win2.offset(o2 * bins * ctx * 4))
            o1 += len(sheet_idxs)
            o2 += len(spec_idxs)
        if (engine.cfg.h1, engine.cfg.w1) != (win_h, win_w):
            engine.set_input_size(1, win_h, win_w)
        if (engine.cfg.h2, engine.cfg.w2) != (bins, ctx):
            engine.set_input_size(2, bins, ctx)
        engine.embed_view1_dev(d_win1.ptr, _lib.IN_F32_RAW, n1, d_codes1.ptr)
        engine.embed_view2_dev(d_win2.ptr, n2, d_codes2.ptr)
        codes1 = d_codes1.download((n1, 32), np.float32)
        codes2 = d_codes2.download((n2, 32), np.float32)
    finally:
        for b in (d_win1, d_win2, d_codes1, d_codes2):
            b.free()
    out, o1, o2 = [], 0, 0
    for sheet_idxs, _, _, spec_idxs, _ in plan:
        out.append(dict(img_codes=codes1[o1:o1 + len(sheet_idxs)], spec_codes=codes2[o2:o2 + len(spec_idxs)],
                        sheet_idxs=sheet_idxs, spec_idxs=spec_idxs))
        o1 += len(sheet_idxs)
        o2 += len(spec_idxs)
    return out


def align_pieces(engine, pool, align_by, sheet_step=10, spec_step=2):
    """-> (per-piece windows + codes, per-piece (mapping, details), per-piece pixel errors)"""
    pieces = embed_pieces(engine, pool, sheet_step, spec_step)
    results = compute_alignments(engine, [(p["img_codes"], p["spec_codes"], p["sheet_idxs"], p["spec_idxs"])
                                          for p in pieces], align_by)
    errors = []
    for i, (mapping, _) in enumerate(results):
        o2c = np.asarray(pool.o2c_maps[i][0])
        errors.append(estimate_alignment_error(o2c[:, 1], o2c[:, 0], mapping))
    return pieces, results, errors


def load_network(model_path, estimate_UV, train_split, config):
    """the model's parameters from EXP_ROOT/<EXP_NAME>[_est_UV]/params[_<tag>].pkl on an engine -> (engine, param
    file) - what the reference's drivers load (:55-66; audio_sheet_server.py:600-608)"""
    model, _ = select_model(model_path)
    layers = model.build_model(show_model=False)
    tag = compile_tag(train_split, config)
    print("Experimental Tag:", tag)
    folder = model.EXP_NAME + ("_est_UV" if estimate_UV else "")
    param_file = os.path.join(EXP_ROOT, folder, "params.pkl" if tag is None else "params_%s.pkl" % tag)
    params = load_params(param_file)
    if isinstance(params[0], list):            # very old dumps hold one full list per layer handle
        params = params[-1]
    network.set_all_param_values(layers, params)
    view1, view2, latent1, _ = layers
    engine = network.function([view1.input_var, view2.input_var],
                              network.get_output(latent1, deterministic=True)).engine
    return engine, param_file


def main(argv=None):
    args = _arguments(argv)
    if args.plots:
        raise SystemExit("--plots: plotting is not part of this implementation")
    if args.real_audio:
        raise SystemExit("--real_audio: audio decoding is not part of this implementation")
    engine, param_file = load_network(args.model, args.estimate_UV, args.train_split, args.config)

    data = select_pieces(args.data, args.seed)
    pool = AudioScoreRetrievalPool(engine, data["images"], data["specs"], data["o2c_maps"],
                                   data_augmentation=dict(NO_AUGMENT), shuffle=False)
    _, _, errors = align_pieces(engine, pool, args.align_by, args.step_sheet, args.step_spec)
    piece_pxl_errors = {}
    for name, pxl_errors in zip(data["names"], errors):
        abs_err = np.abs(pxl_errors)
        print("\nTarget Piece: %s" % name)
        print("Mean Error:   %.3f" % np.mean(abs_err))
        print("Median Error: %.3f" % np.median(abs_err))
        print("Max Error:    %.3f" % np.max(abs_err))
        piece_pxl_errors[name] = pxl_errors
    res_file = result_file(param_file, args.align_by)
    with open(res_file, "wb") as fp:
        pickle.dump(piece_pxl_errors, fp)
    print("\nalignment errors of %d pieces written to %s" % (len(piece_pxl_errors), res_file))
    return piece_pxl_errors


if __name__ == "__main__":
    main()
