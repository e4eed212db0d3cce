#!/usr/bin/env python
"""Timing of the alignment DTW: per-pair asr_dtw_dev (Engine.dtw) against one asr_dtw_batch_dev call
(Engine.dtw_batch), and the audio2sheet_align driver split into its stages.  One leg per process:

    python tools/bench_align.py --leg a    # 64 pairs 2000x2000: 64 sequential dtw calls vs one dtw_batch
    python tools/bench_align.py --leg b    # one 3000x3000 and one 12000x4000 pair, old vs new
    python tools/bench_align.py --leg c    # one 8000x8000 pair (above the LDS cap: global-ring wavefront)
    python tools/bench_align.py --leg d    # driver on 64 synthetic pieces: slicing + embedding, DTW, host post
                                           # (trained weights), mean |pixel error| of baseline and pydtw

Every leg checks that both paths return the same min_dist and path, and prints one JSON line (also written to
--out).  Times are wall clock of the Python call after one warm-up call (codes upload, paths download included),
median of --reps.  cells/s = sum R*C / time; per diagonal = time / (R+C-1) of the largest pair (the wavefront's
serial length).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _codes(rng, n_a, n_b):
    base = rng.standard_normal((max(n_a, n_b), 32))
    a = base[np.linspace(0, len(base) - 1, n_a).astype(int)]
    b = base[np.linspace(0, len(base) - 1, n_b).astype(int)] + 0.4 * rng.standard_normal((n_b, 32))
    f = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return f(a), f(b)


def _median_time(fn, reps):
    fn()                                           # warm-up: workspace growth, code objects
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def _old_vs_new(eng, pairs, reps):
    old = lambda: [eng.dtw(a, b, want_dists=False) for a, b in pairs]
    new = lambda: eng.dtw_batch(pairs)
    r_old, r_new = old(), new()
    for x, y in zip(r_old, r_new):
        assert x[0] == y[0] and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3]), "old and new paths differ"
    t_old, t_new = _median_time(old, reps), _median_time(new, reps)
    cells = float(sum(len(a) * len(b) for a, b in pairs))
    diags = max(len(a) + len(b) - 1 for a, b in pairs)
    return {"pairs": len(pairs), "shape": [len(pairs[0][0]), len(pairs[0][1])], "cells": cells,
            "old_s": t_old, "new_s": t_new, "speedup": t_old / t_new,
            "old_cells_per_s": cells / t_old, "new_cells_per_s": cells / t_new,
            "old_us_per_diagonal": 1e6 * t_old / (len(pairs) * diags),      # the old path runs the pairs one by one
            "new_us_per_diagonal": 1e6 * t_new / diags}


def leg_d(eng, n_pieces, reps):
    from audio_sheet_retrieval_amd import alignment as al, audio2sheet_align as drv
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.data_pools import AudioScoreRetrievalPool
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        eng.set_params([z["p%02d" % i] for i in range(97)])
    images, specs, o2c_maps = synth_data.synth_pieces(n_pieces)
    pool = AudioScoreRetrievalPool(eng, images, specs, o2c_maps, shuffle=False)
    out = {"pieces": n_pieces}
    t_embed = _median_time(lambda: drv.embed_pieces(eng, pool, 10, 2), reps)
    pieces = drv.embed_pieces(eng, pool, 10, 2)
    out["windows_sheet"] = int(sum(len(p["sheet_idxs"]) for p in pieces))
    out["windows_spec"] = int(sum(len(p["spec_idxs"]) for p in pieces))
    out["slice_embed_s"] = t_embed
    pairs = [(p["img_codes"], p["spec_codes"]) for p in pieces]
    out["dtw_cells"] = float(sum(len(a) * len(b) for a, b in pairs))
    out["dtw_batch_s"] = _median_time(lambda: al.dtw_by_dist_codes_batch(eng, pairs, first=True), reps)
    out["dtw_per_piece_old_s"] = _median_time(lambda: [al.dtw_by_dist_codes(eng, a, b) for a, b in pairs], 1)
    for by in ("baseline", "pydtw"):
        t0 = time.perf_counter()
        res = al.compute_alignments(eng, [(p["img_codes"], p["spec_codes"], p["sheet_idxs"], p["spec_idxs"])
                                          for p in pieces], by)
        t1 = time.perf_counter()
        errs = [al.estimate_alignment_error(o[0][:, 1], o[0][:, 0], m) for (m, _), o in zip(res, o2c_maps)]
        t2 = time.perf_counter()
        out[by + "_compute_alignments_s"] = t1 - t0
        out[by + "_error_estimate_s"] = t2 - t1
        out[by + "_mean_abs_px_error"] = float(np.mean(np.abs(np.concatenate(errs))))
        out[by + "_median_abs_px_error"] = float(np.median(np.abs(np.concatenate(errs))))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--leg", choices=["a", "b", "c", "d"], required=True)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--pieces", type=int, default=64)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    from audio_sheet_retrieval_amd import _lib
    eng = _lib.Engine("mutopia_ccal_cont")
    rng = np.random.default_rng(9)
    if args.leg == "a":
        res = _old_vs_new(eng, [_codes(rng, 2000, 2000) for _ in range(64)], args.reps)
    elif args.leg == "b":
        res = {"3000x3000": _old_vs_new(eng, [_codes(rng, 3000, 3000)], args.reps),
               "12000x4000": _old_vs_new(eng, [_codes(rng, 12000, 4000)], args.reps)}
    elif args.leg == "c":
        res = _old_vs_new(eng, [_codes(rng, 8000, 8000)], args.reps)
    else:
        res = leg_d(eng, args.pieces, args.reps)
    eng.close()
    line = json.dumps({"leg": args.leg, "result": res}, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
