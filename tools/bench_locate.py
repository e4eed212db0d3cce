#!/usr/bin/env python
"""Timing of excerpt localisation (piece_identification.locate_scores, asr_dtw_subseq_batch_dev).  Workload: 256
excerpts of 400 frames (4 seeded cuts of each of 64 synthetic pieces) x 5 candidates against the pieces' from_pool sheet
data base, trained weights.  One leg per process, each under its own time limit:

    python tools/bench_locate.py --leg route     # locate_scores against locate_scores_host (the same pairs aligned on
                                                 # the host), and the route's stages: vote, window embedding, DTW call
    python tools/bench_locate.py --leg kernel    # device time (library profile scopes, event timed) of the fused
                                                 # pass against the time Engine.dtw_batch(pairs, want_dists=False,
                                                 # want_path=False) needs merely to write the distances of the same
                                                 # cells; per-diagonal time of a single 180 x 2000 pair
    python tools/bench_locate.py --all --out profiles/r20_locate.json     # both legs, merged

Times are medians of --reps after one warm-up.  Every leg checks that the device route equals the host route.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_PIECES, CUTS, FRAMES, CANDS, STEP = 64, 4, 400, 5, 2
LEG_LIMIT_S = {"route": 420, "kernel": 240}


def _median(fn, reps, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), [float(min(ts)), float(max(ts))]


def _setup(eng):
    from audio_sheet_retrieval_amd import audio_sheet_server as drv, piece_identification as pid
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        eng.set_params([z["p%02d" % i] for i in range(97)])
    images, specs, o2c_maps = synth_data.synth_pieces(N_PIECES)
    pool = AudioScoreRetrievalPool(eng, images, specs, o2c_maps, data_augmentation=dict(NO_AUGMENT), shuffle=False)
    db = pid.EmbeddingDB.from_pool(eng, pool, 1, names=["p%03d" % i for i in range(N_PIECES)])
    excerpts = []
    for cut in range(CUTS):
        excerpts += drv.cut_excerpts(pool.specs, pool.o2c_maps, FRAMES, STEP, 42, 100 + cut)[0]
    return pool, db, excerpts, drv.pool_sheet_columns(pool, len(db))


def _pairs(eng, db, excerpts):
    """the (query codes, reference codes) of every excerpt x candidate, as locate_scores forms them"""
    from audio_sheet_retrieval_amd import piece_identification as pid
    dev, _ = pid._to_device(eng, excerpts)
    votes = pid._detect_batch(eng, db, dev, 2, (92, 42), False, CANDS, 25, 100, None, 4096, with_ids=True)
    starts, desc = pid.locate_window_plan(dev.shapes, dev.offsets, (92, 42), STEP)
    n_win = len(desc)
    d_win, d_codes = eng.alloc(min(n_win, 4096) * 92 * 42 * 4), eng.alloc(n_win * 32 * 4)
    pid.embed_windows_dev(eng, 2, dev.buf.ptr, dev.buf.nbytes // 4, desc, (92, 42), d_win, d_codes, min(n_win, 4096))
    codes = d_codes.download((n_win, 32), np.float32)
    for b in (d_win, d_codes, dev.buf):
        b.free()
    at = np.concatenate([[0], np.cumsum([len(s) for s in starts])])
    segs = pid.piece_segments(db.ids)
    queries = [codes[at[e]:at[e + 1]] for e in range(len(excerpts))]
    refs = {p: db.codes[f:f + n] for p, (f, n) in segs.items()}
    return queries, refs, [(e, int(p)) for e, v in enumerate(votes) for p in v[2]]


def leg_route(eng, reps):
    from audio_sheet_retrieval_amd import piece_identification as pid
    pool, db, excerpts, cols = _setup(eng)
    kw = dict(n_pieces=CANDS, step_spec=STEP, n_candidates=25, sheet_columns=cols)
    got, want = pid.locate_scores(eng, db, excerpts, **kw), pid.locate_scores_host(eng, db, excerpts, **kw)
    for g, w in zip(got, want):
        assert [(c["name"], c["cost"], c["start_row"], c["end_row"]) for c in g] == \
               [(c["name"], c["cost"], c["start_row"], c["end_row"]) for c in w], "device and host routes differ"
        assert all(np.array_equal(a["x"], b["x"]) for a, b in zip(g, w))
    out = {"excerpts": len(excerpts), "pairs": int(sum(len(g) for g in got)), "db_rows": len(db)}
    out["locate_scores_s"], out["locate_scores_range_s"] = _median(lambda: pid.locate_scores(eng, db, excerpts, **kw), reps)
    out["locate_scores_host_s"], out["locate_scores_host_range_s"] = _median(
        lambda: pid.locate_scores_host(eng, db, excerpts, **kw), reps, warm=False)
    out["route_speedup"] = out["locate_scores_host_s"] / out["locate_scores_s"]
    # the stages of the device route, each ended by a call that synchronises
    dev, _ = pid._to_device(eng, excerpts)
    out["vote_s"], _ = _median(lambda: pid._detect_batch(eng, db, dev, 2, (92, 42), False, CANDS, 25, 100, None, 4096), reps)
    starts, desc = pid.locate_window_plan(dev.shapes, dev.offsets, (92, 42), STEP)
    n_win = len(desc)
    d_win, d_codes = eng.alloc(min(n_win, 4096) * 92 * 42 * 4), eng.alloc(n_win * 32 * 4)

    def embed():
        pid.embed_windows_dev(eng, 2, dev.buf.ptr, dev.buf.nbytes // 4, desc, (92, 42), d_win, d_codes, min(n_win, 4096))
        eng.sync()
    out["windows"] = n_win
    out["embed_windows_s"], _ = _median(embed, reps)
    queries, refs, pairs = _pairs(eng, db, excerpts)
    segs = pid.piece_segments(db.ids)
    n_q = np.array([len(s) for s in starts], np.int64)
    at = np.concatenate([[0], np.cumsum(n_q)])
    tabs = ([at[e] for e, _ in pairs], [n_q[e] for e, _ in pairs], [segs[p][0] for _, p in pairs],
            [segs[p][1] for _, p in pairs])
    out["dtw_call_s"], _ = _median(lambda: eng.dtw_subseq_batch_dev(d_codes.ptr, n_win, db._d_codes.ptr, len(db), *tabs,
                                                                    dim=32), reps)
    out["cells"] = float(sum(a * b for a, b in zip(tabs[1], tabs[3])))
    out["dtw_share_of_route"] = out["dtw_call_s"] / out["locate_scores_s"]
    out["dtw_against_embedding"] = out["dtw_call_s"] / out["embed_windows_s"]
    for b in (d_win, d_codes, dev.buf):
        b.free()
    return out


def _scope_ms(eng, name):
    return sum(r["total_ms"] for r in eng.profile() if r["name"] == name)


def leg_kernel(eng, reps):
    pool, db, excerpts, _ = _setup(eng)
    queries, refs, pairs = _pairs(eng, db, excerpts)
    ref_ids = sorted(refs)
    ref_list, where = [refs[p] for p in ref_ids], {p: k for k, p in enumerate(ref_ids)}
    sub_pairs = [(e, where[p]) for e, p in pairs]
    full_pairs = [(queries[e], refs[p]) for e, p in pairs]
    out = {"pairs": len(pairs), "cells": float(sum(len(a) * len(b) for a, b in full_pairs)),
           "query_rows": [int(min(len(q) for q in queries)), int(max(len(q) for q in queries))],
           "reference_rows": [int(min(len(r) for r in ref_list)), int(max(len(r) for r in ref_list))]}
    eng.dtw_subseq_batch(queries, ref_list, sub_pairs)                       # warm-up of both
    eng.dtw_batch(full_pairs, want_dists=False, want_path=False)
    eng.profile_enable(True)
    fused, fused_call, dist = [], [], []
    for _ in range(reps):                                                    # alternating
        eng.profile_reset()
        eng.dtw_subseq_batch(queries, ref_list, sub_pairs)
        fused.append(_scope_ms(eng, "dtw_subseq_wave"))
        fused_call.append(_scope_ms(eng, "dtw_subseq"))
        eng.profile_reset()
        eng.dtw_batch(full_pairs, want_dists=False, want_path=False)
        dist.append(_scope_ms(eng, "dtw_batch"))
    out["fused_kernels_ms"], out["fused_call_device_ms"] = float(np.median(fused)), float(np.median(fused_call))
    out["distance_pass_ms"] = float(np.median(dist))                         # norms + pair table + dtw_batch_dist_kernel
    out["fused_over_distance_pass"] = out["fused_kernels_ms"] / out["distance_pass_ms"]
    out["fused_cells_per_s"] = out["cells"] / (1e-3 * out["fused_kernels_ms"])
    # one pair alone: the serial length of the wavefront
    rng = np.random.default_rng(3)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    for Q, S in ((180, 2000), (40, 2000), (1024, 2000)):
        q, r = unit(rng.standard_normal((Q, 32))), unit(rng.standard_normal((S, 32)))
        eng.dtw_subseq_batch([q], [r], [(0, 0)])
        ms = []
        for _ in range(reps):
            eng.profile_reset()
            eng.dtw_subseq_batch([q], [r], [(0, 0)])
            ms.append(_scope_ms(eng, "dtw_subseq_wave"))
        out["single_%dx%d_ms" % (Q, S)] = float(np.median(ms))
        out["single_%dx%d_us_per_diagonal" % (Q, S)] = 1e3 * float(np.median(ms)) / (Q + S - 1)
    eng.profile_enable(False)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--leg", choices=sorted(LEG_LIMIT_S))
    p.add_argument("--all", action="store_true", help="run every leg in a process of its own and merge the results")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.all:
        res = {}
        for leg in ("kernel", "route"):
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=LEG_LIMIT_S[leg])
            if run.returncode != 0:
                sys.stderr.write(run.stdout + run.stderr)
                raise SystemExit("leg %s failed with status %d" % (leg, run.returncode))
            res[leg] = json.loads(run.stdout.strip().splitlines()[-1])["result"]
        line = json.dumps({"workload": "%d excerpts of %d frames x %d candidates, %d synthetic pieces"
                           % (N_PIECES * CUTS, FRAMES, CANDS, N_PIECES), "reps": args.reps, "result": res}, sort_keys=True)
    else:
        if not args.leg:
            p.error("--leg or --all")
        from audio_sheet_retrieval_amd import _lib
        eng = _lib.Engine("mutopia_ccal_cont")
        res = leg_route(eng, args.reps) if args.leg == "route" else leg_kernel(eng, args.reps)
        eng.close()
        line = json.dumps({"leg": args.leg, "result": res}, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
