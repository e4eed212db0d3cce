#!/usr/bin/env python
"""Timing of piece identification over whole test pieces (audio_sheet_server / sheet_audio_server --full_eval): the
per-piece loop of detect_score / detect_performance against the batched detect_scores / detect_performances (one
asr_piece_vote_batch_dev call for all pieces), and the data-base build (EmbeddingDB.from_pool) timed on its own.
One piece count per process:

    python tools/bench_identify.py --pieces 16
    python tools/bench_identify.py --pieces 64      # also the A2S / S2A rank counts (trained weights)
    python tools/bench_identify.py --pieces 256
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_identify.py --pieces 64 --batched-only

Pieces: synth_data.synth_pieces(n) with the committed trained weights (tests/golden/trained_cont_params.npz), 100
windows per query, --n_candidates 25, top_k = n (the per-piece loop: min(n, 1024), the single-query cap).  Both paths
must give the same ranks.  Times are wall clock of the Python call after one warm-up call, median of --reps.  Prints
one JSON line (also written to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_time(fn, reps):
    fn()                                           # warm-up: buffers, code objects
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pieces", type=int, default=64)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--n_candidates", type=int, default=25)
    p.add_argument("--batched-only", action="store_true", help="only the batched calls (for a kernel-trace run)")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    from audio_sheet_retrieval_amd import _lib, piece_identification as pid
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
    eng = _lib.Engine("mutopia_ccal_cont")
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        eng.set_params([z["p%02d" % i] for i in range(97)])
    n = args.pieces
    images, specs, o2c_maps = synth_data.synth_pieces(n)
    names = ["synthetic_%03d" % i for i in range(n)]
    pool = AudioScoreRetrievalPool(eng, images, specs, o2c_maps, data_augmentation=dict(NO_AUGMENT), shuffle=False)
    res = {"pieces": n, "db_entries": int(pool.shape[0]), "n_candidates": args.n_candidates}
    targets = np.arange(n, dtype=np.int32)
    k = args.n_candidates
    for direction, view in (("A2S", 1), ("S2A", 2)):
        dbs = []
        build = lambda: dbs.append(pid.EmbeddingDB.from_pool(eng, pool, view, names=names))
        res[direction + "_db_build_s"] = _median_time(build, 1 if args.batched_only else args.reps)
        db = dbs[-1]
        for old in dbs[:-1]:
            old.close()
        if direction == "A2S":
            queries = [s[0] for s in specs]
            batched = lambda: pid.detect_scores(eng, db, queries, top_k=n, n_candidates=k, targets=targets)
            single = lambda q: pid.detect_score(eng, db, q, top_k=min(n, 1024), n_candidates=k)
        else:
            queries = images
            batched = lambda: pid.detect_performances(eng, db, queries, top_k=n, n_candidates=k, targets=targets)
            single = lambda q: pid.detect_performance(eng, db, q, top_k=min(n, 1024), n_candidates=k)
        res[direction + "_batched_s"] = _median_time(batched, args.reps)
        _, ranks, ratios = batched()
        if not args.batched_only:
            loop = lambda: [single(q) for q in queries]
            res[direction + "_per_piece_s"] = _median_time(loop, args.reps)
            res[direction + "_speedup"] = res[direction + "_per_piece_s"] / res[direction + "_batched_s"]
            loop_ranks = [pid.full_eval_rank(r[0], r[1], name)[0] for r, name in zip(loop(), names)]
            assert loop_ranks == ranks.tolist(), "per-piece and batched ranks differ"
        summary = pid.rank_summary(ranks)
        res[direction + "_ranks"] = {key: list(v) for key, v in summary.items()}
        res[direction + "_mean_target_ratio"] = float(np.mean(ratios))
        db.close()
    eng.close()
    line = json.dumps({"result": res}, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
