#!/usr/bin/env python
"""Timing of the running piece vote (audio_sheet_server --track; piece_identification.track_scores) against the
per-frame composition of the single-query calls, in the same process on the same device:

    python tools/bench_track.py [--recordings 16] [--frames 3000] [--loop-recordings 2] [--out profiles/r14_track.json]

Workload: --recordings synthetic spectrograms of about --frames frames (92 bins, a silent tenth in the middle), a random
data base of --db codes over --pieces pieces, the committed trained weights, the driver's defaults (running_frames 100,
n_candidates 25, top_k 7).
  batched   : track_scores over all recordings - one gate call, gather / tower 2 / top-k per 4096 voiced frames, one
              sliding-vote call.
  stages    : the same call with a synchronisation after every stage (gate / gather / embed / topk / vote).
  per_frame : per voiced frame one asr_slice_windows_dev, one asr_embed_view2_dev, one asr_topk_db_dev and one
              asr_piece_vote_dev over the index rows of its history, the result downloaded - what the calls that existed
              before this one compose to.  The voiced flags are taken from the batched result and not timed, and only
              the first --loop-recordings recordings are looped (the loop is slow); its time is also given per voiced
              frame and scaled to all recordings.  Both paths must give the same pieces and counts.
Times are wall clock after one warm-up call: median, minimum and maximum of --reps.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _note(text):
    print("[bench_track] " + text, file=sys.stderr, flush=True)


def _times(fn, reps):
    t = time.perf_counter()
    fn()
    _note("warm-up call: %.3f s" % (time.perf_counter() - t))
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts))}


def per_frame_loop(eng, db, spec, frames, top_k, n_candidates, running_frames, win=(92, 42)):
    """the loop of AudioSheetServer.run over the voiced frames with one call per step"""
    spec = np.ascontiguousarray(spec, np.float32)
    rows, T = spec.shape
    d_src = db.scratch("src", spec.nbytes).upload(spec)
    d_win, d_codes = db.scratch("win", win[0] * win[1] * 4), db.scratch("codes", 32 * 4)
    d_idx, d_dist = db.scratch("idx", max(len(frames), 1) * n_candidates * 4), db.scratch("dist", n_candidates * 8)
    out = []
    for k, i in enumerate(frames):
        eng.slice_windows_dev(d_src.ptr, rows, T, 0, win[0], win[1], [i - win[1] + 1], d_win.ptr)
        eng.embed_view2_dev(d_win.ptr, 1, d_codes.ptr)
        db.topk_dev(d_codes.ptr, 1, n_candidates, d_idx.offset(k * n_candidates * 4), d_dist.ptr)
        k0 = max(0, k - running_frames + 1)
        out.append(eng.piece_vote_dev(d_idx.offset(k0 * n_candidates * 4), (k - k0 + 1) * n_candidates, db._d_ids.ptr,
                                      len(db), db.n_pieces, top_k))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--recordings", type=int, default=16)
    p.add_argument("--frames", type=int, default=3000)
    p.add_argument("--loop-recordings", type=int, default=2)
    p.add_argument("--db", type=int, default=20000)
    p.add_argument("--pieces", type=int, default=64)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--running_frames", type=int, default=100)
    p.add_argument("--n_candidates", type=int, default=25)
    p.add_argument("--top_k", type=int, default=7)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    from audio_sheet_retrieval_amd import _lib, piece_identification as pid
    eng = _lib.Engine("mutopia_ccal_cont")
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        eng.set_params([z["p%02d" % i] for i in range(97)])
    rng = np.random.default_rng(14)
    codes = rng.standard_normal((args.db, 32)).astype(np.float32)
    ids = np.sort(rng.integers(0, args.pieces, size=args.db))
    db = pid.EmbeddingDB(eng, codes, ids, {i: "piece_%03d" % i for i in range(args.pieces)})
    specs = []
    for r in range(args.recordings):
        T = args.frames + int(rng.integers(-100, 101))
        s = (3.0 * rng.random((92, T)) ** 2).astype(np.float32)
        s[:, T // 2:T // 2 + T // 10] = 0.0
        specs.append(s)
    kw = dict(top_k=args.top_k, n_candidates=args.n_candidates, running_frames=args.running_frames)
    res = {"recordings": args.recordings, "frames": int(sum(s.shape[1] for s in specs)), "db_entries": args.db,
           "pieces": args.pieces, "reps": args.reps}
    res.update(kw)
    res["batched"] = _times(lambda: pid.track_scores(eng, db, specs, **kw), args.reps)
    _note("batched: %r" % (res["batched"],))
    tracked = pid.track_scores(eng, db, specs, **kw)
    res["voiced_frames"] = int(sum(len(t.frames) for t in tracked))
    per_stage = []
    for _ in range(args.reps + 1):
        st = {}
        pid.track_scores(eng, db, specs, stages=st, **kw)
        per_stage.append(st)
    res["stages"] = {k: {"median_s": float(np.median([s[k] for s in per_stage[1:]])),
                         "min_s": float(np.min([s[k] for s in per_stage[1:]])),
                         "max_s": float(np.max([s[k] for s in per_stage[1:]]))} for k in per_stage[0]}
    _note("stages: %r" % (res["stages"],))
    n_loop = min(args.loop_recordings, args.recordings)
    if n_loop > 0:
        loop = lambda: [per_frame_loop(eng, db, specs[r], tracked[r].frames, **kw) for r in range(n_loop)]
        res["per_frame"] = _times(loop, args.reps)
        voiced_loop = int(sum(len(tracked[r].frames) for r in range(n_loop)))
        res["per_frame"]["recordings"] = n_loop
        res["per_frame"]["voiced_frames"] = voiced_loop
        res["per_frame"]["s_per_voiced_frame"] = res["per_frame"]["median_s"] / max(voiced_loop, 1)
        res["per_frame"]["scaled_to_all_s"] = res["per_frame"]["s_per_voiced_frame"] * res["voiced_frames"]
        res["speedup_scaled"] = res["per_frame"]["scaled_to_all_s"] / res["batched"]["median_s"]
        for r, out in enumerate(loop()):
            for k, (pieces, counts) in enumerate(out):
                n = int(tracked[r].n_out[k])
                assert np.array_equal(pieces, tracked[r].pieces[k, :n]) and np.array_equal(counts, tracked[r].counts[k, :n]), \
                    "per-frame and batched votes differ at recording %d, voiced frame %d" % (r, k)
    db.close()
    eng.close()
    line = json.dumps({"result": res}, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
