#!/usr/bin/env python
"""Timing of one round of the live tracker for N parallel streams: the bank with its state on the device against one
PieceTracker per stream, in the same process on the same device:

    python tools/bench_live_track.py [--streams 1 16] [--columns 2 20] [--out profiles/r25_live_track.json]

Setting (round 14's): a random data base of --db codes over --pieces pieces, the committed trained weights,
running_frames 100, n_candidates 25, top_k 7.  Every stream is loud noise, so the gate is open, and is pushed until its
history is full before anything is timed.
  bank     : one PieceTrackerBank.push on the device columns of all streams (what AudioStream.push_dev returns).
  trackers : one PieceTracker.push per stream on host columns - the route of live_track_scores' default.
Both sides get the same columns and must return the same results.  A sample is the wall clock of --rounds consecutive
rounds divided by --rounds; the two sides alternate sample by sample; median, minimum and maximum of --reps samples
after one warm-up sample each.  Then, in passes of their own: the bank's stages with a synchronisation after each, and
the kernel times of the two new calls from the library's profile scopes (track_stream_gate = column sums + gate + window
numbering, track_stream_windows = window assembly + tail slide, track_stream_vote = votes + ring write-back).  The
window scope's bytes written (twice: every float is read once and written once) are set against the rate of a
device-to-device copy timed in the same process.  Prints one
JSON line.

    python tools/bench_live_track.py --level [--out profiles/r28_live_level.json]

measures instead what the gate at the level of what has been heard so far costs: three banks - the fixed level (the
route above, the baseline), RunningLevel() and RunningLevel(memory=--level_memory) - get the same device columns and
alternate sample by sample in one process.  Per setting the whole round and, in samples of their own with a
synchronisation after every stage, the bank's `gate` stage; medians of --reps samples of --rounds rounds with their
ranges.  The streams are pushed until the history and the level's ring are full before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS, WIDTH = 92, 42


def _note(text):
    print("[bench_live_track] " + text, file=sys.stderr, flush=True)


def _stat(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts))}


def copy_rate(eng):
    """GB/s (read + write) of a 256 MiB device-to-device copy through the HIP runtime the library runs on: a sample is
    ten copies and a synchronisation, the median of 5 samples after a warm-up"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    nbytes, copies = 256 << 20, 10
    a, b = eng.alloc(nbytes), eng.alloc(nbytes)
    try:
        a.upload(np.ones(nbytes // 4, np.float32))
        ts = []
        for _ in range(6):
            assert hip.hipDeviceSynchronize() == 0
            t0 = time.perf_counter()
            for _ in range(copies):
                assert hip.hipMemcpy(b.ptr, a.ptr, nbytes, 3) == 0   # hipMemcpyDeviceToDevice
            assert hip.hipDeviceSynchronize() == 0
            ts.append((time.perf_counter() - t0) / copies)
    finally:
        a.free()
        b.free()
    return 2.0 * nbytes / float(np.median(ts[1:])) / 1e9


def _same(a, b):
    for name in ("m_prob", "voiced", "frames", "pieces", "counts", "n_out", "history", "idx"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def case(eng, db, pid, n_streams, n_cols, args, kw):
    rng = np.random.default_rng(25 * n_streams + n_cols)
    warm = WIDTH + args.running_frames + 20
    rounds = args.rounds * 2 * (args.reps + 1) + 2 * args.rounds + 2
    T = warm + rounds * n_cols
    specs = [(3.0 * rng.random((BINS, T)) ** 2).astype(np.float32) for _ in range(n_streams)]
    levels = [s.sum(axis=0).max() for s in specs]
    bank = pid.PieceTrackerBank(eng, db, levels, **kw)
    trackers = [pid.PieceTracker(eng, db, lv, **kw) for lv in levels]
    d_cols = eng.alloc(n_streams * BINS * max(warm, n_cols) * 4)
    at = [0]

    def blocks(n):
        out = [np.ascontiguousarray(s[:, at[0]:at[0] + n]) for s in specs]
        at[0] += n
        return out

    def handle(blks):
        d_cols.upload(np.concatenate([b.ravel() for b in blks]))
        sizes = [b.size for b in blks]
        return pid.DeviceArrays(d_cols, [int(o) for o in np.concatenate([[0], np.cumsum(sizes)[:-1]])], [b.shape for b in blks])

    try:
        first = blocks(warm)
        got = bank.push(handle(first))
        want = [t.push(b) for t, b in zip(trackers, first)]
        for g, w in zip(got, want):
            _same(g, w)
        assert all(v >= args.running_frames for v in bank.n_voiced), bank.n_voiced       # steady state: history full

        def sample_bank():
            per_round = [blocks(n_cols) for _ in range(args.rounds)]
            t = 0.0
            res = []
            for blks in per_round:
                h = handle(blks)                                     # the columns are on the device already: not timed
                eng.sync()
                t0 = time.perf_counter()
                res.append(bank.push(h))
                t += time.perf_counter() - t0
            return t / args.rounds, per_round, res

        def sample_trackers(per_round):
            t0 = time.perf_counter()
            res = [[tr.push(b) for tr, b in zip(trackers, blks)] for blks in per_round]
            return (time.perf_counter() - t0) / args.rounds, res

        ta, tb = [], []
        for rep in range(args.reps + 1):
            a, per_round, ra = sample_bank()
            b, rb = sample_trackers(per_round)
            for x, y in zip(ra, rb):
                for g, w in zip(x, y):
                    _same(g, w)
                    assert g.voiced.all()                            # gate open
            if rep:
                ta.append(a), tb.append(b)
        row = {"streams": n_streams, "columns": n_cols, "bank": _stat(ta), "trackers": _stat(tb),
               "trackers_over_bank": float(np.median(tb) / np.median(ta))}
        # the bank's stages, a synchronisation after each (the trackers are fed too: they stay in step)
        bank.stages = {}
        for _ in range(args.rounds):
            blks = blocks(n_cols)
            bank.push(handle(blks))
            [t.push(b) for t, b in zip(trackers, blks)]
        row["bank_stages_s"] = {k: v / args.rounds for k, v in bank.stages.items()}
        bank.stages = None
        # kernel times of the new calls from the profile scopes
        eng.profile_enable(True)
        eng.profile_reset()
        for _ in range(args.rounds):
            blks = blocks(n_cols)
            bank.push(handle(blks))
            [t.push(b) for t, b in zip(trackers, blks)]
        prof = {p["name"]: p for p in eng.profile() if p["name"].startswith("track_stream_")}
        eng.profile_enable(False)
        row["kernels_ms"] = {k: v["total_ms"] / max(v["launches"], 1) for k, v in prof.items()}
        win_bytes = 4.0 * n_streams * n_cols * BINS * WIDTH
        ms = row["kernels_ms"].get("track_stream_windows")
        if ms:
            row["windows"] = {"bytes_written": win_bytes, "gb_per_s_written": win_bytes / (ms * 1e-3) / 1e9}
        _note("%r" % (row,))
        return row
    finally:
        bank.close()
        d_cols.free()


def level_case(eng, db, pid, n_streams, n_cols, args, kw):
    """one round of n_cols columns on n_streams streams at the three level rules -> the row of the result"""
    rng = np.random.default_rng(28 * n_streams + n_cols)
    warm = max(WIDTH + args.running_frames + 20, args.level_memory + 50)
    T = warm + 2 * (args.reps + 1) * args.rounds * n_cols
    specs = [(3.0 * rng.random((BINS, T)) ** 2).astype(np.float32) for _ in range(n_streams)]
    rules = {"fixed": None, "running": pid.RunningLevel(), "running_memory": pid.RunningLevel(memory=args.level_memory)}
    banks = {}
    d_cols = eng.alloc(n_streams * BINS * max(warm, n_cols) * 4)
    at = [0]

    def blocks(n):
        out = [np.ascontiguousarray(s[:, at[0]:at[0] + n]) for s in specs]
        at[0] += n
        return out

    def handle(blks):
        d_cols.upload(np.concatenate([b.ravel() for b in blks]))
        sizes = [b.size for b in blks]
        return pid.DeviceArrays(d_cols, [int(o) for o in np.concatenate([[0], np.cumsum(sizes)[:-1]])], [b.shape for b in blks])

    try:
        for name, rule in rules.items():
            banks[name] = (pid.PieceTrackerBank(eng, db, [s.sum(axis=0).max() for s in specs], **kw) if rule is None else
                           pid.PieceTrackerBank(eng, db, rule, n_streams=n_streams, **kw))
        first = blocks(warm)
        for bank in banks.values():
            bank.push(handle(first))
            assert all(v >= args.running_frames for v in bank.n_voiced), bank.n_voiced   # steady state: history full

        def sample(stage):
            """every bank over the same args.rounds rounds, one bank after the other -> seconds per round and bank"""
            per_round = [blocks(n_cols) for _ in range(args.rounds)]
            out = {}
            for name, bank in banks.items():
                bank.stages = {} if stage else None
                t = 0.0
                for blks in per_round:
                    h = handle(blks)                                 # the columns are on the device already: not timed
                    eng.sync()
                    t0 = time.perf_counter()
                    res = bank.push(h)
                    t += time.perf_counter() - t0
                    assert all(r.voiced.all() for r in res)          # gate open: the same work behind every gate
                out[name] = (bank.stages["gate"] if stage else t) / args.rounds
                bank.stages = None
            return out

        times = {"round": {k: [] for k in banks}, "gate": {k: [] for k in banks}}
        for rep in range(args.reps + 1):
            for what, stage in (("round", False), ("gate", True)):
                for name, t in sample(stage).items():
                    if rep:
                        times[what][name].append(t)
        row = {"streams": n_streams, "columns": n_cols,
               "settings": {k: {"round": _stat(times["round"][k]), "gate_stage": _stat(times["gate"][k])} for k in banks}}
        for what, key in (("round", "round"), ("gate", "gate_stage")):
            base = float(np.median(times[what]["fixed"]))
            row[key + "_over_fixed"] = {k: float(np.median(times[what][k]) / base) for k in banks if k != "fixed"}
        _note("%r" % (row,))
        return row
    finally:
        for bank in banks.values():
            bank.close()
        d_cols.free()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--streams", type=int, nargs="+", default=[1, 16])
    p.add_argument("--columns", type=int, nargs="+", default=[2, 20])
    p.add_argument("--db", type=int, default=20000)
    p.add_argument("--pieces", type=int, default=64)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--rounds", type=int, default=20, help="consecutive rounds per timing sample")
    p.add_argument("--running_frames", type=int, default=100)
    p.add_argument("--n_candidates", type=int, default=25)
    p.add_argument("--top_k", type=int, default=7)
    p.add_argument("--out", default=None)
    p.add_argument("--level", action="store_true",
                   help="measure the gate at the level of what has been heard so far against the fixed level")
    p.add_argument("--level_memory", type=int, default=1200, help="--level: the bounded memory (a minute at 20 fps)")
    args = p.parse_args()
    from audio_sheet_retrieval_amd import _lib, piece_identification as pid
    eng = _lib.Engine("mutopia_ccal_cont")
    with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
        eng.set_params([z["p%02d" % i] for i in range(97)])
    rng = np.random.default_rng(14)
    codes = rng.standard_normal((args.db, 32)).astype(np.float32)
    ids = np.sort(rng.integers(0, args.pieces, size=args.db))
    db = pid.EmbeddingDB(eng, codes, ids, {i: "piece_%03d" % i for i in range(args.pieces)})
    kw = dict(top_k=args.top_k, n_candidates=args.n_candidates, running_frames=args.running_frames)
    res = {"tool": "bench_live_track", "db_entries": args.db, "pieces": args.pieces, "reps": args.reps,
           "rounds_per_sample": args.rounds, "bins": BINS, "width": WIDTH}
    res.update(kw)
    if args.level:
        res["tool"], res["level_memory"] = "bench_live_track --level", args.level_memory
        res["cases"] = [level_case(eng, db, pid, n, c, args, kw) for n in sorted(args.streams, reverse=True)
                        for c in args.columns]
    else:
        res["cases"] = [case(eng, db, pid, n, c, args, kw) for n in args.streams for c in args.columns]
        res["copy_gb_per_s"] = copy_rate(eng)
    db.close()
    eng.close()
    for row in res["cases"]:
        if "windows" in row:
            row["windows"]["share_of_copy_rate"] = 2.0 * row["windows"]["gb_per_s_written"] / res["copy_gb_per_s"]
    line = json.dumps({"result": res}, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
