#!/usr/bin/env python
"""Timing of one round of score following for N parallel live streams: the bank with its state on the device against
one ScoreFollower per stream, in the same process on the same device:

    python tools/bench_live_follow.py [--streams 1 16] [--columns 2 20] [--out profiles/r26_live_follow.json]

Setting (round 14's / round 25's): a random data base of --db codes over --pieces pieces with contiguous segments, the
committed trained weights, step_spec 2, --slots fixed candidates per stream (ScoreFollower cannot swap, so neither side
does while it is timed).  Every stream is noise and is pushed past --history windows before anything is timed.
  bank      : one ScoreFollowerBank.push on the device columns of all streams (what AudioStream.push_dev returns).
  followers : one ScoreFollower.push per stream on host columns - the route before the bank.
Both sides get the same columns and must return the same results.  A sample is the wall clock of --rounds consecutive
rounds divided by --rounds; the two sides alternate sample by sample; median, minimum and maximum of --reps samples
after one warm-up sample each.  Then, in passes of their own: the bank's stages with a synchronisation after each; the
kernel times of the two new calls from the library's profile scopes (follow_stream_windows = window assembly + tail
slide, follow_stream_log = log slide + new rows), their bytes (every float read once and written once) set against the
rate of a device-to-device copy timed in the same process; and the time of a round in which every slot of every stream
enters with catch_up windows of history against the round after it, in which none does.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_live_track import _stat, copy_rate  # noqa: E402

BINS, WIDTH, STEP = 92, 42, 2
KEYS = ("cost", "row", "start_row", "x", "start_x")


def _note(text):
    print("[bench_live_follow] " + text, file=sys.stderr, flush=True)


def _same(got, want, slots):
    assert np.array_equal(got.frames, want.frames) and np.array_equal(got.best, want.best)
    for key in KEYS:
        assert np.array_equal(getattr(got, key)[:, :slots], getattr(want, key)), key


def case(eng, db, pid, n_streams, n_cols, args):
    rng = np.random.default_rng(26 * n_streams + n_cols)
    warm = WIDTH + STEP * args.history + 20
    rounds = args.rounds * (2 * (args.reps + 1) + 2) + 2 * args.entries + 2
    T = warm + rounds * n_cols
    specs = [(3.0 * rng.random((BINS, T)) ** 2).astype(np.float32) for _ in range(n_streams)]
    cands = [[int(p) for p in rng.choice(args.pieces, size=2 * args.slots, replace=False)] for _ in range(n_streams)]
    fixed, other = [c[:args.slots] for c in cands], [c[args.slots:] for c in cands]
    bank = pid.ScoreFollowerBank(eng, db, n_streams, n_slots=args.slots, step_spec=STEP, catch_up=args.catch_up)
    followers = [pid.ScoreFollower(eng, db, c, step_spec=STEP) for c in fixed]
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
        for s, c in enumerate(fixed):
            bank.set_candidates(s, c)
        first = blocks(warm)
        got = bank.push(handle(first))
        want = [f.push(b) for f, b in zip(followers, first)]
        for g, w in zip(got, want):
            _same(g, w, args.slots)
        assert all(w > args.history for w in bank.n_windows), bank.n_windows

        def sample_bank():
            per_round = [blocks(n_cols) for _ in range(args.rounds)]
            t, res = 0.0, []
            for blks in per_round:
                h = handle(blks)                                     # the columns are on the device already: not timed
                eng.sync()
                t0 = time.perf_counter()
                res.append(bank.push(h))
                t += time.perf_counter() - t0
            return t / args.rounds, per_round, res

        def sample_followers(per_round):
            t0 = time.perf_counter()
            res = [[f.push(b) for f, b in zip(followers, blks)] for blks in per_round]
            return (time.perf_counter() - t0) / args.rounds, res

        ta, tb = [], []
        for rep in range(args.reps + 1):
            a, per_round, ra = sample_bank()
            b, rb = sample_followers(per_round)
            for x, y in zip(ra, rb):
                for g, w in zip(x, y):
                    _same(g, w, args.slots)
            if rep:
                ta.append(a), tb.append(b)
        row = {"streams": n_streams, "columns": n_cols, "bank": _stat(ta), "followers": _stat(tb),
               "followers_over_bank": float(np.median(tb) / np.median(ta))}
        # the bank's stages, a synchronisation after each
        bank.stages = {}
        for _ in range(args.rounds):
            bank.push(handle(blocks(n_cols)))
        row["bank_stages_s"] = {k: v / args.rounds for k, v in bank.stages.items()}
        bank.stages = None
        # kernel times of the new calls from the profile scopes
        eng.profile_enable(True)
        eng.profile_reset()
        for _ in range(args.rounds):
            bank.push(handle(blocks(n_cols)))
        prof = {p["name"]: p for p in eng.profile() if p["name"].startswith("follow_stream_")}
        eng.profile_enable(False)
        row["kernels_ms"] = {k: v["total_ms"] / max(v["launches"], 1) for k, v in prof.items()}
        n_win = n_cols // STEP
        moved = {"follow_stream_windows": 4.0 * n_streams * BINS * (n_win * WIDTH + WIDTH - 1),
                 "follow_stream_log": 4.0 * n_streams * 32 * (n_win + args.catch_up)}    # the log is full: kept rows move
        row["bytes_written"] = moved
        # a round in which every slot enters (catch_up windows of history each) against the round after it
        t_enter, t_after = [], []
        for k in range(args.entries + 1):
            for s in range(n_streams):
                bank.set_candidates(s, other[s] if k % 2 == 0 else fixed[s])
            for ts in (t_enter, t_after):
                h = handle(blocks(n_cols))
                eng.sync()
                t0 = time.perf_counter()
                res = bank.push(h)
                ts.append(time.perf_counter() - t0)
            assert all((r.since[-1] == r.since[-1][0]).all() and r.since[-1][0] > 0 for r in res)
        row["entering_round"] = _stat(t_enter[1:])
        row["round_after"] = _stat(t_after[1:])
        _note("%r" % (row,))
        return row
    finally:
        bank.close()
        for f in followers:
            f.close()
        d_cols.free()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--streams", type=int, nargs="+", default=[1, 16])
    p.add_argument("--columns", type=int, nargs="+", default=[2, 20])
    p.add_argument("--db", type=int, default=20000)
    p.add_argument("--pieces", type=int, default=64)
    p.add_argument("--slots", type=int, default=5)
    p.add_argument("--catch_up", type=int, default=64)
    p.add_argument("--history", type=int, default=200, help="windows every stream has behind it before the timing")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--rounds", type=int, default=20, help="consecutive rounds per timing sample")
    p.add_argument("--entries", type=int, default=10, help="timed rounds in which every slot enters")
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
    res = {"tool": "bench_live_follow", "db_entries": args.db, "pieces": args.pieces, "reps": args.reps,
           "rounds_per_sample": args.rounds, "bins": BINS, "width": WIDTH, "step_spec": STEP, "slots": args.slots,
           "catch_up": args.catch_up, "history_windows": args.history, "entries": args.entries}
    res["cases"] = [case(eng, db, pid, n, c, args) for n in args.streams for c in args.columns]
    res["copy_gb_per_s"] = copy_rate(eng)
    db.close()
    eng.close()
    for row in res["cases"]:
        row["share_of_copy_rate"] = {}
        for name, nbytes in row["bytes_written"].items():
            ms = row["kernels_ms"].get(name)
            if ms:
                row["share_of_copy_rate"][name] = 2.0 * nbytes / (ms * 1e-3) / 1e9 / res["copy_gb_per_s"]
    line = json.dumps({"result": res}, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
