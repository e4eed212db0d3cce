#!/usr/bin/env python
"""Timing of score following (asr_dtw_follow_batch_dev).  Workload: 16 streams of 1500 windows (three synthetic
performances back to back, a window per frame) x 5 candidate pieces against the pieces' from_pool sheet data base,
trained weights; the windows are embedded once, the legs time the alignment alone.  A stream is fed in blocks of 1, 8,
64 and 512 windows.  One leg per process, each under its own time limit:

    python tools/bench_follow.py --leg device    # (a) one asr_dtw_follow_batch_dev call per block, all 80 pairs;
                                                 # (b) what the library offered before: asr_dtw_subseq_batch_dev on the
                                                 #     whole prefix at every block, while the prefix fits its 1024 rows;
                                                 # kernel time per cell of (a) at each block size (library profile
                                                 # scopes, event timed): what the idle lanes of short blocks cost
    python tools/bench_follow.py --leg host      # (c) alignment.follow_dtw_host per block on the 5 pairs of stream 0,
                                                 #     against (a) on the same 5 pairs
    python tools/bench_follow.py --all --out profiles/r21_follow.json     # both legs, merged

Times are medians of --reps passes over the streams after one warm-up, with their ranges.  Every leg checks that the
blocks' results equal the host's on a pair.
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

N_STREAMS, CANDS, WINDOWS, BLOCKS, SUBSEQ_ROWS = 16, 5, 1500, (1, 8, 64, 512), 1024
LEG_LIMIT_S = {"device": 420, "host": 300}


def _median(fn, reps, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), [float(min(ts)), float(max(ts))]


class _Work(object):
    """the window codes of every stream on the device, the data base, the pair tables and a state buffer"""

    def __init__(self, eng, n_streams=N_STREAMS):
        from audio_sheet_retrieval_amd import piece_identification as pid
        from audio_sheet_retrieval_amd.utils import synth_data
        from audio_sheet_retrieval_amd.utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool
        with np.load(os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")) as z:
            eng.set_params([z["p%02d" % i] for i in range(97)])
        images, specs, o2c_maps = synth_data.synth_pieces(N_STREAMS)
        pool = AudioScoreRetrievalPool(eng, images, specs, o2c_maps, data_augmentation=dict(NO_AUGMENT), shuffle=False)
        self.eng, self.db = eng, pid.EmbeddingDB.from_pool(eng, pool, 1, names=["p%03d" % i for i in range(N_STREAMS)])
        streams = []
        for e in range(n_streams):
            parts, k = [], e
            while sum(p.shape[1] for p in parts) < WINDOWS + 41:
                parts.append(pool.specs[k % N_STREAMS][0])
                k += 1
            streams.append(np.ascontiguousarray(np.hstack(parts)[:, :WINDOWS + 41]))
        dev, _ = pid._to_device(eng, streams)
        desc = np.concatenate([pid._identity_desc(off, 92, T, 0, np.arange(WINDOWS))
                               for (_, T), off in zip(dev.shapes, dev.offsets)])
        self.n_win = len(desc)
        d_win, self.d_codes = eng.alloc(4096 * 92 * 42 * 4), eng.alloc(self.n_win * 32 * 4)
        pid.embed_windows_dev(eng, 2, dev.buf.ptr, dev.buf.nbytes // 4, desc, (92, 42), d_win, self.d_codes, 4096)
        for b in (d_win, dev.buf):
            b.free()
        segs = pid.piece_segments(self.db.ids)
        self.pairs = [(e, (e + c) % N_STREAMS) for e in range(n_streams) for c in range(CANDS)]
        self.q0 = np.array([e * WINDOWS for e, _ in self.pairs], np.int64)
        self.r_row = np.array([segs[p][0] for _, p in self.pairs], np.int64)
        self.n_r = np.array([segs[p][1] for _, p in self.pairs], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.n_r)]).astype(np.int64)
        self.d_acc, self.d_org = eng.alloc(int(self.off[-1]) * 8), eng.alloc(int(self.off[-1]) * 4)
        self.cells_per_row = float(self.n_r.sum())

    def follow_pass(self, block, keep=None):
        """(a): the streams in blocks of `block` windows, one call per block; keep: a list that receives pair 0's rows"""
        n = len(self.pairs)
        for c0 in range(0, WINDOWS, block):
            b = min(block, WINDOWS - c0)
            res = self.eng.dtw_follow_batch_dev(self.d_codes.ptr, self.n_win, self.db._d_codes.ptr, len(self.db),
                                                self.q0 + c0, np.full(n, b), self.r_row, self.n_r, np.full(n, c0), 32,
                                                self.d_acc.ptr, self.d_org.ptr, int(self.off[-1]), self.off[:-1])
            if keep is not None:
                keep.append(res[0])

    def prefix_pass(self, block):
        """(b): the whole prefix at every block, while it fits the subsequence call"""
        n = len(self.pairs)
        for c0 in range(0, SUBSEQ_ROWS - block + 1, block):
            self.eng.dtw_subseq_batch_dev(self.d_codes.ptr, self.n_win, self.db._d_codes.ptr, len(self.db), self.q0,
                                          np.full(n, c0 + block), self.r_row, self.n_r, 32, want_pos=False)

    def host_pair(self, k):
        """pair k's (query codes, reference codes)"""
        codes = self.d_codes.download((self.n_win, 32), np.float32)
        return (codes[self.q0[k]:self.q0[k] + WINDOWS], self.db.codes[self.r_row[k]:self.r_row[k] + self.n_r[k]])

    def check(self, block):
        from audio_sheet_retrieval_amd import alignment as al
        keep = []
        self.follow_pass(block, keep)
        q, r = self.host_pair(0)
        want = al.follow_dtw_host(al.cosine_dists_host(q, r))
        for k in range(3):
            assert np.array_equal(np.concatenate([part[k] for part in keep]), want[k]), "device and host differ"


def _scope_ms(eng, name):
    return sum(r["total_ms"] for r in eng.profile() if r["name"] == name)


def leg_device(eng, reps):
    w = _Work(eng)
    out = {"pairs": len(w.pairs), "windows_per_stream": WINDOWS, "reference_rows": [int(w.n_r.min()), int(w.n_r.max())],
           "cells_per_pass": w.cells_per_row * WINDOWS, "blocks": {}}
    for block in BLOCKS:
        w.check(block)
        o = out["blocks"][str(block)] = {"calls_per_pass": -(-WINDOWS // block)}
        o["follow_pass_s"], o["follow_pass_range_s"] = _median(lambda: w.follow_pass(block), reps)
        o["follow_block_ms"] = 1e3 * o["follow_pass_s"] / o["calls_per_pass"]
        eng.profile_enable(True)
        ms = []
        for _ in range(reps):
            eng.profile_reset()
            w.follow_pass(block)
            ms.append(_scope_ms(eng, "dtw_follow_wave"))
        eng.profile_enable(False)
        o["follow_kernels_pass_ms"], o["follow_kernels_pass_range_ms"] = float(np.median(ms)), [min(ms), max(ms)]
        o["follow_kernel_ns_per_cell"] = 1e6 * o["follow_kernels_pass_ms"] / out["cells_per_pass"]
        # (b) covers the first SUBSEQ_ROWS windows only: compare with (a)'s share of the same windows
        o["prefix_calls"] = SUBSEQ_ROWS // block
        o["prefix_pass_s"], o["prefix_pass_range_s"] = _median(lambda: w.prefix_pass(block), reps)
        o["follow_same_windows_s"] = o["follow_pass_s"] * (o["prefix_calls"] * block) / WINDOWS
        o["prefix_over_follow"] = o["prefix_pass_s"] / o["follow_same_windows_s"]
    # one call of (b) at the longest prefix it takes, against one block of (a)
    n = len(w.pairs)
    full = lambda: eng.dtw_subseq_batch_dev(w.d_codes.ptr, w.n_win, w.db._d_codes.ptr, len(w.db), w.q0, np.full(n, SUBSEQ_ROWS),
                                            w.r_row, w.n_r, 32, want_pos=False)
    out["prefix_1024_call_ms"], rng = _median(full, reps)
    out["prefix_1024_call_ms"], out["prefix_1024_call_range_ms"] = 1e3 * out["prefix_1024_call_ms"], [1e3 * v for v in rng]
    out["prefix_1024_call_over_follow_block_64"] = out["prefix_1024_call_ms"] / out["blocks"]["64"]["follow_block_ms"]
    return out


def leg_host(eng, reps):
    from audio_sheet_retrieval_amd import alignment as al
    w = _Work(eng, n_streams=1)
    pairs = [w.host_pair(k) for k in range(CANDS)]
    out = {"pairs": CANDS, "windows_per_stream": WINDOWS, "blocks": {}}

    def host_pass(block):
        for q, r in pairs:
            state = None
            for c0 in range(0, WINDOWS, block):
                state = al.follow_dtw_host(al.cosine_dists_host(q[c0:c0 + block], r), state)[3]
    for block in BLOCKS:
        w.check(block)
        o = out["blocks"][str(block)] = {}
        o["follow_pass_s"], o["follow_pass_range_s"] = _median(lambda: w.follow_pass(block), reps)
        o["host_pass_s"], o["host_pass_range_s"] = _median(lambda: host_pass(block), reps, warm=False)
        o["host_over_follow"] = o["host_pass_s"] / o["follow_pass_s"]
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
        for leg in ("device", "host"):
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=LEG_LIMIT_S[leg])
            if run.returncode != 0:
                sys.stderr.write(run.stdout + run.stderr)
                raise SystemExit("leg %s failed with status %d" % (leg, run.returncode))
            res[leg] = json.loads(run.stdout.strip().splitlines()[-1])["result"]
        line = json.dumps({"workload": "%d streams of %d windows x %d candidates, %d synthetic pieces, blocks of %s windows"
                           % (N_STREAMS, WINDOWS, CANDS, N_STREAMS, "/".join(map(str, BLOCKS))), "reps": args.reps,
                           "result": res}, sort_keys=True)
    else:
        if not args.leg:
            p.error("--leg or --all")
        from audio_sheet_retrieval_amd import _lib
        eng = _lib.Engine("mutopia_ccal_cont")
        res = leg_device(eng, args.reps) if args.leg == "device" else leg_host(eng, args.reps)
        eng.close()
        line = json.dumps({"leg": args.leg, "result": res}, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
