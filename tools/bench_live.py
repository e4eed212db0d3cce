#!/usr/bin/env python
"""Timing of the streamed audio front-end (audio_frontend.AudioStream, asr_audio_stream_push_dev): one push of 50 ms
(one frame's worth of samples), of 250 ms (five frames' worth) and of 1 s, for 1 and 16 parallel streams at 22.05, 44.1
and 48 kHz, in the steady state (one second of audio has gone before).

    python tools/bench_live.py --out profiles/r22_live.json
    python tools/bench_live.py --dft both --out profiles/r27_live_fft.json

--dft direct (default) times the direct-DFT stream, --dft fft the FFT stream of a SpectrogramProcessor(dft="fft")
(asr_audio_stream_push_fft_dev), --dft both the two in one process on the same blocks, alternating push by push, so that
the direct stream is the yardstick of the same session; a case then holds one block of figures per route ("direct",
"fft") and fft_over_direct_push / fft_over_direct_frames, the FFT stream's push time and frame-kernel time as fractions
of the direct stream's.

Per case, medians of --reps with ranges:
    push_s      AudioStream.push(blocks): upload of the blocks, one asr_audio_stream_push_dev call, download of the columns
    caller_s    what a caller could do without the call: the host keeps, per stream, the inputs from the last multiple
                of `down` at or below the first input the next frame reads (so that the resampler's phases line up), and
                every block is: upload of [tail | block] of all streams, asr_resample_batch_dev, asr_spectrogram_batch_dev
                with every new frame as a one-frame recording at its own offset, download of the new columns.  The bench
                checks that both routes give the same bits.
    frames_ms / carry_ms   device time of the two kernels per push (library profile scopes audio_stream_frames or
                audio_stream_fft_frames, and audio_stream_carry; event timed)
Derived: resample_share = 1 - frames_ms(22.05 kHz) / frames_ms(rate) for the same number of frames - the native-rate kernel
does everything but the resampling - and device_share = (frames_ms + carry_ms) / push time: a small one means the push is
bound by the fixed costs of the call (copies, launches, the synchronisation), not by the kernels.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATES = (22050, 44100, 48000)
STREAMS = (1, 16)
BLOCKS_MS = (50, 250, 1000)
LEAD_S = 1.0


def _stats(ts):
    return float(np.median(ts)), [float(min(ts)), float(max(ts))]


def _scope_ms(eng, name):
    return sum(r["total_ms"] for r in eng.profile() if r["name"] == name)


class Caller(object):
    """the route without asr_audio_stream_push_dev: tails on the host, whole-recording calls on [tail | block] (the
    batched spectrogram call of the processor's dft)"""

    def __init__(self, proc, n_streams, rate):
        from audio_sheet_retrieval_amd import audio_frontend as af
        self.af, self.p, self.eng, self.n = af, proc, proc.engine, n_streams
        if rate == proc.sample_rate:
            self.up, self.down, self.half, self.taps, self.T = 1, 1, 0, None, 0
        else:
            self.up, self.down, self.half, self.taps = af.resample_plan(rate)
            self.T = self.taps.shape[1]
        self.n_in = [0] * n_streams
        self.tails = [np.zeros(0, np.float32) for _ in range(n_streams)]
        self.tail_from = [0] * n_streams
        self.bufs = {}

    def _buf(self, name, nbytes):
        b = self.bufs.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self.bufs[name] = self.eng.alloc(max(4, int(nbytes)))
        return b

    def push(self, blocks):
        p, af = self.p, self.af
        F, nb = p.frame_size, p.num_bins
        xs, plans = [], []
        for s, b in enumerate(blocks):
            xs.append(np.concatenate((self.tails[s], b)))
            plans.append(af.audio_stream_plan(self.n_in[s], b.size, False, F, p.hop, self.up, self.down, self.half, self.T))
        x_cnt = np.asarray([x.size for x in xs], np.int64)
        x_off = np.concatenate([[0], np.cumsum(x_cnt)[:-1]]).astype(np.int64)
        y_cnt = -(-x_cnt * self.up // self.down)
        y_off = np.concatenate([[0], np.cumsum(y_cnt)[:-1]]).astype(np.int64)
        flat = np.concatenate(xs)
        d_y = self._buf("y", int(y_cnt.sum()) * 4)
        if self.taps is None:
            d_y.upload(flat)
        else:
            d_x = self._buf("x", flat.nbytes).upload(flat)
            self.eng.resample_batch_dev(d_x.ptr, flat.size, x_off, x_cnt, y_off, y_cnt, self.up, self.down, self.taps,
                                        self.half, False, d_y.ptr, int(y_cnt.sum()))
        f_off, owner = [], []
        for s, (first, new, keep) in enumerate(plans):
            y0 = self.tail_from[s] * self.up // self.down               # tail_from is a multiple of down
            for i in range(first, first + new):
                f_off.append(int(y_off[s]) + int(float(i) * p.hop) - y0)
                owner.append(s)
        k = len(f_off)
        cols = [np.zeros((nb, 0), np.float32)] * self.n
        if k:
            d_out = self._buf("out", k * nb * 4)
            p._batch_call()(d_y.ptr, int(y_cnt.sum()), f_off, [F] * k, [1] * k, np.arange(k) * nb, F, p.hop, p.window,
                            p.fb_start, p.fb_len, p.fb_w, d_out.ptr, k * nb, transposed=False)
            out = d_out.download((k, nb), np.float32)
            owner = np.asarray(owner)
            cols = [np.ascontiguousarray(out[owner == s].T) for s in range(self.n)]
        for s, (first, new, keep) in enumerate(plans):
            self.n_in[s] += blocks[s].size
            start = keep // self.down * self.down
            self.tails[s] = xs[s][start - self.tail_from[s]:]
            self.tail_from[s] = start
        return cols

    def close(self):
        for b in self.bufs.values():
            b.free()


FRAME_SCOPE = {"direct": "audio_stream_frames", "fft": "audio_stream_fft_frames"}


def run_case(procs, n_streams, rate, block_ms, reps, rng):
    """procs: {"direct": processor, "fft": processor} or one of the two - the routes of a round push the same blocks one
    after the other, each followed by its caller route"""
    eng = next(iter(procs.values())).engine
    block = int(round(rate * block_ms / 1000.0))
    lead = int(LEAD_S * rate)
    total = lead + (reps + 1) * block
    recs = [(0.3 * rng.standard_normal(total)).astype(np.float32) for _ in range(n_streams)]
    streams = {d: p.stream(n_streams, rate, dft="fft" if d == "fft" else None) for d, p in procs.items()}
    callers = {d: Caller(p, n_streams, rate) for d, p in procs.items()}
    t_push, t_call = {d: [] for d in procs}, {d: [] for d in procs}
    dev = {d: {"frames_ms": 0.0, "carry_ms": 0.0} for d in procs}
    frames = 0
    try:
        for d in procs:
            streams[d].push([r[:lead] for r in recs])
            callers[d].push([r[:lead] for r in recs])
        for k in range(reps + 1):                                       # the first round warms every route up
            blocks = [r[lead + k * block:lead + (k + 1) * block] for r in recs]
            for d in procs:
                if k >= 1:
                    eng.profile_enable(True)
                    eng.profile_reset()
                t0 = time.perf_counter()
                got = streams[d].push(blocks)
                t1 = time.perf_counter()
                if k >= 1:
                    t_push[d].append(t1 - t0)
                    dev[d]["frames_ms"] += _scope_ms(eng, FRAME_SCOPE[d])
                    dev[d]["carry_ms"] += _scope_ms(eng, "audio_stream_carry")
                    eng.profile_enable(False)
                t0 = time.perf_counter()
                want = callers[d].push(blocks)
                t1 = time.perf_counter()
                if k >= 1:
                    t_call[d].append(t1 - t0)
                for g, w in zip(got, want):
                    assert g.shape == w.shape and np.array_equal(g, w), "the two routes differ (%s)" % d
            if k >= 1:
                frames += sum(g.shape[1] for g in got)
    finally:
        for d in procs:
            streams[d].close()
            callers[d].close()
    res = {"streams": n_streams, "rate": rate, "block_ms": block_ms, "block_samples": block,
           "frames_per_push": frames / float(reps), "state_floats_per_stream": next(iter(streams.values())).state_cap}
    routes = {}
    for d in procs:
        r = routes[d] = {"frames_ms": dev[d]["frames_ms"] / reps, "carry_ms": dev[d]["carry_ms"] / reps}
        r["push_s"], r["push_range_s"] = _stats(t_push[d])
        r["caller_s"], r["caller_range_s"] = _stats(t_call[d])
        r["caller_over_push"] = r["caller_s"] / r["push_s"]
        r["device_share_of_push"] = 1e-3 * (r["frames_ms"] + r["carry_ms"]) / r["push_s"]
    if len(routes) == 1:                                                # one route: the flat case of round 22
        res.update(next(iter(routes.values())))
    else:
        res.update(routes)
        res["fft_over_direct_push"] = routes["fft"]["push_s"] / routes["direct"]["push_s"]
        if routes["direct"]["frames_ms"] > 0:
            res["fft_over_direct_frames"] = routes["fft"]["frames_ms"] / routes["direct"]["frames_ms"]
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    p.add_argument("--dft", choices=("direct", "fft", "both"), default="direct",
                   help="the stream to time: the direct DFT, the FFT, or both alternating in one process")
    args = p.parse_args()
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    eng = _lib.Engine("mutopia_ccal_cont")
    which = ("direct", "fft") if args.dft == "both" else (args.dft,)
    procs = {d: SpectrogramProcessor(eng, dft=d) for d in which}
    proc = procs[which[0]]
    rng = np.random.default_rng(22)
    cases = []
    for n in STREAMS:
        for rate in RATES:
            for ms in BLOCKS_MS:
                cases.append(run_case(procs, n, rate, ms, args.reps, rng))
                sys.stderr.write(json.dumps(cases[-1], sort_keys=True) + "\n")
                sys.stderr.flush()
    eng.close()
    native = {(c["streams"], c["block_ms"]): c for c in cases if c["rate"] == 22050}
    for c in cases:
        ref = native[(c["streams"], c["block_ms"])]
        if c["rate"] == 22050 or c["frames_per_push"] != ref["frames_per_push"]:
            continue
        for blk, rblk in ([(c, ref)] if len(which) == 1 else [(c[d], ref[d]) for d in which]):
            if blk["frames_ms"] > 0:
                blk["resample_share_of_frame_kernel"] = 1.0 - rblk["frames_ms"] / blk["frames_ms"]
    line = json.dumps({"workload": "steady-state pushes after %.0f s of audio, frames of %d at %d fps" %
                       (LEAD_S, proc.frame_size, proc.fps), "reps": args.reps, "dft": args.dft, "cases": cases},
                      sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
