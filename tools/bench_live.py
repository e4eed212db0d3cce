#!/usr/bin/env python
"""Timing of the streamed audio front-end (audio_frontend.AudioStream, asr_audio_stream_push_dev): one push of 50 ms
(one frame's worth of samples), of 250 ms (five frames' worth) and of 1 s, for 1 and 16 parallel streams at 22.05, 44.1
and 48 kHz, in the steady state (one second of audio has gone before).

    python tools/bench_live.py --out profiles/r22_live.json

Per case, medians of --reps with ranges:
    push_s      AudioStream.push(blocks): upload of the blocks, one asr_audio_stream_push_dev call, download of the columns
    caller_s    what a caller could do without the call: the host keeps, per stream, the inputs from the last multiple
                of `down` at or below the first input the next frame reads (so that the resampler's phases line up), and
                every block is: upload of [tail | block] of all streams, asr_resample_batch_dev, asr_spectrogram_batch_dev
                with every new frame as a one-frame recording at its own offset, download of the new columns.  The bench
                checks that both routes give the same bits.
    frames_ms / carry_ms   device time of the two kernels per push (library profile scopes, event timed)
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
    """the route without asr_audio_stream_push_dev: tails on the host, whole-recording calls on [tail | block]"""

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
            self.eng.spectrogram_batch_dev(d_y.ptr, int(y_cnt.sum()), f_off, [F] * k, [1] * k, np.arange(k) * nb, F, p.hop,
                                           p.window, p.fb_start, p.fb_len, p.fb_w, d_out.ptr, k * nb, transposed=False)
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


def run_case(proc, n_streams, rate, block_ms, reps, rng):
    eng = proc.engine
    block = int(round(rate * block_ms / 1000.0))
    lead = int(LEAD_S * rate)
    total = lead + (reps + 1) * block
    recs = [(0.3 * rng.standard_normal(total)).astype(np.float32) for _ in range(n_streams)]
    stream, caller = proc.stream(n_streams, rate), Caller(proc, n_streams, rate)
    try:
        stream.push([r[:lead] for r in recs])
        caller.push([r[:lead] for r in recs])
        t_push, t_call, frames = [], [], 0
        for k in range(reps + 1):                                       # the first round warms both routes up
            blocks = [r[lead + k * block:lead + (k + 1) * block] for r in recs]
            if k == 1:
                eng.profile_enable(True)
                eng.profile_reset()
            t0 = time.perf_counter()
            got = stream.push(blocks)
            t1 = time.perf_counter()
            if k >= 1:
                t_push.append(t1 - t0)
                frames += sum(g.shape[1] for g in got)
            if k == reps:
                frames_ms, carry_ms = _scope_ms(eng, "audio_stream_frames"), _scope_ms(eng, "audio_stream_carry")
                eng.profile_enable(False)
            t0 = time.perf_counter()
            want = caller.push(blocks)
            t1 = time.perf_counter()
            if k >= 1:
                t_call.append(t1 - t0)
            for g, w in zip(got, want):
                assert g.shape == w.shape and np.array_equal(g, w), "the two routes differ"
    finally:
        stream.close()
        caller.close()
    res = {"streams": n_streams, "rate": rate, "block_ms": block_ms, "block_samples": block,
           "frames_per_push": frames / float(reps), "state_floats_per_stream": stream.state_cap,
           "frames_ms": frames_ms / reps, "carry_ms": carry_ms / reps}
    res["push_s"], res["push_range_s"] = _stats(t_push)
    res["caller_s"], res["caller_range_s"] = _stats(t_call)
    res["caller_over_push"] = res["caller_s"] / res["push_s"]
    res["device_share_of_push"] = 1e-3 * (res["frames_ms"] + res["carry_ms"]) / res["push_s"]
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    eng = _lib.Engine("mutopia_ccal_cont")
    proc = SpectrogramProcessor(eng)
    rng = np.random.default_rng(22)
    cases = []
    for n in STREAMS:
        for rate in RATES:
            for ms in BLOCKS_MS:
                cases.append(run_case(proc, n, rate, ms, args.reps, rng))
                sys.stderr.write(json.dumps(cases[-1], sort_keys=True) + "\n")
                sys.stderr.flush()
    eng.close()
    native = {(c["streams"], c["block_ms"]): c for c in cases if c["rate"] == 22050}
    for c in cases:
        ref = native[(c["streams"], c["block_ms"])]
        if c["rate"] != 22050 and c["frames_per_push"] == ref["frames_per_push"] and c["frames_ms"] > 0:
            c["resample_share_of_frame_kernel"] = 1.0 - ref["frames_ms"] / c["frames_ms"]
    line = json.dumps({"workload": "steady-state pushes after %.0f s of audio, frames of %d at %d fps" %
                       (LEAD_S, proc.frame_size, proc.fps), "reps": args.reps, "cases": cases}, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
