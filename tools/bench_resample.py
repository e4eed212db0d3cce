#!/usr/bin/env python
"""Recordings at 44.1 / 48 kHz to spectrograms: the device resampler (asr_resample_batch_dev) against the route a
caller had before it - scipy.signal.resample_poly with the same taps on the host, then process_many_dev.

    python tools/bench_resample.py [--reps 5] [--out profiles/r16_resample.json] [--cases 32x20@44100,32x20@48000,1x600@44100]

Per case (N recordings of S seconds at R Hz: seeded tones plus noise, float32):
    resample_call   one asr_resample_batch_dev call on audio that is on the device (tables and taps uploaded, kernel,
                    synchronise) - host clock
    device_route    process_many_dev(sample_rates=...): upload at the native rate, resample, spectrogram launch, asr_sync
    host_route      resample_poly per recording on the host, then process_many_dev on the result, asr_sync; the share of
                    the host resampler is reported with it
    kernel          the resampling kernel alone, from the library's event profiler (passes of their own), with its
                    algorithmic bytes 4 (n_in + n_out) and operations 2 T n_out: rates, the least time each bound allows
                    and which of the two is the larger
Before anything is timed the device result is compared with audio_frontend.resample_host at the timed size, bit for bit,
and the spectrograms of the two routes are compared (they differ where the float64 sums of scipy and of the definition
round differently; the largest difference is reported).  Every shape is warmed first; medians of --reps with ranges.
Prints one JSON line.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_GBS = 6290.0                # measured float4 copy rate of the MI355X (8000 GB/s on the data sheet)
FP64_VECTOR_TFLOPS = 78.6        # data sheet, counting a fused multiply-add as two operations
MODEL = "mutopia_ccal_cont"


def recordings(n, seconds, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * rate)) / float(rate)
    out = []
    for _ in range(n):
        x = sum(a * np.sin(2 * np.pi * f * t) for a, f in zip(rng.uniform(0.1, 0.3, 5), rng.uniform(60, 4000, 5)))
        out.append((x + 0.01 * rng.standard_normal(t.size)).astype(np.float32))
    return out


def stats(times):
    return dict(median_ms=round(1e3 * float(np.median(times)), 3), min_ms=round(1e3 * min(times), 3),
                max_ms=round(1e3 * max(times), 3))


def run_case(eng, proc, n, seconds, rate, reps):
    from scipy import signal
    from audio_sheet_retrieval_amd.audio_frontend import resample_host, resample_plan
    recs = recordings(n, seconds, rate, seed=rate + n)
    up, down, half, taps = resample_plan(rate)
    T = taps.shape[1]
    h = taps.T.ravel()[:2 * half + 1]
    in_counts = np.asarray([r.size for r in recs], np.int64)
    out_counts = -(-in_counts * up // down)
    in_off = np.concatenate([[0], np.cumsum(in_counts)[:-1]]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(out_counts)[:-1]]).astype(np.int64)
    n_in, n_out = int(in_counts.sum()), int(out_counts.sum())
    d_in = eng.alloc(n_in * 4).upload(np.concatenate(recs))
    d_out = eng.alloc(n_out * 4)

    def resample_call():
        eng.resample_batch_dev(d_in.ptr, n_in, in_off, in_counts, out_off, out_counts, up, down, taps, half, False,
                               d_out.ptr, n_out)
        eng.sync()

    def device_route():
        dev = proc.process_many_dev(recs, None, sample_rates=[rate] * n)
        eng.sync()
        return dev

    def host_route():
        t0 = time.perf_counter()
        host = [signal.resample_poly(r, up, down, window=h / up).astype(np.float32) for r in recs]
        t1 = time.perf_counter()
        dev = proc.process_many_dev(host)
        eng.sync()
        return dev, t1 - t0

    def download(dev):
        total = sum(r * c for r, c in dev.shapes)
        flat = dev.buf.download((total,), np.float32)
        dev.buf.free()
        return flat

    # the same results at the timed size, and the warm-up of every shape
    resample_call()
    got = d_out.download((n_out,), np.float32)
    for r, o, c in zip(recs, out_off, out_counts):
        if not np.array_equal(got[o:o + c], resample_host(r, rate)):
            raise SystemExit("device and resample_host differ at %d x %g s @ %d Hz" % (n, seconds, rate))
    spec_dev = download(device_route())
    spec_host = download(host_route()[0])
    spec_diff = float(np.abs(spec_dev - spec_host).max())

    t_call, t_dev, t_host, t_host_resample, t_kernel = [], [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        resample_call()
        t_call.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        dev = device_route()
        t_dev.append(time.perf_counter() - t0)
        dev.buf.free()
        t0 = time.perf_counter()
        dev, t_res = host_route()
        t_host.append(time.perf_counter() - t0)
        t_host_resample.append(t_res)
        dev.buf.free()
    eng.profile_enable(True)
    for _ in range(reps):
        eng.profile_reset()
        resample_call()
        rec = [p for p in eng.profile() if p["name"] == "resample_batch"]
        t_kernel.append(1e-3 * rec[0]["total_ms"] / rec[0]["launches"])
    eng.profile_enable(False)
    eng.profile_reset()
    d_in.free()
    d_out.free()

    k = float(np.median(t_kernel))
    nbytes, ops = 4.0 * (n_in + n_out), 2.0 * T * n_out
    t_bytes = nbytes / (COPY_GBS * 1e9)
    t_ops = ops / (0.5 * FP64_VECTOR_TFLOPS * 1e12)        # multiplies and adds are separate instructions: half the rate
    kernel = stats(t_kernel)
    kernel.update(bytes=nbytes, operations=ops, gb_per_s=round(nbytes / k / 1e9, 1),
                  share_of_copy_rate=round(nbytes / k / 1e9 / COPY_GBS, 4), gflop_per_s=round(ops / k / 1e9, 1),
                  least_ms_by_bytes=round(1e3 * t_bytes, 4), least_ms_by_operations=round(1e3 * t_ops, 4),
                  bound_by="operations" if t_ops > t_bytes else "bytes",
                  share_of_bound=round(max(t_ops, t_bytes) / k, 4))
    call = stats(t_call)
    call["kernel_share_of_call"] = round(k / float(np.median(t_call)), 4)
    host = stats(t_host)
    host["host_resample"] = stats(t_host_resample)
    return dict(recordings=n, seconds=seconds, rate=rate, up=up, down=down, taps_per_phase=T, n_in=n_in, n_out=n_out,
                bit_equal_with_resample_host=True, spectrogram_max_abs_diff_between_routes=spec_diff,
                resample_call=call, device_route=stats(t_dev), host_route=host, kernel=kernel,
                host_over_device=round(float(np.median(t_host)) / float(np.median(t_dev)), 2))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="32x20@44100,32x20@48000,1x600@44100", help="N x seconds @ rate, comma separated")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.audio_frontend import RESAMPLE_TILE, SpectrogramProcessor
    eng = _lib.Engine(MODEL, device=0)
    proc = SpectrogramProcessor(eng)
    cases = []
    for spec in args.cases.split(","):
        shape, rate = spec.split("@")
        n, seconds = shape.split("x")
        cases.append(run_case(eng, proc, int(n), float(seconds), int(rate), args.reps))
    eng.close()
    result = dict(tool="bench_resample", reps=args.reps, tile=RESAMPLE_TILE, copy_rate_gb_per_s=COPY_GBS,
                  fp64_vector_tflops=FP64_VECTOR_TFLOPS, cases=cases)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
