#!/usr/bin/env python
"""The batched spectrogram: the direct DFT (asr_spectrogram_batch_dev, spectrogram_batch_kernel) against the FFT route
(asr_spectrogram_fft_batch_dev, spectrogram_fft_batch_kernel), in one process.

    python tools/bench_spectrogram.py [--reps 5] [--out profiles/r24_spectrogram_fft.json] [--cases 8x20@22050,...]

Per case (N recordings of S seconds at R Hz: seeded tones plus noise, float32; a rate other than 22050 goes through
asr_resample_batch_dev first, and the kernels are timed on the resampled audio where it lies on the device):
    kernel   both kernels alone, from the library's event profiler, alternating direct / fft, one warm-up pass, medians
             of --reps with [min - max]; for the FFT kernel the LDS bytes and floating-point operations of its plan, the
             rates they give and the least time each of the chip's bounds allows
    call     one call of either entry point on audio that is on the device (tables uploaded, kernel, synchronise) - host
             clock, alternating
    route    SpectrogramProcessor.process_many_dev (upload included, resampling where the rate asks for it) with
             dft="direct" and dft="fft" - host clock around work that ends in asr_sync, alternating
    deviation  each route's largest deviation from the float64 spectrogram of the same (resampled) samples: float64
             product of sample and float32 window, np.fft.rfft in float64, the filterbank in float64 with the float32
             weights, log10(1 + s) in float64
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
MODEL = "mutopia_ccal_cont"
SR = 22050
# MI355X_MICROARCH figures: LDS streaming with every CU busy, and the fp32 vector rate
LDS_READ_TBS, LDS_WRITE_TBS, FP32_VECTOR_TFLOPS = 150.0, 45.0, 157.0
# the plan of spectrogram_fft_batch_kernel per frame: five passes write and read 1024 complex values each, the post-pass
# reads 2 x 1024 complex values and writes 1024 magnitudes, the filterbank reads one magnitude per weight
FFT_LDS_WRITE = 5 * 8192 + 4096
FFT_LDS_READ_FIXED = 5 * 8192 + 16384
# operations: a pass has 16 real additions per butterfly and 3 complex products (6 each, none in the last pass); the
# post-pass 4 additions, a complex product, 2 more additions and the magnitude (4) per bin; the filterbank 2 per weight
FFT_FLOP_FIXED = 256 * (5 * 16 + 4 * 18) + 1024 * 16


def recordings(n, seconds, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * rate)) / float(rate)
    out = []
    for _ in range(n):
        x = sum(a * np.sin(2 * np.pi * f * t) for a, f in zip(rng.uniform(0.1, 0.3, 5), rng.uniform(60, 4000, 5)))
        out.append((x + 0.01 * rng.standard_normal(t.size)).astype(np.float32))
    return out


def stats(times):
    return dict(median_ms=round(1e3 * float(np.median(times)), 4), min_ms=round(1e3 * min(times), 4),
                max_ms=round(1e3 * max(times), 4))


def float64_spectrogram(samples, proc):
    """(num_bins, n_frames) float64 of one recording at the processor's rate"""
    n = proc.num_frames(samples.size)
    starts = (np.arange(n, dtype=np.float64) * proc.hop).astype(np.int64)
    x = np.concatenate([samples.astype(np.float64), np.zeros(proc.frame_size)])
    fr = x[starts[:, None] + np.arange(proc.frame_size)[None, :]] * proc.window.astype(np.float64)[None, :]
    mag = np.abs(np.fft.rfft(fr, axis=1))[:, :proc.frame_size // 2]
    out, off = np.zeros((proc.num_bins, n)), 0
    for f in range(proc.num_bins):
        b0, ln = int(proc.fb_start[f]), int(proc.fb_len[f])
        out[f] = mag[:, b0:b0 + ln] @ proc.fb_w[off:off + ln].astype(np.float64)
        off += ln
    return np.log10(1.0 + out)


def run_case(eng, procs, n, seconds, rate, reps):
    from audio_sheet_retrieval_amd.audio_frontend import resample_plan
    proc = procs["direct"]
    recs = recordings(n, seconds, rate, seed=rate + n)
    in_counts = np.asarray([r.size for r in recs], np.int64)
    in_off = np.concatenate([[0], np.cumsum(in_counts)[:-1]]).astype(np.int64)
    if rate == SR:
        counts, s_off = in_counts, in_off
        d_samples = eng.alloc(int(counts.sum()) * 4).upload(np.concatenate(recs))
    else:                                                       # the audio the spectrogram launch reads: resampled in place
        up, down, half, taps = resample_plan(rate)
        counts = -(-in_counts * up // down)
        s_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        d_native = eng.alloc(int(in_counts.sum()) * 4).upload(np.concatenate(recs))
        d_samples = eng.alloc(int(counts.sum()) * 4)
        eng.resample_batch_dev(d_native.ptr, int(in_counts.sum()), in_off, in_counts, s_off, counts, up, down, taps, half,
                               False, d_samples.ptr, int(counts.sum()))
        d_native.free()
    n_samples = int(counts.sum())
    frames = np.asarray([proc.num_frames(int(c)) for c in counts], np.int64)
    o_off = np.concatenate([[0], np.cumsum(frames * proc.num_bins)[:-1]]).astype(np.int64)
    total, out_floats = int(frames.sum()), int(frames.sum()) * proc.num_bins
    d_out = eng.alloc(out_floats * 4)
    calls = {"direct": eng.spectrogram_batch_dev, "fft": eng.spectrogram_fft_batch_dev}
    labels = {"direct": "spectrogram_batch", "fft": "spectrogram_fft_batch"}

    def call(which):
        calls[which](d_samples.ptr, n_samples, s_off, counts, frames, o_off, proc.frame_size, proc.hop, proc.window,
                     proc.fb_start, proc.fb_len, proc.fb_w, d_out.ptr, out_floats, transposed=True)
        eng.sync()

    def route(which):
        dev = procs[which].process_many_dev(recs, None, sample_rates=[rate] * n)
        eng.sync()
        return dev

    # the float64 yardstick of the samples the launch reads, and each route's deviation from it (also the warm-up)
    flat = d_samples.download((n_samples,), np.float32)
    ref = np.concatenate([float64_spectrogram(flat[o:o + c], proc).ravel() for o, c in zip(s_off, counts)])
    deviation = {}
    for which in ("direct", "fft"):
        call(which)
        from_call = d_out.download((out_floats,), np.float32)
        dev = route(which)
        from_route = dev.buf.download((out_floats,), np.float32)
        dev.buf.free()
        if not np.array_equal(from_call, from_route):
            raise SystemExit("%s: the call and the route differ at %d x %g s @ %d Hz" % (which, n, seconds, rate))
        deviation[which] = float(np.abs(from_route.astype(np.float64) - ref).max())

    t_call, t_route, t_kernel = ({"direct": [], "fft": []} for _ in range(3))
    for _ in range(reps):
        for which in ("direct", "fft"):
            t0 = time.perf_counter()
            call(which)
            t_call[which].append(time.perf_counter() - t0)
    for _ in range(reps):
        for which in ("direct", "fft"):
            t0 = time.perf_counter()
            dev = route(which)
            t_route[which].append(time.perf_counter() - t0)
            dev.buf.free()
    eng.profile_enable(True)
    for rep in range(reps + 1):                                 # pass 0 warms the profiled path
        for which in ("direct", "fft"):
            eng.profile_reset()
            call(which)
            rec = [p for p in eng.profile() if p["name"] == labels[which]]
            if rep:
                t_kernel[which].append(1e-3 * rec[0]["total_ms"] / rec[0]["launches"])
    eng.profile_enable(False)
    eng.profile_reset()
    d_samples.free()
    d_out.free()

    weights = int(proc.fb_len.sum())
    max_bin = int((proc.fb_start + proc.fb_len).max())
    k_direct, k_fft = float(np.median(t_kernel["direct"])), float(np.median(t_kernel["fft"]))
    direct = stats(t_kernel["direct"])
    direct.update(operations=4.0 * proc.frame_size * max_bin * total,
                  tflop_per_s=round(4.0 * proc.frame_size * max_bin * total / k_direct / 1e12, 2))
    lds_r, lds_w = (FFT_LDS_READ_FIXED + 4.0 * weights) * total, float(FFT_LDS_WRITE) * total
    flop = (FFT_FLOP_FIXED + 2.0 * weights) * total
    least_lds = lds_r / (LDS_READ_TBS * 1e12) + lds_w / (LDS_WRITE_TBS * 1e12)
    fft = stats(t_kernel["fft"])
    fft.update(operations=flop, gflop_per_s=round(flop / k_fft / 1e9, 1), lds_bytes_read=lds_r, lds_bytes_written=lds_w,
               lds_tb_per_s=round((lds_r + lds_w) / k_fft / 1e12, 2), least_ms_by_lds=round(1e3 * least_lds, 4),
               least_ms_by_operations=round(1e3 * flop / (FP32_VECTOR_TFLOPS * 1e12), 5),
               share_of_lds_bound=round(least_lds / k_fft, 4),
               gemm_form_least_ms=round(1e3 * 4.0 * proc.frame_size * max_bin * total / (FP32_VECTOR_TFLOPS * 1e12), 4),
               median_below_direct_min=bool(k_fft < min(t_kernel["direct"])))
    r_direct, r_fft = float(np.median(t_route["direct"])), float(np.median(t_route["fft"]))
    return dict(recordings=n, seconds=seconds, rate=rate, frames=total, samples=n_samples,
                kernel=dict(direct=direct, fft=fft, direct_over_fft=round(k_direct / k_fft, 2)),
                call=dict(direct=stats(t_call["direct"]), fft=stats(t_call["fft"])),
                route=dict(direct=stats(t_route["direct"]), fft=stats(t_route["fft"]),
                           direct_over_fft=round(r_direct / r_fft, 3), fft_not_above_direct=bool(r_fft <= r_direct),
                           fft_kernel_share_of_route=round(k_fft / r_fft, 4),
                           direct_kernel_share_of_route=round(k_direct / r_direct, 4)),
                max_abs_deviation_from_float64=deviation)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="8x20@22050,32x20@22050,8x20@44100,32x20@44100",
                    help="N x seconds @ rate, comma separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_spectrogram_fft.json"),
                    help="the JSON is also written here")
    args = ap.parse_args(argv)
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    eng = _lib.Engine(MODEL, device=0)
    procs = {"direct": SpectrogramProcessor(eng), "fft": SpectrogramProcessor(eng, dft="fft")}
    cases = []
    for spec in args.cases.split(","):
        shape, rate = spec.split("@")
        n, seconds = shape.split("x")
        cases.append(run_case(eng, procs, int(n), float(seconds), int(rate), args.reps))
    eng.close()
    result = dict(tool="bench_spectrogram", reps=args.reps, lds_read_tb_per_s=LDS_READ_TBS,
                  lds_write_tb_per_s=LDS_WRITE_TBS, fp32_vector_tflops=FP32_VECTOR_TFLOPS, cases=cases)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
