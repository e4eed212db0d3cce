#!/usr/bin/env python
"""Timing of staff-system detection (sheet_utils: OpticalMusicRecognizer.detect_systems_pages), one page set per
process:

    python tools/bench_omr.py --pages tutorial --cpu-baseline
    python tools/bench_omr.py --pages 1
    python tools/bench_omr.py --pages 16
    python tools/bench_omr.py --pages 64
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_omr.py --pages 16 --reps 1

Pages: the tutorial page (tests/golden/omr_tutorial_page.npz, 1181 x 835) or N seeded synthetic score-like pages of
the same size, uint8, with the reference's weights (tests/golden/omr_{system,bar}_params.npz).  End to end is the wall
clock of detect_systems_pages (upload, both networks, stitch, download, host post-processing) after a warm-up call,
median of --reps.  Device time per label comes from the library's event profiler (asr_profile_*): the U-Net chunks
and the stitch.  FLOP per page: direct-form 3x3 / transposed / 1x1 convolutions over every tile.  --cpu-baseline: one
page through the float32 CPU port of the same graph (tests/omr_ref.py: torch's CPU correlation for the 3x3 convs,
numpy for the rest) on 16 threads.  Prints one JSON line (also written to --out).

    python tools/bench_omr.py --pages tutorial --notes --bars
    python tools/bench_omr.py --pages 32 --notes --bars

--notes / --bars time the stage after the note / bar network's map exists instead (detect_stage below): one JSON line
per mode.  Without them the output is what it always was.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FP32_PEAK_TFLOPS = 157.3           # MI355X vector fp32


def synth_page(seed, h=1181, w=835):
    """a seeded score-like page: white, groups of five staff lines every 180 rows, note-like blobs, noise"""
    rng = np.random.default_rng(seed)
    p = np.full((h, w), 255, np.uint8)
    for top in range(100 + int(rng.integers(0, 20)), h - 100, 180):
        for k in range(5):
            p[top + 10 * k:top + 10 * k + 2, 40:w - 40] = 0
        for x in rng.integers(60, w - 60, size=w // 30):
            y = top + int(rng.integers(-10, 50))
            p[y:y + 8, x:x + 10] = 20
        p[top:top + 42, 40:42] = 0
        p[top:top + 42, w - 42:w - 40] = 0
    return np.clip(p.astype(int) + rng.integers(-6, 6, size=p.shape), 0, 255).astype(np.uint8)


def unet_flop(th, tw):
    plane = th * tw
    conv = [(1, 8, 0), (8, 8, 0), (8, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 2), (32, 64, 3), (64, 64, 3),
            (32, 32, 2), (32, 32, 2), (16, 16, 1), (16, 16, 1), (8, 8, 0), (8, 8, 0)]
    f = sum(2.0 * 9 * ci * co * (plane >> (2 * lv)) for ci, co, lv in conv)
    f += sum(2.0 * 4 * ci * co * (plane >> (2 * lv)) for ci, co, lv in [(64, 32, 3), (32, 16, 2), (16, 8, 1)])
    return f + 2.0 * 8 * plane


def detect_stage(a, pages, which):
    """--notes / --bars: the stage after the network's map exists, on the device (asr_notes_from_map_dev /
    asr_bars_from_map_dev + bars_from_stats, the maps where the network left them) and on the host (notes_from_map /
    bars_from_map on the same maps, downloaded once outside the timing) in the same process: median, minimum and
    maximum of --reps each after one warm-up, and that the two agree.  The host stage is the baseline."""
    from ctypes import c_void_p

    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import omr_ref
    params = {k: omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_%s_params.npz" % k)) for k in ("system", "bar", "note")}
    rec = build_recognizer(params["system"], params["bar"], note_params=params["note"])
    net = rec.note_detector if which == "notes" else rec.bar_detector
    eng = net.engine
    out, x, (_, _, sizes, _, hs, ws) = net.predict_pages_dev(pages, in_mode=O.IN_U8_RAW)
    eng.sync()
    flat = out.download((int(sizes.sum()),), np.float64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    maps = [flat[o:o + n].reshape(h, w) for o, n, h, w in zip(offs, sizes, hs, ws)]

    def device():
        if which == "notes":
            return [c for _, c in O.notes_from_map_dev(eng, c_void_p(out.ptr), hs, ws, seg=net.handle)]
        res, _ = O.bar_blobs_from_map_dev(eng, c_void_p(out.ptr), hs, ws, seg=net.handle)
        return [None if st is None else O.bars_from_stats(st) for _, st in res]

    def host():
        return [O.notes_from_map(m) if which == "notes" else O.bars_from_map(m) for m in maps]

    def timed(f):
        res = f()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            res = f()
            ts.append((time.perf_counter() - t) * 1e3)
        return res, {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}

    try:
        dev_res, dev_ms = timed(device)
        host_res, host_ms = timed(host)
    finally:
        out.free()
        if x is not None:
            x.free()
    h, w = pages[0].shape
    return {
        "what": "%s after the network's map exists, %s pages of %dx%d: device stage against the host stage on the same "
                "maps, same process" % (which, a.pages, h, w),
        "pages": len(pages),
        "device_stage_ms": dev_ms,
        "host_stage_ms": host_ms,
        "host_over_device": host_ms["median"] / dev_ms["median"],
        "undecided_on_device": int(sum(r is None for r in dev_res)),
        "equal": bool(all(d is not None and np.array_equal(d, hh) for d, hh in zip(dev_res, host_res))),
        "found": [int(len(r)) for r in host_res][:8],
        "reps": a.reps,
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pages", default="tutorial", help="'tutorial' or a number of synthetic pages")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--cpu-baseline", action="store_true")
    p.add_argument("--out", default=None)
    p.add_argument("--notes", action="store_true", help="time note-head detection after the map: device and host stage")
    p.add_argument("--bars", action="store_true", help="time bar detection after the map: device and host stage")
    a = p.parse_args()

    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import omr_ref

    ps = omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz"))
    pb = omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_bar_params.npz"))
    if a.pages == "tutorial":
        pages = [np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]]
    else:
        pages = [synth_page(1000 + i) for i in range(int(a.pages))]
    n = len(pages)
    if a.notes or a.bars:
        lines = [json.dumps(detect_stage(a, pages, which)) for which, on in (("notes", a.notes), ("bars", a.bars)) if on]
        print("\n".join(lines))
        if a.out:
            with open(a.out, "w") as fp:
                fp.write("\n".join(lines) + "\n")
        return
    rec = build_recognizer(ps, pb)
    eng = rec.system_detector.engine

    def run():
        return rec.detect_systems_pages(pages, in_mode=O.IN_U8_RAW)

    res = run()
    ts = []
    for _ in range(a.reps):
        t = time.perf_counter()
        res = run()
        ts.append(time.perf_counter() - t)
    wall = float(np.median(ts))

    # device time per label, one more call with the event profiler on
    eng.profile_enable(True)
    eng.profile_reset()
    rec.system_detector.predict_pages(pages, in_mode=O.IN_U8_RAW)
    rec.bar_detector.predict_pages(pages, in_mode=O.IN_U8_RAW)
    prof = {r["name"]: r for r in eng.profile()}
    eng.profile_enable(False)
    net_ms = prof.get("seg_unet", {}).get("total_ms", float("nan"))
    stitch_ms = prof.get("seg_stitch", {}).get("total_ms", float("nan"))

    # host post-processing alone, on the maps of the last call
    sm = rec.system_detector.predict_pages(pages, in_mode=O.IN_U8_RAW)
    bm = rec.bar_detector.predict_pages(pages, in_mode=O.IN_U8_RAW)
    t = time.perf_counter()
    for pg, s, b in zip(pages, sm, bm):
        try:
            O.systems_from_maps(O.prepare_image(pg), s, b)
        except Exception:
            pass
    host_ms = (time.perf_counter() - t) * 1e3

    h, w = pages[0].shape
    n_sys = len(O.tile_grid(h, w, 512, 512)[2]) * len(O.tile_grid(h, w, 512, 512)[3])
    n_bar = len(O.tile_grid(h, w, 256, 512)[2]) * len(O.tile_grid(h, w, 256, 512)[3])
    flop_page = n_sys * unet_flop(512, 512) + n_bar * unet_flop(256, 512)
    out = {
        "what": "staff-system detection, detect_systems_pages on %s pages of %dx%d (uint8, prepare on the device)"
                % (a.pages, h, w),
        "pages": n,
        "pages_per_s": n / wall,
        "end_to_end_ms_per_page": 1e3 * wall / n,
        "device_ms_per_page": {"networks": net_ms / n, "stitch": stitch_ms / n},
        "host_postprocess_ms_per_page": host_ms / n,
        "host_share_of_end_to_end": (host_ms / n) / (1e3 * wall / n),
        "tiles_per_page": {"system_512x512": n_sys, "bar_256x512": n_bar},
        "gflop_per_page_direct_form": flop_page / 1e9,
        "networks_share_of_fp32_peak": (flop_page * n / (net_ms * 1e-3)) / (FP32_PEAK_TFLOPS * 1e12),
        "systems_found": [int(r.shape[0]) if not isinstance(r, Exception) else None for r in res][:8],
        "reps": a.reps,
    }
    if a.cpu_baseline:
        import torch
        torch.set_num_threads(16)
        x = O.prepare_image(pages[0])
        t = time.perf_counter()
        sp = omr_ref.sliding_window(x, (512, 512), lambda tl: omr_ref.unet_forward(tl, ps, dtype=np.float32))
        bp = omr_ref.sliding_window(x, (256, 512), lambda tl: omr_ref.unet_forward(tl, pb, dtype=np.float32))
        try:
            O.systems_from_maps(x, sp, bp)
        except Exception:
            pass
        out["cpu_float32_port_16_threads_pages_per_s"] = 1.0 / (time.perf_counter() - t)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
