#!/usr/bin/env python
"""Page scans at 300 dpi inside a scanner's black frame, cropped on the device (asr_crop_estimate_dev,
asr_crop_pages_dev): what the stage adds to the scan route, what its kernels reach, what the host would take, and what
it does to the systems found on a framed page.

    python tools/bench_crop.py [--reps 5] [--pages 64] [--shape 3508x2480] [--host_pages 4]
                               [--out profiles/r31_crop.json]

N pages (uint8) of --shape: the tutorial page of tests/golden replicated to three times its size, cut to the paper's size
and set into a frame of 0-bytes of 111 / 156 rows and 123 / 87 columns (three times the frame of
tests/test_page_crop_host.py), in its four orientations.
    cropped_call    one DevicePages.cropped() on pages that are on the device (tables uploaded, the counts zeroed, two
                    launches, the rects downloaded, the output buffer allocated, one launch) and asr_sync - host clock
    kernels         crop_counts, crop_rects and crop_copy alone, from the library's event profiler (passes of their
                    own), each with its algorithmic bytes (counts: the three quarters of every page that lie in a band,
                    read once; rects: the counts read once; copy: every byte of the rects read once and written once):
                    GB/s and the share of the copy rate measured in the same session (tools/bench_live_track.copy_rate)
    route_with      DevicePages(raw pages).cropped().flattened().deskewed(64).resized(835): one upload, asr_sync
    route_without   DevicePages(raw pages).flattened().deskewed(64).resized(835): the route as it was, same process
    host            crop_page_host on --host_pages pages, scaled to N (it is linear in the pages); marked as scaled
    systems         the tutorial page (1181 x 835) in its frame (1270 x 905), straight and tilted by 30 / 1024, through the
                    real OMR weights on the device by the route [crop,] deskew, resize to 835: the system boxes with the
                    crop (at the default margin and at margin 0) and without, beside those of the clean page
Before anything is timed the rects and the cropped bytes of the first and the last page are compared with the host.
Medians of --reps with ranges.  Prints one JSON line.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODEL = "mutopia_ccal_cont"
FRAME = (111, 156, 123, 87)              # rows at the top and at the bottom, columns left and right
KERNELS = ("crop_counts", "crop_rects", "crop_copy")


def stats(times):
    return dict(median_ms=round(1e3 * float(np.median(times)), 3), min_ms=round(1e3 * min(times), 3),
                max_ms=round(1e3 * max(times), 3))


def tutorial_page():
    return np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]


def framed_pages(n, h, w):
    from test_page_crop_host import framed
    big = np.repeat(np.repeat(tutorial_page(), 3, axis=0), 3, axis=1)
    ph, pw = h - FRAME[0] - FRAME[1], w - FRAME[2] - FRAME[3]
    reps = (-(-ph // big.shape[0]), -(-pw // big.shape[1]))
    scan = framed(np.ascontiguousarray(np.tile(big, reps)[:ph, :pw]), FRAME)
    four = [np.ascontiguousarray(p) for p in (scan, scan[::-1], scan[:, ::-1], scan[::-1, ::-1])]
    return [four[i % 4] for i in range(n)]


def kernel_row(times, nbytes, copy_gbs):
    k = float(np.median(times))
    row = stats(times)
    row.update(bytes=nbytes, gb_per_s=round(nbytes / k / 1e9, 1), share_of_copy_rate=round(nbytes / k / 1e9 / copy_gbs, 4),
               least_ms_by_bytes=round(1e3 * nbytes / (copy_gbs * 1e9), 4))
    return row


def measure(eng, O, pages, args, copy_gbs):
    n = len(pages)
    raw = O.DevicePages(eng, pages)

    def cropped_call():
        out = raw.cropped()
        eng.sync()
        return out

    cut = cropped_call()
    rects = cut.rects.copy()
    for i in sorted({0, n - 1}):                                     # the same integers and bytes at the timed size
        want, status = O.crop_rect_host(pages[i])
        if tuple(rects[i].tolist()) != want or int(cut.crop_status[i]) != status or \
                not np.array_equal(cut.download_page(i), O.crop_page_host(pages[i])):
            raise SystemExit("device and host differ on page %d" % i)
    out_bytes = float(cut.nbytes)
    cut.free()
    t_call, t_k = [], {name: [] for name in KERNELS}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = cropped_call()
        t_call.append(time.perf_counter() - t0)
        out.free()
    eng.profile_enable(True)
    for _ in range(args.reps):
        eng.profile_reset()
        cropped_call().free()
        rec = {p["name"]: p for p in eng.profile()}
        for name in t_k:
            t_k[name].append(1e-3 * rec[name]["total_ms"])
    eng.profile_enable(False)
    eng.profile_reset()
    page_bytes = float(raw.nbytes)
    count_bytes = 4.0 * float(raw.heights.astype(np.int64).sum() + raw.widths.astype(np.int64).sum())
    raw.free()
    band_bytes = float(sum(p.size - 4 * (p.shape[0] // 4) * (p.shape[1] // 4) for p in pages))
    res = dict(pages=n, shape=list(pages[0].shape), frame=list(FRAME), rect=rects[0].tolist(), margin=O.crop_margin(pages[0].shape[1]),
               mb=round(page_bytes / 1e6, 1), cropped_call=stats(t_call),
               kernels=dict(crop_counts=kernel_row(t_k["crop_counts"], band_bytes, copy_gbs),
                            crop_rects=kernel_row(t_k["crop_rects"], count_bytes, copy_gbs),
                            crop_copy=kernel_row(t_k["crop_copy"], 2 * out_bytes, copy_gbs)))

    def route(crop):
        pages_dev = O.DevicePages(eng, pages)
        stages = ([lambda p: p.cropped()] if crop else []) + [lambda p: p.flattened(), lambda p: p.deskewed(64),
                                                              lambda p: p.resized(args.width)]
        for stage in stages:
            following = stage(pages_dev)
            pages_dev.free()
            pages_dev = following
        eng.sync()
        return pages_dev

    route(True).free()
    route(False).free()
    t_with, t_without = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        small = route(True)
        t_with.append(time.perf_counter() - t0)
        small.free()
        t0 = time.perf_counter()
        small = route(False)
        t_without.append(time.perf_counter() - t0)
        small.free()
    m = min(args.host_pages, n)
    t_host = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for p in pages[:m]:
            O.crop_page_host(p)
        t_host.append((time.perf_counter() - t0) * n / m)            # scaled to all pages
    host = stats(t_host)
    host.update(measured_on_pages=m, scaled_to_pages=n)
    res.update(route_with=stats(t_with), route_without=stats(t_without),
               stage_adds_ms=round(1e3 * (float(np.median(t_with)) - float(np.median(t_without))), 3),
               with_over_without=round(float(np.median(t_with)) / float(np.median(t_without)), 4), host=host,
               host_over_cropped_call=round(float(np.median(t_host)) / float(np.median(t_call)), 1))
    return res


def systems(O, width):
    """the system boxes the real weights find on the clean tutorial page and on the framed one, straight and tilted, by the
    route [crop,] deskew, resize - on the device"""
    import omr_ref
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    from test_page_crop_host import framed
    rec = build_recognizer(omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz")),
                           omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_bar_params.npz")))
    eng = rec.system_detector.engine
    clean = tutorial_page()
    scan = framed(clean)

    def boxes(page, crop, margin=None):
        pages_dev = O.DevicePages(eng, [page])
        out = {}
        stages = ([lambda p: p.cropped(margin=margin)] if crop else []) + [lambda p: p.deskewed(64), lambda p: p.resized(width)]
        for stage in stages:
            following = stage(pages_dev)
            pages_dev.free()
            pages_dev = following
            if hasattr(following, "rects"):
                out["rect"] = following.rects[0].tolist()
            if hasattr(following, "slopes"):
                out["slope"] = int(following.slopes[0])
        out["shape"] = [int(pages_dev.heights[0]), int(pages_dev.widths[0])]
        found = rec.detect_systems_pages([pages_dev.download_page(0)], in_mode=O.IN_U8_RAW, dev_pages=pages_dev)[0]
        pages_dev.free()
        if isinstance(found, Exception):
            out["error"] = repr(found)
            return out
        found = [np.asarray(s).astype(int) for s in found]
        out.update(systems=len(found), rows=[[int(s[:, 0].min()), int(s[:, 0].max())] for s in found],
                   columns=[[int(s[:, 1].min()), int(s[:, 1].max())] for s in found])
        return out

    tilted = O.shear_page_host(scan, 30, fill=0)
    return dict(clean=boxes(clean, False), framed_without=boxes(scan, False), framed_with=boxes(scan, True),
                framed_with_margin_0=boxes(scan, True, 0),
                tilted_without=boxes(tilted, False), tilted_with=boxes(tilted, True),
                tilted_with_margin_0=boxes(tilted, True, 0))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--shape", default="3508x2480", help="rows x columns of every page")
    ap.add_argument("--width", type=int, default=835)
    ap.add_argument("--host_pages", type=int, default=4, help="pages the host crop is measured on (scaled to --pages)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    from bench_live_track import copy_rate
    h, w = (int(v) for v in args.shape.split("x"))
    pages = framed_pages(args.pages, h, w)
    eng = _lib.Engine(MODEL, device=0)
    copy_gbs = copy_rate(eng)
    result = dict(tool="bench_crop", reps=args.reps, floor=O.CROP_FLOOR, share=O.CROP_SHARE,
                  copy_rate_gb_per_s=round(copy_gbs, 1), equal_with_the_host=True,
                  scan=measure(eng, O, pages, args, copy_gbs))
    eng.close()
    result["systems"] = systems(O, args.width)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
