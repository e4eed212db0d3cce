#!/usr/bin/env python
"""Shaded page scans at 300 dpi flattened on the device (asr_flatten_pages_dev): what the stage adds to the scan route,
what its kernels reach, what the host would take, and what it does to the systems found on a shaded page.

    python tools/bench_flatten.py [--reps 5] [--pages 64] [--shape 3508x2480] [--host_pages 4]
                                  [--out profiles/r29_flatten.json]

N pages (uint8): the tutorial page of tests/golden replicated to three times its size and cut to --shape, under the
shade of tests/test_page_flatten_host.py (a spine shadow and a gradient), in its four orientations.
    flatten_call    one DevicePages.flattened() on pages that are on the device (tables uploaded, two launches, the
                    output buffer allocated) and asr_sync - host clock
    kernels         flatten_dilate and flatten_erode alone, from the library's event profiler (passes of their own), each
                    with its algorithmic bytes (dilate: every page byte read once, every byte of D written once; erode:
                    D and the page read once, the result written once): GB/s and the share of the copy rate measured in
                    the same session (tools/bench_live_track.copy_rate).  A tile's halo is read from cache more than
                    once; those reads are not bytes of this count.
    route_with      DevicePages(raw pages).flattened().deskewed(64).resized(835): one upload, asr_sync
    route_without   DevicePages(raw pages).deskewed(64).resized(835): the route as it was, in the same process
    host            flatten_page_host on --host_pages pages, scaled to N (it is linear in the pages); marked as scaled
    systems         the shaded tutorial page (1181 x 835) through the real OMR weights on the device: the system boxes of
                    the clean page, of the shaded page, and of the shaded page after the stage
Before anything is timed the flattened bytes of the first and the last page are compared with the host.  Medians of
--reps with ranges.  Prints one JSON line.  Needs a GPU.
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


def stats(times):
    return dict(median_ms=round(1e3 * float(np.median(times)), 3), min_ms=round(1e3 * min(times), 3),
                max_ms=round(1e3 * max(times), 3))


def tutorial_page():
    return np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]


def shaded_pages(n, h, w):
    from test_page_flatten_host import shaded
    big = np.repeat(np.repeat(tutorial_page(), 3, axis=0), 3, axis=1)
    reps = (-(-h // big.shape[0]), -(-w // big.shape[1]))
    dark = shaded(np.ascontiguousarray(np.tile(big, reps)[:h, :w]))
    four = [np.ascontiguousarray(p) for p in (dark, dark[::-1], dark[:, ::-1], dark[::-1, ::-1])]
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

    def flatten_call():
        out = raw.flattened()
        eng.sync()
        return out

    flat = flatten_call()
    radii = flat.radii.tolist()
    for i in sorted({0, n - 1}):                                     # the same bytes at the timed size
        if not np.array_equal(flat.download_page(i), O.flatten_page_host(pages[i])):
            raise SystemExit("device and host differ on page %d" % i)
    flat.free()
    t_call, t_k = [], {"flatten_dilate": [], "flatten_erode": []}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = flatten_call()
        t_call.append(time.perf_counter() - t0)
        out.free()
    eng.profile_enable(True)
    for _ in range(args.reps):
        eng.profile_reset()
        flatten_call().free()
        rec = {p["name"]: p for p in eng.profile()}
        for name in t_k:
            t_k[name].append(1e-3 * rec[name]["total_ms"])
    eng.profile_enable(False)
    eng.profile_reset()
    page_bytes = float(raw.nbytes)
    d_bytes = float(sum((int(h) + 2 * r) * (int(w) + 2 * r) for h, w, r in zip(raw.heights, raw.widths, radii)))
    raw.free()
    both = [a + b for a, b in zip(t_k["flatten_dilate"], t_k["flatten_erode"])]
    res = dict(pages=n, shape=list(pages[0].shape), radius=sorted(set(radii)), mb=round(page_bytes / 1e6, 1),
               flatten_call=stats(t_call),
               kernels=dict(flatten_dilate=kernel_row(t_k["flatten_dilate"], page_bytes + d_bytes, copy_gbs),
                            flatten_erode=kernel_row(t_k["flatten_erode"], d_bytes + 2 * page_bytes, copy_gbs),
                            both=kernel_row(both, 2 * d_bytes + 3 * page_bytes, copy_gbs)))

    def route(flatten):
        pages_dev = O.DevicePages(eng, pages)
        stages = ([lambda p: p.flattened()] if flatten else []) + [lambda p: p.deskewed(64), lambda p: p.resized(args.width)]
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
            O.flatten_page_host(p)
        t_host.append((time.perf_counter() - t0) * n / m)            # scaled to all pages
    host = stats(t_host)
    host.update(measured_on_pages=m, scaled_to_pages=n)
    res.update(route_with=stats(t_with), route_without=stats(t_without),
               stage_adds_ms=round(1e3 * (float(np.median(t_with)) - float(np.median(t_without))), 3),
               with_over_without=round(float(np.median(t_with)) / float(np.median(t_without)), 4), host=host,
               host_over_flatten_call=round(float(np.median(t_host)) / float(np.median(t_call)), 1))
    return res


def systems(O):
    """the system boxes the real weights find on the clean, the shaded and the flattened tutorial page, on the device"""
    import omr_ref
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    from test_page_flatten_host import shaded
    rec = build_recognizer(omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz")),
                           omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_bar_params.npz")))
    eng = rec.system_detector.engine
    clean = tutorial_page()
    dark = shaded(clean)

    def boxes(dev_pages):
        found = rec.detect_systems_pages([dev_pages.download_page(0)], in_mode=O.IN_U8_RAW, dev_pages=dev_pages)[0]
        if isinstance(found, Exception):
            return dict(error=repr(found))
        found = [np.asarray(s).astype(int) for s in found]
        return dict(systems=len(found), rows=[[int(s[:, 0].min()), int(s[:, 0].max())] for s in found],
                    columns=[[int(s[:, 1].min()), int(s[:, 1].max())] for s in found])

    out = {}
    for name, page in (("clean", clean), ("shaded", dark)):
        dev = O.DevicePages(eng, [page])
        out[name] = boxes(dev)
        if name == "shaded":
            flat = dev.flattened()
            out["flattened"] = boxes(flat)
            out["flattened"]["radius"] = flat.radii.tolist()
            out["flattened"]["largest_difference_from_clean_page"] = int(
                np.abs(flat.download_page(0).astype(np.int64) - clean).max())
            flat.free()
        dev.free()
    out["darkest_paper_pixel_of_shaded"] = int(dark[clean == 255].min())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--shape", default="3508x2480", help="rows x columns of every page")
    ap.add_argument("--width", type=int, default=835)
    ap.add_argument("--host_pages", type=int, default=4, help="pages the host flattening is measured on (scaled to --pages)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    from bench_live_track import copy_rate
    h, w = (int(v) for v in args.shape.split("x"))
    pages = shaded_pages(args.pages, h, w)
    eng = _lib.Engine(MODEL, device=0)
    copy_gbs = copy_rate(eng)
    result = dict(tool="bench_flatten", reps=args.reps, tile=O.FLATTEN_TILE, floor=O.FLATTEN_FLOOR,
                  copy_rate_gb_per_s=round(copy_gbs, 1), equal_with_the_host=True,
                  scan=measure(eng, O, pages, args, copy_gbs))
    eng.close()
    result["systems"] = systems(O)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
