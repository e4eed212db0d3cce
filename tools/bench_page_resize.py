#!/usr/bin/env python
"""Page scans at 300 dpi to the OMR networks' width: the device resize (asr_resize_pages_dev) against the route a caller
had before it - resizing on the host first and uploading 835-wide pages.

    python tools/bench_page_resize.py [--reps 5] [--pages 64] [--shape 3508x2480] [--out profiles/r17_page_resize.json]

N synthetic pages (seeded noise over a staff-like pattern, uint8):
    resize_call     one asr_resize_pages_dev call on pages that are on the device (page table uploaded, kernel,
                    synchronise) - host clock
    kernel          the kernel alone, from the library's event profiler (passes of their own), with its algorithmic bytes
                    (every source byte read once, every output byte written once): GB/s and the share of the device's
                    measured copy rate
    device_route    DevicePages(raw pages) + .resized(835): one upload of the raw pages, one launch, asr_sync
    host_route      omr.resize_pages_host on the host, then DevicePages(resized pages), asr_sync; the share of the host
                    resize is reported with it
    pil_route       the same with PIL's Image.resize(..., BOX) as the host resize.  For time only: PIL samples the box at
                    pixel centres and computes other values than the definition
Before anything is timed the device result is compared with omr.resize_page_host on the first and the last page, byte
for byte.  Every leg is warmed first, all legs run in this one process, alternating; medians of --reps with ranges.
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
COPY_GBS = 6290.0                # measured float4 copy rate of the MI355X, read + write (8000 GB/s on the data sheet)
MODEL = "mutopia_ccal_cont"


def synthetic_pages(n, h, w, seed):
    rng = np.random.default_rng(seed)
    rows = np.where((np.arange(h) // 7) % 9 < 5, 40, 250).astype(np.int16)[:, None]     # staff-like dark lines
    return [np.clip(rows + rng.integers(-40, 40, (h, w), dtype=np.int16), 0, 255).astype(np.uint8) for _ in range(n)]


def stats(times):
    return dict(median_ms=round(1e3 * float(np.median(times)), 3), min_ms=round(1e3 * min(times), 3),
                max_ms=round(1e3 * max(times), 3))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--shape", default="3508x2480", help="rows x columns of every page")
    ap.add_argument("--width", type=int, default=835)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    from PIL import Image
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    h, w = (int(v) for v in args.shape.split("x"))
    ho, wo = O.resized_shape(h, w, args.width)
    pages = synthetic_pages(args.pages, h, w, seed=17)
    eng = _lib.Engine(MODEL, device=0)
    raw = O.DevicePages(eng, pages)

    def resize_call():
        small = raw.resized(args.width)
        eng.sync()
        return small

    def device_route():
        up = O.DevicePages(eng, pages)
        small = up.resized(args.width)
        eng.sync()
        up.free()
        return small

    def host_route(resize):
        t0 = time.perf_counter()
        host = resize(pages)
        t1 = time.perf_counter()
        small = O.DevicePages(eng, host)
        eng.sync()
        return small, t1 - t0

    by_definition = lambda ps: O.resize_pages_host(ps, args.width)
    by_pil = lambda ps: [np.asarray(Image.fromarray(p).resize((wo, ho), Image.BOX)) for p in ps]

    # the same bytes at the timed size, and the warm-up of every leg
    small = resize_call()
    for i in sorted({0, args.pages - 1}):
        if not np.array_equal(small.download_page(i), O.resize_page_host(pages[i], ho, wo)):
            raise SystemExit("device and resize_page_host differ on page %d of %d x %d" % (i, h, w))
    small.free()
    device_route().free()
    host_route(by_definition)[0].free()
    pil_small = host_route(by_pil)[0]
    pil_differs = float(np.mean(pil_small.download_page(0) != O.resize_page_host(pages[0], ho, wo)))
    pil_small.free()

    t_call, t_dev, t_host, t_host_resize, t_pil, t_pil_resize, t_kernel = [], [], [], [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        small = resize_call()
        t_call.append(time.perf_counter() - t0)
        small.free()
        t0 = time.perf_counter()
        small = device_route()
        t_dev.append(time.perf_counter() - t0)
        small.free()
        t0 = time.perf_counter()
        small, t_res = host_route(by_definition)
        t_host.append(time.perf_counter() - t0)
        t_host_resize.append(t_res)
        small.free()
        t0 = time.perf_counter()
        small, t_res = host_route(by_pil)
        t_pil.append(time.perf_counter() - t0)
        t_pil_resize.append(t_res)
        small.free()
    eng.profile_enable(True)
    for _ in range(args.reps):
        eng.profile_reset()
        resize_call().free()
        rec = [p for p in eng.profile() if p["name"] == "resize_pages"]
        t_kernel.append(1e-3 * rec[0]["total_ms"] / rec[0]["launches"])
    eng.profile_enable(False)
    eng.profile_reset()
    raw.free()
    eng.close()

    k = float(np.median(t_kernel))
    nbytes = float(args.pages) * (h * w + ho * wo)
    kernel = stats(t_kernel)
    kernel.update(bytes=nbytes, gb_per_s=round(nbytes / k / 1e9, 1),
                  share_of_copy_rate=round(nbytes / k / 1e9 / COPY_GBS, 4),
                  least_ms_by_bytes=round(1e3 * nbytes / (COPY_GBS * 1e9), 4))
    call = stats(t_call)
    call["kernel_share_of_call"] = round(k / float(np.median(t_call)), 4)
    host = stats(t_host)
    host["host_resize"] = stats(t_host_resize)
    pil = stats(t_pil)
    pil["host_resize"] = stats(t_pil_resize)
    pil["share_of_pixels_that_differ_from_the_definition"] = round(pil_differs, 4)
    result = dict(tool="bench_page_resize", reps=args.reps, pages=args.pages, shape=[h, w], resized=[ho, wo],
                  tile=[16, 64], copy_rate_gb_per_s=COPY_GBS, byte_equal_with_resize_page_host=True,
                  raw_upload_mb=round(args.pages * h * w / 1e6, 1), resized_upload_mb=round(args.pages * ho * wo / 1e6, 1),
                  resize_call=call, kernel=kernel, device_route=stats(t_dev), host_route=host, pil_route=pil,
                  host_over_device=round(float(np.median(t_host)) / float(np.median(t_dev)), 2),
                  pil_over_device=round(float(np.median(t_pil)) / float(np.median(t_dev)), 2))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
