#!/usr/bin/env python
"""The score map on the device (asr_score_map_dev): what the call and its kernels take on the bar maps of N pages, what
the host takes for the same table, and what the stage adds to the loader route.

    python tools/bench_score_map.py [--reps 5] [--pages 64] [--pieces 16] [--out profiles/r30_score_map.json]

N copies of the tutorial page of tests/golden (1181 x 835), --pieces pieces of N / pieces pages, through the real OMR
weights on the device.
    score_map_call  one sheet_utils.omr.score_map_dev on bar maps that are on the device (the tables built and uploaded,
                    three launches, the rows downloaded) - host clock
    kernels         score_map_counts, score_map_lines and score_map_table alone, from the library's event profiler
                    (passes of their own), with their algorithmic bytes (counts: every float64 of every band once;
                    lines: a flag word per 64 columns; table: the rows written): GB/s and the share of the copy rate
                    measured in the same session (tools/bench_live_track.copy_rate)
    host            DeviceMaps.download() of all bar maps, then score_map_host, in the same process; the two parts apart
    route_with      load_umc_scans(dir, return_device=True, device_post=True, page_width=None, deskew=False,
                    score_map=True) on the pages as PNG files - load_umc_sheets' route, with the map
    route_without   the same call with score_map=False: the route as it was, in the same process, alternating
Before anything is timed the device table is compared with the host's.  Medians of --reps with ranges.  Prints one JSON
line.  Needs a GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def stats(times):
    return dict(median_ms=round(1e3 * float(np.median(times)), 3), min_ms=round(1e3 * min(times), 3),
                max_ms=round(1e3 * max(times), 3))


def kernel_row(times, nbytes, copy_gbs):
    k = float(np.median(times))
    row = stats(times)
    row.update(bytes=nbytes, gb_per_s=round(nbytes / k / 1e9, 2), share_of_copy_rate=round(nbytes / k / 1e9 / copy_gbs, 5),
               least_ms_by_bytes=round(1e3 * nbytes / (copy_gbs * 1e9), 5))
    return row


def recognizer():
    import omr_ref
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    return build_recognizer(omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz")),
                            omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_bar_params.npz")))


def measure_call(O, rec, pages, n_pieces, reps, copy_gbs):
    eng = rec.system_detector.engine
    n = len(pages)
    per = n // n_pieces
    piece_of_page = [min(p // per, n_pieces - 1) for p in range(n)]
    dev_pages = O.DevicePages(eng, pages)
    try:
        found, bar_maps = rec.detect_systems_keep_bars_dev(pages, in_mode=O.IN_U8_RAW, dev_pages=dev_pages)
    finally:
        dev_pages.free()
    try:
        page_rows = [O.unroll_rows(p.shape, s, with_index=True) for p, s in zip(pages, found)]
        want = O.score_map_host(bar_maps.download(), page_rows, piece_of_page, n_pieces)
        got = O.score_map_dev(bar_maps, page_rows, piece_of_page, n_pieces)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            raise SystemExit("device and host differ")
        t_call, t_down, t_host = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            O.score_map_dev(bar_maps, page_rows, piece_of_page, n_pieces)
            t_call.append(time.perf_counter() - t0)
        names = ("score_map_counts", "score_map_lines", "score_map_table")
        t_k = {name: [] for name in names}
        eng.profile_enable(True)
        for _ in range(reps):
            eng.profile_reset()
            O.score_map_dev(bar_maps, page_rows, piece_of_page, n_pieces)
            prof = {p["name"]: p for p in eng.profile()}
            for name in names:
                t_k[name].append(1e-3 * prof[name]["total_ms"])
        eng.profile_enable(False)
        eng.profile_reset()
        for _ in range(reps):
            t0 = time.perf_counter()
            maps = bar_maps.download()
            t1 = time.perf_counter()
            O.score_map_host(maps, page_rows, piece_of_page, n_pieces)
            t_down.append(t1 - t0)
            t_host.append(time.perf_counter() - t1)
    finally:
        bar_maps.free()
    systems = [r for rows in page_rows for r in rows]
    band = float(sum((r1 - r0) * (c1 - c0) for r0, r1, c0, c1, _, _ in systems)) * 8
    words = float(sum(-(-(c1 - c0) // 64) for _, _, c0, c1, _, _ in systems)) * 8
    rows_b = float(len(got[0])) * 32
    all_k = [a + b + c for a, b, c in zip(*(t_k[name] for name in names))]
    both = [a + b for a, b in zip(t_down, t_host)]
    return dict(pages=n, pieces=n_pieces, shape=list(pages[0].shape), systems=len(systems), measures=int(len(got[0])),
                measures_per_system_of_the_first_page=np.bincount(
                    [m[3] for m in got[0][:got[1][1]].tolist() if m[2] == 0], minlength=len(page_rows[0])).tolist(),
                map_mb=round(float(sum(p.size for p in pages)) * 8 / 1e6, 1), band_mb=round(band / 1e6, 1),
                score_map_call=stats(t_call),
                kernels=dict(score_map_counts=kernel_row(t_k[names[0]], band, copy_gbs),
                             score_map_lines=kernel_row(t_k[names[1]], words, copy_gbs),
                             score_map_table=kernel_row(t_k[names[2]], rows_b, copy_gbs),
                             all=kernel_row(all_k, band + words + rows_b, copy_gbs)),
                host=dict(download=stats(t_down), score_map_host=stats(t_host), both=stats(both)),
                host_over_score_map_call=round(float(np.median(both)) / float(np.median(t_call)), 1))


def measure_route(rec, pages, n_pieces, reps):
    from PIL import Image
    from audio_sheet_retrieval_amd.sheet_utils import umc
    per = len(pages) // n_pieces
    with tempfile.TemporaryDirectory() as tmp:
        for p, page in enumerate(pages):
            d = os.path.join(tmp, "piece%03d" % min(p // per, n_pieces - 1), "sheet")
            os.makedirs(d, exist_ok=True)
            Image.fromarray(page).save(os.path.join(d, "%03d.png" % p))

        def route(score_map):
            with contextlib.redirect_stdout(io.StringIO()):
                out = umc.load_umc_scans(tmp, omr=rec, return_device=True, device_post=True, page_width=None, deskew=False,
                                         score_map=score_map)
            out[3].buf.free()
            return out

        route(True)
        route(False)
        t_with, t_without = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            route(True)
            t_with.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            route(False)
            t_without.append(time.perf_counter() - t0)
    return dict(route_with=stats(t_with), route_without=stats(t_without),
                stage_adds_ms=round(1e3 * (float(np.median(t_with)) - float(np.median(t_without))), 3),
                with_over_without=round(float(np.median(t_with)) / float(np.median(t_without)), 4))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--pieces", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    from bench_live_track import copy_rate
    page = np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]
    pages = [page] * args.pages
    rec = recognizer()
    copy_gbs = copy_rate(rec.system_detector.engine)
    result = dict(tool="bench_score_map", reps=args.reps, threshold=O.SCORE_MAP_THRESHOLD, min_rows=O.SCORE_MAP_MIN_ROWS,
                  tol=O.BAR_MISSING_TOL, max_lines=O.SCORE_MAP_MAX_LINES, copy_rate_gb_per_s=round(copy_gbs, 1),
                  equal_with_the_host=True)
    result.update(measure_call(O, rec, pages, args.pieces, args.reps, copy_gbs))
    result.update(measure_route(rec, pages, args.pieces, args.reps))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
