#!/usr/bin/env python
"""Tilted page scans at 300 dpi straightened on the device (asr_skew_estimate_dev, asr_deskew_pages_dev) against the
route a caller had before: omr.deskew_page_host on the host first.

    python tools/bench_deskew.py [--reps 5] [--pages 64] [--shape 3508x2480] [--max_slope 64] [--host_pages 4]
                                 [--umc_profile profiles/<bench_umc --device_post>.json] [--strips]
                                 [--out profiles/r23_deskew.json]

Two sets of N pages (uint8): `dense` - seeded noise over a staff-like pattern (tools/bench_page_resize.py's pages: no
pixel is blank, every run of every row adds to a profile), sheared by four slopes on the host - and `scan` - the tutorial
page of tests/golden replicated to three times its size (3543 x 2505: mostly paper, as a scan is), sheared likewise.
    estimate_call   one asr_skew_estimate_dev call on pages that are on the device (tables uploaded, profiles cleared,
                    kernels, slopes downloaded) - host clock
    shear_call      one asr_deskew_pages_dev call with those slopes - host clock
    kernels         skew_profiles, skew_scores and deskew_pages alone, from the library's event profiler (passes of their
                    own), each with its algorithmic bytes (skew_profiles: every page byte read once; skew_scores: every
                    profile word read once; deskew_pages: every byte read once and written once): GB/s and the share of
                    the device's measured copy rate.  The profile kernel's atomic adds are not bytes of this count.
    device_route    DevicePages(raw pages).deskewed(max_slope).resized(835): one upload, asr_sync
    host_route      deskew_page_host per page on the host, then DevicePages(pages).resized(835), asr_sync.  The host
                    deskew runs on --host_pages pages and is scaled to N (it is linear in the pages; 64 pages take over
                    a minute per pass); the scaled figure is marked as such
Before anything is timed the slopes and the sheared bytes of the first and the last page are compared with the host.
With --umc_profile: the estimate and the shear on as many tutorial pages as that tools/bench_umc.py --device_post run
had, and their share of its batched_device_post total plus themselves.  With --strips (reported, not gated; the
embedding network has synthetic weights): the tutorial page at slopes 12 and 30 - the strips of the straight, the
tilted and the deskewed page are cut into windows, embedded, and the cosine distances of the tilted and the deskewed
windows to the straight ones are reported.  Medians of --reps with ranges.  Prints one JSON line.  Needs a GPU.
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
COPY_GBS = 6290.0                # measured float4 copy rate of the MI355X, read + write (8000 GB/s on the data sheet)
MODEL = "mutopia_ccal_cont"
SLOPES = (30, -17, 8, -50)


def stats(times):
    return dict(median_ms=round(1e3 * float(np.median(times)), 3), min_ms=round(1e3 * min(times), 3),
                max_ms=round(1e3 * max(times), 3))


def tutorial_page():
    return np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]


def page_sets(n, h, w, O):
    rng = np.random.default_rng(23)
    rows = np.where((np.arange(h) // 7) % 9 < 5, 40, 250).astype(np.int16)[:, None]     # staff-like dark lines
    dense = [O.shear_page_host(np.clip(rows + rng.integers(-40, 40, (h, w), dtype=np.int16), 0, 255).astype(np.uint8), k)
             for k in SLOPES]
    big = np.repeat(np.repeat(tutorial_page(), 3, axis=0), 3, axis=1)
    scan = [O.shear_page_host(big, k) for k in SLOPES]
    return {"dense": [dense[i % 4] for i in range(n)], "scan": [scan[i % 4] for i in range(n)]}


def kernel_row(times, nbytes):
    k = float(np.median(times))
    row = stats(times)
    row.update(bytes=nbytes, gb_per_s=round(nbytes / k / 1e9, 1), share_of_copy_rate=round(nbytes / k / 1e9 / COPY_GBS, 4),
               least_ms_by_bytes=round(1e3 * nbytes / (COPY_GBS * 1e9), 4))
    return row


def measure(eng, O, pages, args, with_routes):
    K, n = args.max_slope, len(pages)
    raw = O.DevicePages(eng, pages)

    def estimate_call():
        return eng.skew_estimate_dev(raw.buf.ptr, raw.nbytes, raw.offsets, raw.heights, raw.widths, K)

    def shear_call(slopes):
        out = raw.deskewed(slopes=slopes)
        eng.sync()
        return out

    slopes = estimate_call()
    straight = shear_call(slopes)
    for i in sorted({0, n - 1}):                                     # the same integers and bytes at the timed size
        k = O.estimate_skew_host(pages[i], K)
        if k != slopes[i] or not np.array_equal(straight.download_page(i), O.shear_page_host(pages[i], k)):
            raise SystemExit("device and host differ on page %d" % i)
    straight.free()
    t_est, t_shear, t_k = [], [], {"skew_profiles": [], "skew_scores": [], "deskew_pages": []}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        estimate_call()
        t_est.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        out = shear_call(slopes)
        t_shear.append(time.perf_counter() - t0)
        out.free()
    eng.profile_enable(True)
    for _ in range(args.reps):
        eng.profile_reset()
        estimate_call()
        shear_call(slopes).free()
        rec = {p["name"]: p for p in eng.profile()}
        for name in t_k:
            t_k[name].append(1e-3 * rec[name]["total_ms"])
    eng.profile_enable(False)
    eng.profile_reset()
    page_bytes = float(raw.nbytes)
    prof_bytes = float(sum((2 * K + 1) * (int(h) + 2 * ((K * (int(w) - 1) + 1024) >> 11)) * 4
                           for h, w in zip(raw.heights, raw.widths)))
    res = dict(pages=n, shape=list(pages[0].shape), slopes_found=sorted(set(int(s) for s in slopes)),
               mb=round(page_bytes / 1e6, 1), estimate_call=stats(t_est), shear_call=stats(t_shear),
               kernels=dict(skew_profiles=kernel_row(t_k["skew_profiles"], page_bytes),
                            skew_scores=kernel_row(t_k["skew_scores"], prof_bytes),
                            deskew_pages=kernel_row(t_k["deskew_pages"], 2 * page_bytes)))
    raw.free()
    if not with_routes:
        return res

    def device_route():
        up = O.DevicePages(eng, pages)
        straight = up.deskewed(K)
        up.free()
        small = straight.resized(args.width)
        straight.free()
        eng.sync()
        return small

    def host_route():
        m = min(args.host_pages, n)
        t0 = time.perf_counter()
        host = [O.deskew_page_host(p, K)[0] for p in pages[:m]]
        t_host = (time.perf_counter() - t0) * n / m                 # scaled to all pages
        t0 = time.perf_counter()
        up = O.DevicePages(eng, [host[i % m] for i in range(n)])
        small = up.resized(args.width)
        up.free()
        eng.sync()
        return small, t_host, time.perf_counter() - t0

    device_route().free()
    host_route()[0].free()
    t_dev, t_host, t_host_deskew = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        small = device_route()
        t_dev.append(time.perf_counter() - t0)
        small.free()
        small, t_h, t_rest = host_route()
        small.free()
        t_host.append(t_h + t_rest)
        t_host_deskew.append(t_h)
    host = stats(t_host)
    host.update(host_deskew=stats(t_host_deskew), host_deskew_measured_on_pages=min(args.host_pages, n),
                scaled_to_pages=n)
    res.update(device_route=stats(t_dev), host_route=host,
               host_over_device=round(float(np.median(t_host)) / float(np.median(t_dev)), 2))
    return res


def umc_share(eng, O, args):
    with open(args.umc_profile) as fp:
        umc = json.loads(fp.readline())
    n = int(umc["pieces"]) * int(umc["pages_per_piece"])
    page = O.shear_page_host(tutorial_page(), 30)
    raw = O.DevicePages(eng, [page] * n)
    t_est, t_shear = [], []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        slopes = eng.skew_estimate_dev(raw.buf.ptr, raw.nbytes, raw.offsets, raw.heights, raw.widths, args.max_slope)
        t1 = time.perf_counter()
        out = raw.deskewed(slopes=slopes)
        eng.sync()
        t2 = time.perf_counter()
        out.free()
        if rep:                                                     # the first pass warms
            t_est.append(t1 - t0)
            t_shear.append(t2 - t1)
    raw.free()
    total = float(umc["batched_device_post"]["total"]["median_ms"])
    e, s = 1e3 * float(np.median(t_est)), 1e3 * float(np.median(t_shear))
    return dict(pages=n, page_shape=list(page.shape), umc_batched_device_post_total_ms=total, estimate_call=stats(t_est),
                shear_call=stats(t_shear), estimate_share_of_route=round(e / (total + e + s), 4),
                estimate_and_shear_share_of_route=round((e + s) / (total + e + s), 4))


def strip_distances(eng, O):
    """the windows of the straight, the tilted and the deskewed tutorial page's strips, embedded (synthetic weights)"""
    import omr_ref
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    rec = build_recognizer(omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz")),
                           omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_bar_params.npz")))
    eng.set_params(synth_data.synth_params(param_shapes(MODEL), seed=1, trained_like=True))
    page = tutorial_page()

    def codes(p):
        systems = rec.detect_systems_pages([p], in_mode=O.IN_U8_RAW)[0]
        strip = O.unwrap_systems(p, systems, 160)
        starts = np.arange(0, strip.shape[1] - 200, 50)
        windows = np.stack([strip[:, s:s + 200] for s in starts])[:, None]
        z = eng.embed_view1(np.ascontiguousarray(windows), prepared=False)
        return z / np.maximum(np.linalg.norm(z, axis=1, keepdims=True), 1e-12), strip.shape[1]

    straight, w0 = codes(page)
    out = dict(weights="synthetic (synth_params, trained_like)", windows="columns 0, 50, ... of each strip, 160 x 200",
               straight_strip_width=w0)
    for k in (12, 30):
        tilted_page = O.shear_page_host(page, k)
        fixed_page, found = O.deskew_page_host(tilted_page)
        row = dict(slope_found=int(found))
        for name, p in (("tilted", tilted_page), ("deskewed", fixed_page)):
            z, w = codes(p)
            m = min(len(z), len(straight))
            d = 1.0 - np.sum(z[:m] * straight[:m], axis=1)
            row[name] = dict(strip_width=w, windows=m, cosine_distance_mean=round(float(d.mean()), 4),
                             cosine_distance_median=round(float(np.median(d)), 4),
                             cosine_distance_max=round(float(d.max()), 4))
        out["slope_%d" % k] = row
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--shape", default="3508x2480", help="rows x columns of every dense page")
    ap.add_argument("--width", type=int, default=835)
    ap.add_argument("--max_slope", type=int, default=64)
    ap.add_argument("--host_pages", type=int, default=4, help="pages the host deskew is measured on (scaled to --pages)")
    ap.add_argument("--umc_profile", default=None, help="JSON of tools/bench_umc.py --device_post")
    ap.add_argument("--strips", action="store_true", help="also the cosine distances of the strips' windows")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    h, w = (int(v) for v in args.shape.split("x"))
    sets = page_sets(args.pages, h, w, O)
    eng = _lib.Engine(MODEL, device=0)
    result = dict(tool="bench_deskew", reps=args.reps, max_slope=args.max_slope, copy_rate_gb_per_s=COPY_GBS,
                  slopes_applied=list(SLOPES), equal_with_the_host=True,
                  dense=measure(eng, O, sets["dense"], args, True), scan=measure(eng, O, sets["scan"], args, False))
    if args.umc_profile:
        result["umc"] = umc_share(eng, O, args)
    if args.strips:
        result["strips"] = strip_distances(eng, O)
    eng.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
