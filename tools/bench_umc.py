#!/usr/bin/env python
"""Stage timing of the UMC piece-identification path (umc_a2s_server / umc_s2a_server), batched against per-item:

    python tools/bench_umc.py [--pieces 8] [--pages 2] [--seconds 20] [--reps 5] [--out profiles/r12_umc_8x2.json]
                              [--device_post]

A synthetic UMC directory is written to a temporary folder: --pieces pieces of --pages pages each (PNG; the tutorial
page of tests/golden and its left-right mirror in turn - the seeded pages of tools/bench_omr.py time the networks
well but yield no staff system with the reference's weights, and a strip without columns has no window to cut) and one
--seconds long recording per piece (sums of sines, 16-bit .wav), the OMR
networks with the reference's weights (tests/golden), the embedding network with synthetic weights.  Both directions
run on it, stage by stage, and the wall time of every stage is taken with time.perf_counter() around calls that
return after the device is done (every library call here synchronises before it returns):

    stage          batched path                                      per-item path (code of the parent commit)
    png_read       imread_gray of every page                         the same
    networks       pages uploaded once, both U-Nets read them        predict_pages per network, each uploading the pages
    host_post      systems_from_maps per page                        the same
    device_post    (--device_post, a third path "batched_device_post": the batched path with the maps left on the
                   device - the networks stage ends without their download - and asr_systems_from_maps_dev in place of
                   host_post; pages it does not decide go through systems_from_maps inside this stage)
    unroll         unroll_rows + asr_unroll_systems_dev, one launch  unwrap_systems per page + hstack per piece
    audio_read     load_audio of every recording                     the same
    spectrograms   process_many_dev: one launch                      process() per recording
    data_base      from_images + from_specs on the device handles    per piece: host slices, embed_view1 / embed_view2
    queries        detect_scores + detect_performances, handles      detect_score + detect_performance per piece

One warm-up pass, then --reps passes; per stage the median, minimum and maximum over the passes.  The device time of
the two new kernels comes from the library's event profiler in one extra pass, with the fraction of the HBM peak the
unroll copy reaches.  The ranks of both paths are compared (they must be equal).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
HBM_PEAK_GBS = 8000.0              # MI355X HBM3E
STAGES = ["png_read", "networks", "host_post", "unroll", "audio_read", "spectrograms", "data_base", "queries"]
STAGES_DEVICE_POST = [s if s != "host_post" else "device_post" for s in STAGES]     # the third path's rows
N_CANDIDATES = 25


def write_directory(root, n_pieces, n_pages, seconds):
    from PIL import Image
    from scipy.io import wavfile
    rng = np.random.default_rng(12)
    page = np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]
    variants = [page, np.ascontiguousarray(page[:, ::-1])]
    for i in range(n_pieces):
        d = os.path.join(root, "piece_%03d" % i)
        os.makedirs(os.path.join(d, "sheet"))
        for k in range(n_pages):
            Image.fromarray(variants[(i + k) % 2]).save(os.path.join(d, "sheet", "%02d.png" % (k + 1)))
        t = np.arange(int(seconds * 22050)) / 22050.0
        x = sum(a * np.sin(2 * np.pi * f * t) for a, f in zip(rng.uniform(0.1, 0.3, 5), rng.uniform(60, 4000, 5)))
        wavfile.write(os.path.join(d, "score_ppq.wav"), 22050, (x / np.abs(x).max() * 0.8 * 32767).astype(np.int16))
        wavfile.write(os.path.join(d, "01_performance.wav"), 22050, np.zeros(2205, np.int16))


class Clock(object):
    def __init__(self, stages):
        self.t = OrderedDict((s, 0.0) for s in stages)

    def stage(self, name):
        clock = self

        class _Ctx(object):
            def __enter__(self):
                self.t0 = time.perf_counter()

            def __exit__(self, *exc):
                clock.t[name] += time.perf_counter() - self.t0
        return _Ctx()


def host_post(O, rec, pages, sys_maps, bar_maps):
    out = []
    for page, sp, bp in zip(pages, sys_maps, bar_maps):
        try:
            out.append(O.systems_from_maps(O.prepare_image(page), sp, bp))
        except Exception:
            out.append(np.zeros((0, 4, 2)))           # a page without systems adds no column (the bench keeps the piece)
    return out


def rank_all(results, names):
    from audio_sheet_retrieval_amd.piece_identification import full_eval_rank
    return [full_eval_rank(res, votes, name)[0] for (res, votes), name in zip(results, names)]


def device_post(O, rec, pages, sys_out, bar_out, table):
    """asr_systems_from_maps_dev on the maps where the networks left them; undecided pages through the host path"""
    eng = rec.system_detector.engine
    ptr, mode, sizes, offs, hs, ws = table
    decided, _ = O.systems_from_maps_dev(eng, ptr, mode, offs, hs, ws, sys_out.ptr, bar_out.ptr, None,
                                         rec.system_detector.handle, rec.bar_detector.handle)
    out, fallbacks = [], 0
    for i, (st, corners) in enumerate(decided):
        if st == 3:
            fallbacks += 1
            shape = (int(hs[i]), int(ws[i]))
            sp = O._download_at(eng, sys_out, int(offs[i]) * 8, int(sizes[i])).reshape(shape)
            bp = O._download_at(eng, bar_out, int(offs[i]) * 8, int(sizes[i])).reshape(shape)
            out += host_post(O, rec, [pages[i]], [sp], [bp])
        else:
            out.append(corners if st == 0 else np.zeros((0, 4, 2)))
    return out, fallbacks


def run_pass(batched, data_dir, rec, engine, proc_of, dev_post=False):
    import glob
    from audio_sheet_retrieval_amd.audio_frontend import load_audio
    from audio_sheet_retrieval_amd.piece_identification import (DeviceArrays, EmbeddingDB, detect_performance,
                                                                detect_performances, detect_score, detect_scores)
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    c = Clock(STAGES_DEVICE_POST if dev_post else STAGES)
    fallbacks = 0
    piece_dirs = sorted(glob.glob(os.path.join(data_dir, "*")))
    names = [os.path.basename(d) for d in piece_dirs]
    n = len(names)
    with c.stage("png_read"):
        pages_of = [[O.imread_gray(p) for p in sorted(glob.glob(os.path.join(d, "sheet", "*.png")))] for d in piece_dirs]
    pages = [p for ps in pages_of for p in ps]
    piece_of_page = [i for i, ps in enumerate(pages_of) for _ in ps]
    with c.stage("audio_read"):
        audio = [load_audio(os.path.join(d, "score_ppq.wav")) for d in piece_dirs]
    targets = np.arange(n, dtype=np.int32)

    if batched:
        with c.stage("networks"):
            dev_pages = O.DevicePages(rec.system_detector.engine, pages)
            if dev_post:
                sys_out, _, table = rec.system_detector.predict_pages_dev(dev_pages)
                bar_out, _, _ = rec.bar_detector.predict_pages_dev(dev_pages)
                rec.system_detector.engine.sync()
            else:
                sys_maps = rec.system_detector.predict_pages(dev_pages)
                bar_maps = rec.bar_detector.predict_pages(dev_pages)
        if dev_post:
            with c.stage("device_post"):
                systems, fallbacks = device_post(O, rec, pages, sys_out, bar_out, table)
            sys_out.free()
            bar_out.free()
        else:
            with c.stage("host_post"):
                systems = host_post(O, rec, pages, sys_maps, bar_maps)
        with c.stage("unroll"):
            rows = [O.unroll_rows(p.shape, s) for p, s in zip(pages, systems)]
            strips = DeviceArrays(*O.unroll_systems_dev(dev_pages, rows, piece_of_page, n))
            dev_pages.free()
        with c.stage("spectrograms"):
            specs = proc_of(audio[0][1]).process_many_dev([a[0] for a in audio], [a[1] for a in audio])
        with c.stage("data_base"):
            sheet_db = EmbeddingDB.from_images(engine, names, strips)
            audio_db = EmbeddingDB.from_specs(engine, names, specs)
        with c.stage("queries"):
            _, r_a2s, _ = detect_scores(engine, sheet_db, specs, top_k=n, n_candidates=N_CANDIDATES, targets=targets)
            _, r_s2a, _ = detect_performances(engine, audio_db, strips, top_k=n, n_candidates=N_CANDIDATES,
                                              targets=targets)
        strips.buf.free()
        specs.buf.free()
        ranks = [int(r) for r in r_a2s] + [int(r) for r in r_s2a]
    else:
        with c.stage("networks"):
            sys_maps = rec.system_detector.predict_pages(pages, in_mode=O.IN_U8_RAW)
            bar_maps = rec.bar_detector.predict_pages(pages, in_mode=O.IN_U8_RAW)
        with c.stage("host_post"):
            systems = host_post(O, rec, pages, sys_maps, bar_maps)
        with c.stage("unroll"):
            sheets, k = [], 0
            for ps in pages_of:
                sheet = np.zeros((O.SYSTEM_HEIGHT, 0), np.uint8)
                for p in ps:
                    sheet = np.hstack((sheet, O.unwrap_systems(p, systems[k])))
                    k += 1
                sheets.append(sheet)
        with c.stage("spectrograms"):
            spec_list = [proc_of(scale).process(samples) for samples, scale in audio]
        with c.stage("data_base"):
            dbs = []
            for view, arrays, (h, w) in ((1, sheets, (160, 200)), (2, spec_list, (92, 42))):
                codes, ids = [], []
                for i, a in enumerate(arrays):
                    idx = np.arange(0, a.shape[1] - w, w // 4)
                    r0 = a.shape[0] // 2 - h // 2 if view == 1 else 0
                    if len(idx) == 0:
                        continue
                    x = np.stack([a[r0:r0 + h, s:s + w] for s in idx])[:, None]
                    codes.append(engine.embed_view1(x, prepared=False) if view == 1 else engine.embed_view2(x))
                    ids += [i] * len(idx)
                dbs.append(EmbeddingDB(engine, np.concatenate(codes), np.asarray(ids, np.int32), dict(enumerate(names))))
            sheet_db, audio_db = dbs
        with c.stage("queries"):
            res_a = [detect_score(engine, sheet_db, s, top_k=n, n_candidates=N_CANDIDATES) for s in spec_list]
            res_s = [detect_performance(engine, audio_db, s, top_k=n, n_candidates=N_CANDIDATES) for s in sheets]
        ranks = rank_all(res_a, names) + rank_all(res_s, names)
    n_windows = (len(sheet_db), len(audio_db))
    sheet_db.close()
    audio_db.close()
    return c.t, ranks, n_windows, sum(len(s) for s in systems), fallbacks


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pieces", type=int, default=8)
    p.add_argument("--pages", type=int, default=2)
    p.add_argument("--seconds", type=float, default=20.0)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    p.add_argument("--device_post", action="store_true",
                   help="also time the batched path with asr_systems_from_maps_dev in place of host_post")
    a = p.parse_args()

    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.audio_frontend import SpectrogramProcessor
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import omr_ref

    rec = build_recognizer(omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz")),
                           omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_bar_params.npz")))
    model = "mutopia_ccal_cont"
    engine = _lib.Engine(model, device=0)
    engine.set_params(synth_data.synth_params(param_shapes(model), seed=1, trained_like=True))
    procs = {}

    def proc_of(scale):
        if scale not in procs:
            procs[scale] = SpectrogramProcessor(engine, window_scale=scale)
        return procs[scale]

    out = OrderedDict(bench="umc", pieces=a.pieces, pages_per_piece=a.pages, seconds_per_recording=a.seconds,
                      reps=a.reps, n_candidates=N_CANDIDATES)
    with tempfile.TemporaryDirectory() as tmp:
        write_directory(tmp, a.pieces, a.pages, a.seconds)
        ranks = {}
        for path in ("batched", "per_item") + (("batched_device_post",) if a.device_post else ()):
            args = (path != "per_item", tmp, rec, engine, proc_of, path == "batched_device_post")
            run_pass(*args)                                                        # warm-up
            passes = []
            for _ in range(a.reps):
                t, ranks[path], n_windows, n_systems, fallbacks = run_pass(*args)
                passes.append(t)
            table = OrderedDict()
            for s in passes[0]:
                v = [ps[s] * 1e3 for ps in passes]
                table[s] = OrderedDict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3),
                                       max_ms=round(max(v), 3))
            tot = [sum(ps.values()) * 1e3 for ps in passes]
            table["total"] = OrderedDict(median_ms=round(float(np.median(tot)), 3), min_ms=round(min(tot), 3),
                                         max_ms=round(max(tot), 3))
            out[path] = table
        out["db_windows_sheet_audio"] = list(n_windows)
        out["systems"] = n_systems
        out["ranks_equal"] = all(r == ranks["batched"] for r in ranks.values())
        if a.device_post:
            out["device_post_fallback_pages"] = fallbacks

        # device time of the two new kernels: one more batched pass under the event profiler
        oe = rec.system_detector.engine
        for e in (oe, engine):
            e.profile_enable(True)
            e.profile_reset()
        run_pass(True, tmp, rec, engine, proc_of, a.device_post)
        prof = {r["name"]: r for e in (oe, engine) for r in e.profile()}
        for e in (oe, engine):
            e.profile_enable(False)
    post = ("post_rows", "post_threshold", "post_close", "post_label_pass", "post_blobs") if a.device_post else ()
    for label in ("unroll_systems", "spectrogram_batch") + post:
        r = prof.get(label)
        if r:
            out[label] = OrderedDict(device_ms=round(r["total_ms"], 4), bytes=r.get("bytes"), flops=r.get("flops"))
            if label in post:
                out[label]["launches"] = r.get("launches")
    r = prof.get("unroll_systems")
    if r and r["total_ms"] > 0:
        gbs = r["bytes"] / (r["total_ms"] * 1e-3) / 1e9
        out["unroll_systems"]["gb_per_s"] = round(gbs, 1)
        out["unroll_systems"]["hbm_fraction"] = round(gbs / HBM_PEAK_GBS, 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
