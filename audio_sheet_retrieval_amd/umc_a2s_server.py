#!/usr/bin/env python
"""Piece identification on scanned commercial scores ("UMC"), audio -> sheet ("A2S").  Command line of the reference's
umc_a2s_server.py (:178-189):

    python -m audio_sheet_retrieval_amd.umc_a2s_server --model models/mutopia_ccal_cont.py --data_dir <dir> \
        --train_split splits/all_split.yaml --config exp_configs/mutopia_full_aug.yaml \
        --init_sheet_db --full_eval --dump_results [--real_perf] [--n_candidates 25] [--estimate_UV] \
        --system_params system_params.pkl --bar_params bar_params.pkl [--device_post] [--resample] [--page_width 835]
        [--deskew] [--flatten] [--crop] [--live [--bank] [--live_dft direct|fft] [--block_ms 100] [--running_frames 100]
                   [--level running [--level_memory N] [--level_floor F]]]
        [--locate [--excerpt_frames 400] [--locate_pieces 5] [--step_spec 2] [--seed 23]]

<dir> holds one folder per piece: sheet/*.png (the page scans), score_ppq.* (the synthesised recording) and, for
--real_perf, 01_performance*.  The pages go through the two segmentation networks (their parameter pickles:
--system_params / --bar_params; the reference hard-codes sheet_utils/omr_models/), the detected staff systems are
unrolled into one strip per piece (sheet_utils/umc.load_umc_sheets, require_performance=True).  --device_post (off by
default) also finds the systems from the two maps on the device (asr_systems_from_maps_dev: the maps are not
downloaded; a page the device does not decide goes through the host path, the result is the same).  --init_sheet_db embeds
the strip windows (EmbeddingDB.from_images: initialize_sheet_db_from_imges) into umc_sheet_db_file.pkl in the working
directory; without it that file is loaded.  --full_eval queries the data base with every piece's recording: 100
windows per piece, n_candidates neighbours per window, top_k = number of pieces, the reference's rank rule; a piece
whose recording is missing is left out of the ranks (:234-235).  --dump_results writes
umc_retrieval_<tag>_<dset>_A2S[_real].yaml next to the parameters.

All pages go through each network in one call, all systems are unrolled in one call, all recordings become
spectrograms in one call, and strips and spectrograms stay on the device for the data base and the queries
(piece_identification.detect_scores / detect_performances).  umc_s2a_server.py is the S2A direction of this driver.
Recordings are read by audio_frontend.load_audio: .wav or .npy at 22050 Hz.  --resample (off by default) reads .wav
files of any sample rate (audio_frontend.read_audio) and resamples them to 22050 Hz on the device, between the upload
and the spectrogram launch (asr_resample_batch_dev).  The pages are taken at the resolution the networks were trained on,
835 pixels wide; --page_width W (none by default; 835 for these networks) accepts scans of any resolution and reduces
them to W columns on the device, between the upload and the first network (asr_resize_pages_dev: exact area
resampling, the shape rule of the reference's scripts/prepare_umc_data.py).  --deskew (off by default; with or without
--page_width) takes flat-bed scans whose staves are not horizontal: the slope of every page is estimated and the page
sheared by it on the device, between the upload and the resize (sheet_utils/umc.load_umc_scans).  --flatten (off by
default; with or without --deskew and --page_width) takes scans whose paper is not white - a spine shadow, a gradient,
yellowed paper: every page is divided by the grey closing of its paper on the device, right after the upload
(asr_flatten_pages_dev).  --crop (off by default; with or without the other three) takes scans of pages smaller than the
scanner's glass: the black frame around the paper is found and cut off on the device, before everything else, so that
--page_width scales the paper and not the frame (asr_crop_estimate_dev, asr_crop_pages_dev).

--live (A2S only, off by default) runs the reference's default mode, the running vote of AudioSheetServer.run, on the
recordings as a sound card would deliver them: every queried piece's recording is read at its own rate
(audio_frontend.read_audio), cut into blocks of --block_ms milliseconds and streamed through
piece_identification.live_track_scores (AudioStream: asr_audio_stream_push_dev, then PieceTracker).  Per piece it prints
the first frame at which the piece leads and the share of voiced frames at which it leads
(audio_sheet_server.report_tracking); --dump_results writes umc_tracking_<tag>_<dset>_A2S[_real].yaml.  The level of the
music gate is taken from the finished spectrogram, as --track of audio_sheet_server does; a microphone has to be given one.
--bank (with --live) tracks all recordings of one sample rate with one piece_identification.PieceTrackerBank, whose
state stays on the device (live_track_scores(batched=True)): the same printout and the same file.
--level running (with --live --bank; default recording) gates every frame at the level of what its stream has brought
so far (piece_identification.RunningLevel; --level_memory N: of its last N columns, --level_floor F: never below F): no
spectrogram is computed beforehand - what a microphone can do.  The report and the file name the rule.
--live_dft fft (with --live; default direct) computes the streamed frames with the real-input FFT
(asr_audio_stream_push_fft_dev): the processor is built with dft="fft" and its streams are asked for by that name, so the
tracking equals track_scores on that processor's spectrograms.  --fast_dft stays a flag of the offline routes.

--locate (A2S only, off by default) answers "where in which scan?" in bars and pages: a seeded excerpt of
--excerpt_frames frames of every recording is located in the data base of the scans (piece_identification.locate_scores,
--locate_pieces candidates, a query window every --step_spec frames, as audio_sheet_server --locate), and the score map
(score_map.ScoreMap: the measures of every piece in strip coordinates, built on the device from the bar network's maps
while the pages are unrolled - asr_score_map_dev) turns the strip coordinates into bars, pages and systems.  Per
recording it prints the least-cost candidate, the rank of the recording's own piece among the candidates and the bars
the excerpt covers; --dump_results writes umc_location_<tag>_<dset>_A2S[_real].yaml.  Bars are counted from 1 in the
report, pages and systems from 0.  With --init_sheet_db the map is written next to the data-base file
(umc_sheet_db_file_score_map.npz); a run without it loads the map from there.  Building the map detects the systems by
the device post-processing (--device_post's route: the same systems), which keeps the bar maps for it.
"""
import argparse
import os

import numpy as np

from . import audio2sheet_align
from .audio_frontend import SpectrogramProcessor
from .audio_sheet_server import (TRACK_TOP_K, check_level_arguments, common_arguments, level_arguments, level_rule,
                                 report_ranks, report_tracking)
from .piece_identification import EmbeddingDB, detect_performances, detect_scores, live_track_scores, locate_scores
from .score_map import ScoreMap
from .sheet_utils import umc

# per direction: data-base flag, data-base file, data-base view
DIRECTIONS = {
    "A2S": dict(init_flag="--init_sheet_db", db_file="umc_sheet_db_file.pkl", db_view=1),
    "S2A": dict(init_flag="--init_audio_db", db_file="umc_audio_db_file.pkl", db_view=2),
}


def _arguments(argv, direction):
    d = DIRECTIONS[direction]
    p = argparse.ArgumentParser(description="Identify every piece of a directory of scanned scores: %s." %
                                ("audio -> sheet music" if direction == "A2S" else "sheet music -> audio"))
    common_arguments(p, d["init_flag"], d["db_file"], "umc_retrieval_<tag>_<dset>_%s[_real].yaml" % direction)
    p.add_argument("--real_perf", action="store_true", help="use the real recordings (01_performance*)")
    p.add_argument("--data_dir", type=str, default=None, help="one folder per piece: sheet/*.png and the recordings")
    p.add_argument("--system_params", type=str, default="sheet_utils/omr_models/system_params.pkl",
                   help="parameters of the system detector")
    p.add_argument("--bar_params", type=str, default="sheet_utils/omr_models/bar_params.pkl",
                   help="parameters of the bar detector")
    p.add_argument("--device_post", action="store_true",
                   help="find the systems from the U-Net maps on the device too (asr_systems_from_maps_dev)")
    p.add_argument("--resample", action="store_true",
                   help="accept recordings at any sample rate and resample them on the device (asr_resample_batch_dev)")
    p.add_argument("--page_width", type=int, default=None,
                   help="accept page scans of any resolution and resize them to this width on the device "
                        "(asr_resize_pages_dev); the networks were trained at 835")
    p.add_argument("--deskew", action="store_true",
                   help="estimate the slope of every page's staves and straighten the page on the device, before the "
                        "resize (asr_skew_estimate_dev, asr_deskew_pages_dev; sheet_utils/umc.load_umc_scans)")
    p.add_argument("--flatten", action="store_true",
                   help="divide every page by the grey closing of its paper on the device, before the deskew and the "
                        "resize: shadows, gradients, yellowed paper (asr_flatten_pages_dev; "
                        "sheet_utils/umc.load_umc_scans)")
    p.add_argument("--crop", action="store_true",
                   help="cut every page to the paper inside the scanner's black frame on the device, before the flatten, "
                        "the deskew and the resize (asr_crop_estimate_dev, asr_crop_pages_dev; "
                        "sheet_utils/umc.load_umc_scans)")
    p.add_argument("--fast_dft", action="store_true",
                   help="compute the spectrograms' magnitudes with an FFT (asr_spectrogram_fft_batch_dev; "
                        "SpectrogramProcessor(dft=\"fft\")): the same spectrograms to float32 rounding, not bit for bit")
    if direction == "A2S":
        p.add_argument("--live", action="store_true",
                       help="stream every recording block by block through the running vote (live_track_scores)")
        p.add_argument("--bank", action="store_true",
                       help="--live with one PieceTrackerBank per sample rate in place of a PieceTracker per recording: "
                            "the trackers' state stays on the device (live_track_scores(batched=True))")
        p.add_argument("--live_dft", choices=("direct", "fft"), default="direct",
                       help="--live: the transform of the streamed front-end - the direct DFT, or the real-input FFT "
                            "(asr_audio_stream_push_fft_dev; SpectrogramProcessor(dft=\"fft\").stream(dft=\"fft\"))")
        p.add_argument("--block_ms", type=float, default=100.0, help="milliseconds of audio per block (--live)")
        p.add_argument("--running_frames", type=int, default=100,
                       help="voiced frames in the history of the running vote (--live)")
        level_arguments(p, "--live --bank")
        p.add_argument("--locate", action="store_true",
                       help="locate a seeded excerpt of every recording in the scans and report bars and pages "
                            "(locate_scores, score_map.ScoreMap)")
        p.add_argument("--excerpt_frames", type=int, default=400, help="frames of the excerpt (--locate)")
        p.add_argument("--locate_pieces", type=int, default=5, help="candidates of the vote that are aligned (--locate)")
        p.add_argument("--step_spec", type=int, default=2, help="frames between the query windows (--locate)")
        p.add_argument("--seed", type=int, default=23, help="seed of the excerpts (--locate)")
    args = p.parse_args(argv)
    if getattr(args, "locate", False) and getattr(args, "live", False):
        p.error("--locate and --live are two modes: choose one")
    if args.fast_dft and getattr(args, "live", False):
        p.error("--fast_dft with --live: the streamed front-end computes the direct DFT unless --live_dft fft asks for "
                "its FFT")
    if getattr(args, "live_dft", "direct") != "direct" and not args.live:
        p.error("--live_dft needs --live: it chooses the transform of the streamed front-end")
    if getattr(args, "bank", False) and not args.live:
        p.error("--bank needs --live: it chooses how the streamed recordings are tracked")
    if direction == "A2S":
        check_level_arguments(p, args, args.live and args.bank,
                              "--level running needs --live --bank: the running level's state lives on the device, in "
                              "the PieceTrackerBank")
    return args


def tracking_file(param_file, dset, real_perf=False):
    """result_file's name with umc_tracking_ in place of umc_retrieval_"""
    return result_file(param_file, dset, "A2S", real_perf).replace("umc_retrieval_", "umc_tracking_", 1)


def live_track(engine, db, processor, piece_paths, names, audio_file, n_candidates, running_frames, block_ms,
               batched=False, dft=None, level=None):
    """the recordings of `piece_paths`, streamed in blocks of block_ms milliseconds -> (names, first_lead, lead_share) as
    audio_sheet_server.track.  dft: live_track_scores' ("fft" with a dft="fft" processor); level: None - the finished
    spectrogram's maximum, computed beforehand - or a RunningLevel (batched only)"""
    from .audio_frontend import read_audio
    recs, scales, rates, integer = [], [], [], []
    for piece_path in piece_paths:
        samples, scale, rate, is_int = read_audio(umc.get_performance_audio_path(piece_path, audio_file))
        recs.append(samples)
        scales.append(scale)
        rates.append(rate)
        integer.append(is_int)
    steps = [max(1, int(round(rate * block_ms / 1000.0))) for rate in rates]
    results = live_track_scores(engine, db, processor, recs, rates, steps, level, top_k=TRACK_TOP_K,
                                n_candidates=n_candidates, running_frames=running_frames, integer=integer,
                                window_scales=scales, batched=batched, dft=dft)
    ids = {name: i for i, name in db.id_to_name.items()}
    first_lead, lead_share = [], []
    for name, res in zip(names, results):
        leads = (res.n_out > 0) & (res.pieces[:, 0] == ids.get(name, -2)) if len(res.frames) else np.zeros(0, bool)
        first_lead.append(int(res.frames[np.argmax(leads)]) if leads.any() else -1)
        lead_share.append(float(leads.mean()) if leads.size else 0.0)
    return names, first_lead, lead_share


def location_file(param_file, dset, real_perf=False):
    """result_file's name with umc_location_ in place of umc_retrieval_"""
    return result_file(param_file, dset, "A2S", real_perf).replace("umc_retrieval_", "umc_location_", 1)


def locate(engine, db, score_map, specs, names, n_candidates, excerpt_frames, n_pieces, step_spec, seed,
           spec_shape=(92, 42)):
    """a seeded excerpt of every spectrogram (host arrays, one per name) located in the data base of the scans -> one
    dict per recording: name; candidate, cost (the least-cost candidate); own_rank (the rank by cost of the recording's
    own piece among the candidates, 0: not among them); first_bar / last_bar (from 1) and start_page, start_system,
    end_page, end_system (from 0) of the candidate's path through its score"""
    rng = np.random.RandomState(seed)
    excerpts = []
    for spec in specs:
        n = min(int(excerpt_frames), spec.shape[1])
        f0 = int(rng.randint(0, spec.shape[1] - n + 1))
        excerpts.append(np.ascontiguousarray(spec[:, f0:f0 + n]))
    found = locate_scores(engine, db, excerpts, n_pieces=n_pieces, step_spec=step_spec, n_candidates=n_candidates,
                          spec_shape=spec_shape)
    out = []
    for name, cands in zip(names, found):
        entry = dict(name=str(name), candidate=None, cost=None, own_rank=0, first_bar=None, last_bar=None,
                     start_page=None, start_system=None, end_page=None, end_system=None)
        for rank, cand in enumerate(cands):
            if cand["name"] == name:
                entry["own_rank"] = rank + 1
                break
        if cands:
            best = cands[0]
            ann = score_map.annotate(best)
            start, end = ann["start_x"], ann["end_x"]
            entry.update(candidate=str(best["name"]), cost=float(best["cost"]),
                         first_bar=int(start["bar"]) + 1, last_bar=int(end["bar"]) + 1,
                         start_page=int(start["page"]), start_system=int(start["system"]),
                         end_page=int(end["page"]), end_system=int(end["system"]))
        out.append(entry)
    return out


def report_location(entries, res_file=None):
    import yaml
    for e in entries:
        if e["candidate"] is None:
            print("no candidate                                                          %s" % e["name"])
            continue
        own = "%02d" % e["own_rank"] if e["own_rank"] else "--"
        print("own piece at rank %s; bars %3d - %3d (page %d system %d - page %d system %d) of %s  <- %s"
              % (own, e["first_bar"], e["last_bar"], e["start_page"], e["start_system"], e["end_page"], e["end_system"],
                 e["candidate"], e["name"]))
    print("own piece first by cost: %d of %d" % (sum(e["own_rank"] == 1 for e in entries), len(entries)))
    if res_file is not None:
        with open(res_file, "w") as fp:
            yaml.dump(entries, fp, default_flow_style=False)
        print("location of %d recordings written to %s" % (len(entries), res_file))
    return entries


def _download_arrays(dev):
    """the arrays of a piece_identification.DeviceArrays on the host, in one copy"""
    total = sum(r * c for r, c in dev.shapes)
    flat = dev.buf.download((total,), np.float32) if total else np.zeros(0, np.float32)
    return [flat[o:o + r * c].reshape(r, c) for o, (r, c) in zip(dev.offsets, dev.shapes)]


def result_file(param_file, dset, direction, real_perf=False):
    """the reference's dump name (:270-274): a tag-less params.pkl gives params_<dset>_<direction>.yaml"""
    ret_dir = direction + ("_real" if real_perf else "")
    return param_file.replace("params_", "umc_retrieval_").replace(".pkl", "_%s_%s.yaml") % (dset, ret_dir)


def run(argv, direction):
    d = DIRECTIONS[direction]
    args = _arguments(argv, direction)
    if args.data_dir is None:
        raise SystemExit("--data_dir: the directory of pieces is required")
    omr = umc.build_recognizer(args.system_params, args.bar_params)
    locating = getattr(args, "locate", False)
    build_map = locating and args.init_db                   # otherwise --locate loads the map the data base was saved with
    if args.deskew or args.flatten or args.crop or build_map:  # (no flag: load_umc_scans is load_umc_sheets with the map)
        loaded = umc.load_umc_scans(args.data_dir, require_performance=True, omr=omr, return_device=True,
                                    device_post=args.device_post, page_width=args.page_width, deskew=args.deskew,
                                    flatten=args.flatten, score_map=build_map, crop=args.crop)
    else:
        loaded = umc.load_umc_sheets(args.data_dir, require_performance=True, omr=omr, return_device=True,
                                     device_post=args.device_post, page_width=args.page_width)
    te_pieces, piece_paths, _, strips = loaded[:4]
    score_map = loaded[4] if build_map else None
    try:
        dset = os.path.basename(args.data_dir)
        audio_file = "01_performance" if args.real_perf else "score_ppq"
        engine, param_file = audio2sheet_align.load_network(args.model, args.estimate_UV, args.train_split, args.config)
        live_fft = getattr(args, "live_dft", "direct") == "fft"
        processor = SpectrogramProcessor(engine, dft="fft" if args.fast_dft or live_fft else "direct")
        if direction == "A2S":
            # a piece without the recording is left out of the ranks
            queried = []
            for i, piece_path in enumerate(piece_paths):
                try:
                    umc.get_performance_audio_path(piece_path, audio_file)
                    queried.append(i)
                except IndexError:
                    pass
        else:
            print("Loading spectrograms ...")
            queried = list(range(len(te_pieces)))
        specs = umc.load_specs([piece_paths[i] for i in queried], audio_file, processor, return_device=True,
                               resample=args.resample or getattr(args, "live", False))
        try:
            if args.init_db:
                print("Initializing %s db ..." % ("sheet music" if direction == "A2S" else "audio"))
                if direction == "A2S":
                    db = EmbeddingDB.from_images(engine, te_pieces, strips)
                else:
                    db = EmbeddingDB.from_specs(engine, te_pieces, specs)
                print("%d %s of %d pieces collected" % (len(db), "sheet snippet codes" if direction == "A2S" else
                                                        "audio excerpts", len(te_pieces)))
                db.save(d["db_file"])
                if score_map is not None:
                    score_map.save(ScoreMap.path_for(d["db_file"]))
            else:
                db = EmbeddingDB.load(engine, d["db_file"])
                if locating:
                    score_map = ScoreMap.load(ScoreMap.path_for(d["db_file"]))
            if locating:
                print("\nLocating an excerpt of every recording:")
                names = [te_pieces[i] for i in queried]
                return report_location(locate(engine, db, score_map, _download_arrays(specs), names, args.n_candidates,
                                              args.excerpt_frames, args.locate_pieces, args.step_spec, args.seed),
                                       location_file(param_file, dset, args.real_perf) if args.dump_results else None)
            if getattr(args, "live", False):
                print("\nStreaming every recording through the running vote:")
                names = [te_pieces[i] for i in queried]
                return report_tracking(*live_track(engine, db, processor, [piece_paths[i] for i in queried], names,
                                                   audio_file, args.n_candidates, args.running_frames, args.block_ms,
                                                   batched=args.bank, dft="fft" if live_fft else None,
                                                   level=level_rule(args)),
                                       res_file=tracking_file(param_file, dset, args.real_perf) if args.dump_results
                                       else None, level=level_rule(args))
            if not args.full_eval:
                return []
            print("\nRunning full evaluation:")
            ids = {name: i for i, name in db.id_to_name.items()}
            names = [te_pieces[i] for i in queried]
            targets = np.array([ids.get(n, -1) for n in names], np.int32)
            if not names:
                ranks, ratios = np.zeros(0, np.int32), np.zeros(0, np.float64)
            elif direction == "A2S":
                _, ranks, ratios = detect_scores(engine, db, specs, top_k=len(te_pieces), n_candidates=args.n_candidates,
                                                 targets=targets)
            else:
                _, ranks, ratios = detect_performances(engine, db, strips, top_k=len(te_pieces),
                                                       n_candidates=args.n_candidates, targets=targets)
        finally:
            specs.buf.free()
    finally:
        strips.buf.free()
    return report_ranks(names, ranks, ratios, "scores",
                        result_file(param_file, dset, direction, args.real_perf) if args.dump_results else None)


def main(argv=None):
    return run(argv, "A2S")


if __name__ == "__main__":
    main()
