"""load_umc_sheets of umc_a2s_server.py / umc_s2a_server.py: unrolled sheets of every piece under a data directory
(<piece>/sheet/*.png), with the systems of all pages detected in one device call per network - and, with
return_device, unrolled in one more (the strips stay on the device for the data base and the queries).  load_umc_scans:
the same for flat-bed scans, straightened and resized on the device first.  load_specs /
get_performance_audio_path: the recordings of the pieces (umc_a2s_server.py:28-45)."""
from __future__ import print_function

import glob
import os

import numpy as np

from audio_sheet_retrieval_amd.sheet_utils import bar_detector, note_detector, system_detector
from audio_sheet_retrieval_amd.sheet_utils.omr import (IN_U8_RAW, PAGE_WIDTH, SYSTEM_HEIGHT, DevicePages,
                                                       OpticalMusicRecognizer, SegmentationNetwork, imread_gray,
                                                       score_map_dev, unroll_rows, unroll_systems_dev, unwrap_systems)

OKBLUE, ENDC = "\033[94m", "\033[0m"       # utils/plotting.BColors


def build_recognizer(system_params, bar_params, device=0, note_params=None):
    """the system and bar networks - and, with note_params, the note-head network - with their parameters: pickle
    paths or lists of the 99 arrays"""
    system_net = SegmentationNetwork(system_detector.build_model(), device=device)
    system_net.load(system_params)
    bar_net = SegmentationNetwork(bar_detector.build_model(), device=device)
    bar_net.load(bar_params)
    note_net = None
    if note_params is not None:
        note_net = SegmentationNetwork(note_detector.build_model(), device=device)
        note_net.load(note_params)
    return OpticalMusicRecognizer(note_detector=note_net, system_detector=system_net, bar_detector=bar_net)


def get_performance_audio_path(piece_path, file_pattern):
    """the recording of a piece: the reference takes glob(piece_path/file_pattern*)[0]; here the sorted matches are
    tried in order and the first with a loadable extension wins (score_ppq.wav next to score_ppq.flac).  Without a
    loadable match the first match is returned (loading it names the format); IndexError without any match, as
    the reference."""
    from audio_sheet_retrieval_amd.audio_frontend import LOADABLE
    matches = sorted(glob.glob(os.path.join(piece_path, file_pattern + "*")))
    for path in matches:
        if os.path.splitext(path)[1].lower() in LOADABLE:
            return path
    return matches[0]


def load_specs(piece_paths, audio_file, processor, return_device=False, resample=False):
    """ Compute spectrograms given piece paths

    The recordings <piece_path>/<audio_file>* of all pieces, read with audio_frontend.load_audio and turned into
    (92, frames) spectrograms in one device call.  -> list of arrays; with return_device the
    piece_identification.DeviceArrays handle instead (the spectrograms stay on the device).  resample=True: the
    recordings may be at any sample rate (audio_frontend.read_audio) and are resampled on the device on the way."""
    from audio_sheet_retrieval_amd.audio_frontend import load_audio, read_audio
    recordings, scales, rates, integer = [], [], [], []
    for piece_path in piece_paths:
        try:
            audio_path = get_performance_audio_path(piece_path, audio_file)
        except IndexError:
            raise IOError("piece %s: no recording %s* in %s" % (os.path.basename(piece_path), audio_file, piece_path))
        if resample:
            samples, scale, rate, is_int = read_audio(audio_path)
            rates.append(rate)
            integer.append(is_int)
        else:
            samples, scale = load_audio(audio_path)
        recordings.append(samples)
        scales.append(scale)
    process = processor.process_many_dev if return_device else processor.process_many
    if resample:
        return process(recordings, scales, rates, integer)
    return process(recordings, scales)


class _PagesOnDevice(object):
    """the host side of resized pages that live in a DevicePages: a sequence whose entries are downloaded when they
    are asked for (the host post-processing reads every page, the device one only the pages it does not decide)"""

    def __init__(self, dev_pages):
        self.dev_pages = dev_pages
        self._host = {}

    def __len__(self):
        return len(self.dev_pages)

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        if i not in self._host:
            self._host[i] = self.dev_pages.download_page(i)
        return self._host[i]


def _next_stage(dev_pages, stage):
    """stage(dev_pages) -> the next DevicePages; the one it was made from is freed, also when the stage fails"""
    try:
        return stage(dev_pages)
    finally:
        dev_pages.free()


_CROPPED_STRIPS = []        # the class of _strips_with_crop, made once (piece_identification is imported late)


def _strips_with_crop(strips, rects, status):
    """the DeviceArrays `strips` as a DeviceArrays - the same three fields, a tuple of three as before - that also
    carries the crop of every raw page as .crop_rects (int32 (n_pages, 4): r0 r1 c0 c1) and .crop_status"""
    if not _CROPPED_STRIPS:
        from audio_sheet_retrieval_amd.piece_identification import DeviceArrays

        class CroppedStrips(DeviceArrays):
            pass                                                # no __slots__: instances take attributes
        _CROPPED_STRIPS.append(CroppedStrips)
    res = _CROPPED_STRIPS[0](*strips)
    res.crop_rects, res.crop_status = rects, status
    return res


def load_umc_sheets(data_dir, require_performance=False, omr=None, system_params=None, bar_params=None, device=0,
                    return_device=False, device_post=False, page_width=None):
    """ load unwarpped sheets

    Returns (piece_names, piece_paths, unwrapped_sheets) as the reference: pieces without a sheet directory (or,
    with require_performance, without a performance) are skipped, and so is every piece with a page on which system
    detection failed.  `omr`: an OpticalMusicRecognizer; otherwise one is built from system_params / bar_params.
    return_device=True: the pages are uploaded once, both networks and the unrolling read them on the device, and a
    fourth value is returned - the strips as a piece_identification.DeviceArrays (float32, 0..255; free its .buf when
    done).  The host strips are then the downloaded device strips; they equal the host unrolling bit for bit.
    device_post=True: the steps of detect_systems after the networks run on the device too
    (detect_systems_pages_dev); the systems are the same integers.
    page_width=W (the networks' width is omr.PAGE_WIDTH = 835): the pages may have any resolution.  They are uploaded
    once as they are and reduced to W columns on the device (DevicePages.resized: asr_resize_pages_dev, the shape rule
    of scripts/prepare_umc_data.py); the networks, the unrolling rules and the unroll see the resized pages.  On the
    host route they are downloaded once for unwrap_systems; with return_device a resized page comes to the host only
    where the post-processing reads it there (device_post=False: every page; device_post=True: a page the device does
    not decide).  None: the pages are taken as they are.
    The score map (bars and pages for strip positions) is an option of load_umc_scans, which with deskew=False and
    page_width=None is this function."""
    return _load_sheets(data_dir, require_performance, omr, system_params, bar_params, device, return_device, device_post,
                        page_width, False, 0)


def load_umc_scans(data_dir, require_performance=False, omr=None, system_params=None, bar_params=None, device=0,
                   return_device=False, device_post=False, page_width=PAGE_WIDTH, deskew=True, max_slope=64, flatten=False,
                   flatten_radius=None, flatten_floor=64, score_map=False, crop=False, crop_floor=64, crop_share=512,
                   crop_margin=None):
    """load_umc_sheets for flat-bed scans: pages of any resolution whose staves need not be horizontal, whose paper
    need not be white and need not fill the scanner's glass.  The raw pages are uploaded once; with crop (off by
    default) every page is first cut to the paper inside the scanner's black frame on the device (DevicePages.cropped:
    asr_crop_estimate_dev, asr_crop_pages_dev; crop_floor: a pixel below this is dark, crop_share: a border row or
    column is dark over this many 1/1024 of its central band, crop_margin None: by each page's width) - before
    everything else, so that the resize scales the paper, not the frame, to page_width; with return_device=True the
    returned strips then carry the rects as .crop_rects (int32 (n_pages, 4): r0 r1 c0 c1 in the pixels of the raw scans,
    every page of every piece that was read, in reading order) and .crop_status (1: undecided, the page was left whole).
    With flatten (off by default) every page is then divided by
    the grey closing of its paper on the device (DevicePages.flattened: asr_flatten_pages_dev; flatten_radius None: by
    each page's width, flatten_floor: a background darker than this is left alone) - before the deskew, whose shear
    fills the corners with white and whose score should read ink, not shadow; with deskew the slope of every page is
    estimated among -max_slope .. max_slope (in 1/1024 pixel per pixel) and the page sheared by it on the device
    (DevicePages.deskewed: asr_skew_estimate_dev, asr_deskew_pages_dev), then the pages are reduced to page_width columns
    (DevicePages.resized; None: left at their size) - the area resize after the shear takes the interpolation blur away
    again.  Everything downstream reads the result on the device, as in load_umc_sheets; the return values are the
    same.  With deskew=False and page_width=None (and no flatten, no crop) this is load_umc_sheets.
    score_map=True (with return_device=True and a bar network; ValueError otherwise): one more value is returned, the
    score_map.ScoreMap of the kept pieces - their measures in strip coordinates, built on the device from the bar
    network's maps in the pass that unrolls the pages (asr_score_map_dev).  The bar network runs once: the systems are
    then detected by the device post-processing whatever device_post says (the same integers), which hands its bar maps
    on.  Page coordinates in the map are those of the pages the networks saw, after crop, flatten, deskew and resize."""
    return _load_sheets(data_dir, require_performance, omr, system_params, bar_params, device, return_device, device_post,
                        page_width, deskew, max_slope, (flatten_radius, flatten_floor) if flatten else None,
                        score_map=score_map, crop=(crop_floor, crop_share, crop_margin) if crop else None)


def _load_sheets(data_dir, require_performance, omr, system_params, bar_params, device, return_device, device_post,
                 page_width, deskew, max_slope, flatten=None, score_map=False, crop=None):
    """the body of load_umc_sheets / load_umc_scans.  flatten: None, or (radius, floor) of DevicePages.flattened; crop:
    None, or (floor, share, margin) of DevicePages.cropped"""
    if score_map and not return_device:
        raise ValueError("score_map=True needs return_device=True: the map is built where the bar maps are")
    if omr is None:
        omr = build_recognizer(system_params, bar_params, device=device)
    if score_map and omr.bar_detector is None:
        raise ValueError("score_map=True needs a bar network")

    piece_names = []
    unwrapped_sheets = []
    piece_paths = []

    piece_dirs = np.sort(glob.glob(os.path.join(data_dir, '*')))
    n_pieces = len(piece_dirs)

    # pass 1: the reference's loop, collecting the pages; messages in its order
    jobs = []                                  # (piece_name, piece_dir, [page arrays])
    for i_piece, piece_dir in enumerate(piece_dirs):
        piece_name = piece_dir.split('/')[-1]
        print(OKBLUE + "Processing piece %d of %d (%s)" % (i_piece + 1, n_pieces, piece_name) + ENDC)
        if require_performance and len(glob.glob(os.path.join(piece_dir, "*performance*"))) == 0:
            print("No performance found!")
            continue
        page_paths = np.sort(glob.glob(os.path.join(piece_dir, "sheet/*.png")))
        if len(page_paths) == 0:
            print("No sheet available!!!")
            continue
        jobs.append((piece_name, piece_dir, [imread_gray(p) for p in page_paths]))

    # every page of every piece: one call per network (prepare_image on the device)
    all_pages = [I for _, _, pages in jobs for I in pages]
    dev_pages = None
    cropped = None                                              # (rects, status) of the raw pages
    if (page_width is not None or deskew or flatten is not None or crop is not None) and all_pages:
        from audio_sheet_retrieval_amd.sheet_utils.omr import _engine
        engine = omr.system_detector.engine or _engine(omr.system_detector.device)
        dev_pages = DevicePages(engine, all_pages)              # upload raw, then crop, flatten, deskew, resize
        if crop is not None:
            dev_pages = _next_stage(dev_pages, lambda pages: pages.cropped(*crop))
            cropped = (dev_pages.rects, dev_pages.crop_status)
        if flatten is not None:
            dev_pages = _next_stage(dev_pages, lambda pages: pages.flattened(*flatten))
        if deskew:
            dev_pages = _next_stage(dev_pages, lambda pages: pages.deskewed(max_slope))
        if page_width is not None:
            dev_pages = _next_stage(dev_pages, lambda pages: pages.resized(page_width))
    if return_device:
        res = _unroll_on_device(omr, jobs, all_pages, device_post=device_post, dev_pages=dev_pages, score_map=score_map)
        if crop is not None:
            rects, status = cropped if cropped is not None else (np.zeros((0, 4), np.int32), np.zeros(0, np.int32))
            res = res[:3] + (_strips_with_crop(res[3], rects, status),) + res[4:]
        return res
    detect = omr.detect_systems_pages_dev if device_post else omr.detect_systems_pages
    if dev_pages is not None:
        try:
            all_pages = dev_pages.download()
            k = 0
            for j, (piece_name, piece_dir, pages) in enumerate(jobs):
                jobs[j] = (piece_name, piece_dir, all_pages[k:k + len(pages)])
                k += len(pages)
            results = detect(all_pages, in_mode=IN_U8_RAW, dev_pages=dev_pages)
        finally:
            dev_pages.free()
    else:
        results = detect(all_pages, in_mode=IN_U8_RAW) if all_pages else []

    kept_pages = 0
    k = 0
    for piece_name, piece_dir, pages in jobs:
        unwrapped_sheet = np.zeros((SYSTEM_HEIGHT, 0), dtype=np.uint8)
        system_problem = False
        for I in pages:
            kept_pages += 1
            page_systems = results[k]
            k += 1
            if isinstance(page_systems, Exception):
                print("Problem in system detection!!!")
                system_problem = True
                continue
            unwrapped_sheet = np.hstack((unwrapped_sheet, unwrap_systems(I, page_systems, SYSTEM_HEIGHT)))
        if not system_problem:
            piece_names.append(piece_name)
            piece_paths.append(piece_dir)
            unwrapped_sheets.append(unwrapped_sheet)

    print("%d pieces covering %d pages of sheet music." % (len(piece_names), kept_pages))
    return piece_names, piece_paths, unwrapped_sheets


def _unroll_on_device(omr, jobs, all_pages, device_post=False, dev_pages=None, score_map=False):
    """the second half of load_umc_sheets with the pages resident on the device.  dev_pages: the resized pages, where
    load_umc_sheets resized them (freed here); otherwise all_pages are uploaded.  score_map: the bar maps stay on the
    device until the unroll rows are known, and the ScoreMap of the kept pieces is returned as a fifth value"""
    from audio_sheet_retrieval_amd.piece_identification import DeviceArrays
    from audio_sheet_retrieval_amd.sheet_utils.omr import _engine
    if dev_pages is None:
        engine = omr.system_detector.engine or _engine(omr.system_detector.device)
        dev_pages = DevicePages(engine, all_pages)
    else:
        all_pages = _PagesOnDevice(dev_pages)
    bar_maps = None
    try:
        if score_map:
            results, bar_maps = omr.detect_systems_keep_bars_dev(all_pages, in_mode=IN_U8_RAW, dev_pages=dev_pages) \
                if all_pages else ([], None)
        else:
            detect = omr.detect_systems_pages_dev if device_post else omr.detect_systems_pages
            results = detect(all_pages, in_mode=IN_U8_RAW, dev_pages=dev_pages) if all_pages else []
        piece_names, piece_paths = [], []
        kept_pages = 0
        k = 0
        page_rows, piece_of_page = [None] * len(all_pages), np.zeros(len(all_pages), np.int64)
        for piece_name, piece_dir, pages in jobs:
            first = k
            system_problem = False
            for _ in pages:
                kept_pages += 1
                if isinstance(results[k], Exception):
                    print("Problem in system detection!!!")
                    system_problem = True
                else:                       # the reference unrolls the good pages of a piece it drops, too: messages
                    page_shape = (int(dev_pages.heights[k]), int(dev_pages.widths[k]))
                    page_rows[k] = unroll_rows(page_shape, results[k], SYSTEM_HEIGHT, with_index=score_map)
                k += 1
            if system_problem:
                page_rows[first:k] = [None] * (k - first)
            else:
                piece_of_page[first:k] = len(piece_names)
                piece_names.append(piece_name)
                piece_paths.append(piece_dir)
        buf, offsets, shapes = unroll_systems_dev(dev_pages, page_rows, piece_of_page, len(piece_names), SYSTEM_HEIGHT)
        if score_map:
            from audio_sheet_retrieval_amd.score_map import ScoreMap
            try:
                measures, piece_first = score_map_dev(bar_maps, page_rows, piece_of_page, len(piece_names)) \
                    if bar_maps is not None else (np.zeros((0, 8), np.int32), np.zeros(1, np.int32))
                the_map = ScoreMap.from_table(piece_names, measures, piece_first, [c for _, c in shapes])
            except Exception:
                buf.free()
                raise
    finally:
        dev_pages.free()
        if bar_maps is not None:
            bar_maps.free()
    total = sum(r * c for r, c in shapes)
    flat = buf.download((total,), np.float32) if total else np.zeros(0, np.float32)
    unwrapped_sheets = [flat[o:o + r * c].reshape(r, c).astype(np.uint8) for o, (r, c) in zip(offsets, shapes)]
    print("%d pieces covering %d pages of sheet music." % (len(piece_names), kept_pages))
    if score_map:
        return piece_names, piece_paths, unwrapped_sheets, DeviceArrays(buf, offsets, shapes), the_map
    return piece_names, piece_paths, unwrapped_sheets, DeviceArrays(buf, offsets, shapes)
