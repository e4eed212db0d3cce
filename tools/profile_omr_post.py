#!/usr/bin/env python
"""A few detect_systems_pages_dev calls on copies of the tutorial page and its mirror, to be run under the profiler:

    rocprofv3 --kernel-trace --stats -d <dir> -o r13_omr_post -- python tools/profile_omr_post.py [--pages 16] [--calls 3]

The per-kernel device time of asr_systems_from_maps_dev (the post_* kernels) is read from the kernel statistics; the
U-Net kernels of the two networks are in the same trace.  Prints one JSON line: pages, calls, labelling passes of one
call and of the tutorial page alone, fallback pages, systems found.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pages", type=int, default=16)
    p.add_argument("--calls", type=int, default=3)
    a = p.parse_args()
    import omr_ref
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    from audio_sheet_retrieval_amd.sheet_utils.umc import build_recognizer
    rec = build_recognizer(omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz")),
                           omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_bar_params.npz")))
    page = np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]
    variants = [page, np.ascontiguousarray(page[:, ::-1])]
    rec.detect_systems_pages_dev([page], in_mode=O.IN_U8_RAW)
    passes_one = rec.last_label_passes
    pages = [variants[i % 2] for i in range(a.pages)]
    for _ in range(a.calls):
        out = rec.detect_systems_pages_dev(pages, in_mode=O.IN_U8_RAW)
    print(json.dumps(dict(pages=a.pages, calls=a.calls, label_passes_tutorial_page=passes_one,
                          label_passes_call=rec.last_label_passes, fallback_pages=rec.last_fallback_pages,
                          systems=int(sum(len(s) for s in out if not isinstance(s, Exception))))))


if __name__ == "__main__":
    main()
