"""Record tests/golden/omr_tutorial_bar_counts.npz: the column counts of the six systems of the tutorial page at
threshold 0.5 (sheet_utils/omr.strip_bar_counts_host), from the reference's weights through the float32 numpy U-Net of
tests/omr_ref.py, with the systems' unroll rows.  CPU only, about ten seconds.

    python tools/record_score_map_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import omr_ref  # noqa: E402
from audio_sheet_retrieval_amd.sheet_utils import omr as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    page = np.load(os.path.join(GOLDEN, "omr_tutorial_page.npz"))["page"]
    ps = omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_system_params.npz"))
    pb = omr_ref.params_from_npz(os.path.join(GOLDEN, "omr_bar_params.npz"))
    x = O.prepare_image(page)
    sp = omr_ref.sliding_window(x, (512, 512), lambda t: omr_ref.unet_forward(t, ps, dtype=np.float32))
    bp = omr_ref.sliding_window(x, (256, 512), lambda t: omr_ref.unet_forward(t, pb, dtype=np.float32))
    systems = O.systems_from_maps(x, sp, bp)
    rows = O.unroll_rows(page.shape, systems, with_index=True)
    counts = [O.strip_bar_counts_host(bp, r0, r1, c0, c1, 0.5) for r0, r1, c0, c1, _, _ in rows]
    out = os.path.join(GOLDEN, "omr_tutorial_bar_counts.npz")
    np.savez_compressed(out, rows=np.asarray(rows, np.int32), threshold=np.float64(0.5), page_shape=np.asarray(page.shape),
                        counts=np.concatenate(counts).astype(np.int16))
    table, first = O.score_map_host(None, [rows], [0], 1, counts=counts)
    print(out, os.path.getsize(out), "bytes;", len(table), "measures; x0 =", table[:, 0].tolist(), "width", table[-1, 1])


if __name__ == "__main__":
    main()
