#!/usr/bin/env python
"""Fixtures of the staff-system detector (build container only; the reference tree never travels).

    python tests/golden/make_omr_golden.py      # -> tests/golden/omr_system_params.npz, omr_bar_params.npz,
                                                #    omr_tutorial_page.npz

Data only, no reference code:
  omr_{system,bar}_params.npz   sheet_utils/omr_models/{system,bar}_params.pkl: the 99 float32 arrays of each U-Net,
                                in the pickle's order, as p00 .. p98 (a Python-2 pickle of numpy arrays, read with
                                encoding='latin1')
  omr_tutorial_page.npz         tutorials/sheet_image.png as the uint8 grayscale array cv2.imread(path, 0) yields
                                (alpha dropped, fixed-point BT.601), converted by sheet_utils.omr.imread_gray
"""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    from audio_sheet_retrieval_amd.sheet_utils.omr import imread_gray
    for name in ("system", "bar"):
        with open(os.path.join(REF, "audio_sheet_retrieval", "sheet_utils", "omr_models", "%s_params.pkl" % name),
                  "rb") as fp:
            params = pickle.load(fp, encoding="latin1")
        assert len(params) == 99
        np.savez_compressed(os.path.join(HERE, "omr_%s_params.npz" % name),
                            **{"p%02d" % i: np.asarray(a, np.float32) for i, a in enumerate(params)})
    page = imread_gray(os.path.join(REF, "tutorials", "sheet_image.png"))
    assert page.shape == (1181, 835) and page.dtype == np.uint8
    np.savez_compressed(os.path.join(HERE, "omr_tutorial_page.npz"), page=page)


if __name__ == "__main__":
    main()
