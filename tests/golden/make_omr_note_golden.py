#!/usr/bin/env python
"""Fixture of the note-head detector (build container only; the reference tree never travels).

    python tests/golden/make_omr_note_golden.py      # -> tests/golden/omr_note_params.npz

Data only, no reference code: sheet_utils/omr_models/note_params.pkl, the 99 float32 arrays of the note U-Net in the
pickle's order, as p00 .. p98 (a Python-2 pickle of numpy arrays, read with encoding='latin1') - the layout of
omr_system_params.npz and omr_bar_params.npz (make_omr_golden.py).
"""
import os
import pickle

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    with open(os.path.join(REF, "audio_sheet_retrieval", "sheet_utils", "omr_models", "note_params.pkl"), "rb") as fp:
        params = pickle.load(fp, encoding="latin1")
    assert len(params) == 99 and sum(int(np.asarray(a).size) for a in params) == 110033
    np.savez_compressed(os.path.join(HERE, "omr_note_params.npz"),
                        **{"p%02d" % i: np.asarray(a, np.float32) for i, a in enumerate(params)})


if __name__ == "__main__":
    main()
