#!/usr/bin/env python
"""Piece identification over whole test pieces, sheet -> audio ("S2A").  Command line of the reference's
sheet_audio_server.py (:26-34):

    python -m audio_sheet_retrieval_amd.sheet_audio_server --model models/mutopia_ccal_cont.py --data synthetic:16 \
        --train_split splits/all_split.yaml --config exp_configs/mutopia_full_aug.yaml \
        --init_audio_db --full_eval --dump_results [--n_candidates 25] [--estimate_UV]

--init_audio_db embeds the spectrogram excerpts of every test piece (initialize_audio_db, audio_sheet_server.py:356-394)
into audio_db_file.pkl in the working directory; --full_eval queries it with every piece's unrolled sheet
(detect_performance, :253-300) and --dump_results writes retrieval_<tag>_S2A.yaml.  The driver is
audio_sheet_server.run in the S2A direction.
"""
from .audio_sheet_server import run


def main(argv=None):
    return run(argv, "S2A")


if __name__ == "__main__":
    main()
