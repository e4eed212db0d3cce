#!/usr/bin/env python
"""Piece identification on scanned commercial scores ("UMC"), sheet -> audio ("S2A").  Command line of the reference's
umc_s2a_server.py (:29-40):

    python -m audio_sheet_retrieval_amd.umc_s2a_server --model models/mutopia_ccal_cont.py --data_dir <dir> \
        --train_split splits/all_split.yaml --config exp_configs/mutopia_full_aug.yaml \
        --init_audio_db --full_eval --dump_results [--real_perf] [--n_candidates 25] [--estimate_UV] \
        --system_params system_params.pkl --bar_params bar_params.pkl [--device_post] [--resample] [--page_width 835]
        [--deskew] [--flatten] [--crop]

The spectrograms of all pieces are loaded up front (a piece without its recording is an error that names the piece;
recordings at 22050 Hz, or with --resample at any sample rate, resampled on the device);
--init_audio_db embeds their excerpts (EmbeddingDB.from_specs: initialize_audio_db_from_specs) into
umc_audio_db_file.pkl in the working directory; --full_eval queries it with every piece's unrolled strip and
--dump_results writes umc_retrieval_<tag>_<dset>_S2A[_real].yaml.  --device_post, --resample, --page_width, --deskew,
--flatten and --crop as in umc_a2s_server.
The driver is umc_a2s_server.run in the S2A direction.
"""
from .umc_a2s_server import run


def main(argv=None):
    return run(argv, "S2A")


if __name__ == "__main__":
    main()
