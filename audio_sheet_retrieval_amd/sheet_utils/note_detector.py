"""sheet_utils/note_detector.py: the note-head U-Net, system_detector's graph on 1 x 256 x 512 tiles."""
from audio_sheet_retrieval_amd.sheet_utils.system_detector import UNet, param_shapes  # noqa: F401

INPUT_SHAPE = [1, 256, 512]


def build_model(in_shape=INPUT_SHAPE):
    """Compile net architecture"""
    return UNet(in_shape)
