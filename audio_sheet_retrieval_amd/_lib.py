"""ctypes binding of libasr_hip.so (include/asr_hip.h) and a thin `Engine` object.

There is NO CPU fallback: if the library is missing or no HIP device is
available every entry point raises (AsrLibraryError / AsrError).  The oracle
under oracle/ is test infrastructure and is never imported from here.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libasr_hip.so")

ASR_OK = 0
ASR_ERR_INVALID, ASR_ERR_HIP, ASR_ERR_STATE, ASR_ERR_COMM, ASR_ERR_NOMEM = 1, 2, 3, 4, 5      # include/asr_hip.h
IN_F32_PREPARED, IN_F32_RAW, IN_U8_RAW = 0, 1, 2
OUT_LATENT, OUT_FEATURES = 0, 1
SYSTEM_MIN_AREA = 50000            # detect_systems: smallest system blob (asr_systems_from_maps_dev's capacity rule)

#: every symbol include/asr_hip.h declares (tests check the .so exports them all)
EXPORTS = [
    "asr_create", "asr_destroy", "asr_last_error", "asr_version", "asr_sync", "asr_set_input_size",
    "asr_param_count", "asr_param_size", "asr_set_params", "asr_get_params", "asr_set_cca",
    "asr_embed_view1", "asr_embed_view2", "asr_embed_view1_dev", "asr_embed_view2_dev", "asr_embed_both",
    "asr_rank", "asr_rank_dev", "asr_topk", "asr_topk_dev", "asr_cca_fit", "asr_cca_fit_dev",
    "asr_db_create", "asr_db_refresh", "asr_db_destroy", "asr_db_size", "asr_topk_db_dev", "asr_rank_db_dev",
    "asr_topk_rank_db_dev", "asr_rank_dstar_db_dev", "asr_topk_count_db_dev", "asr_topk_merge_dev", "asr_rank_finish_dev",
    "asr_dev_alloc", "asr_dev_free", "asr_dev_upload", "asr_dev_download",
    "asr_host_alloc", "asr_host_free", "asr_eval_batches",
    "asr_profile_enable", "asr_profile_filter", "asr_profile_reset", "asr_profile_count", "asr_profile_get", "asr_profile_symbol",
    "asr_debug_activation",
    "asr_train_begin", "asr_train_end", "asr_train_set_global_batch", "asr_train_step", "asr_train_step_dev", "asr_valid_loss", "asr_set_objective", "asr_burn_in",
    "asr_compute_gradients", "asr_train_step_in", "asr_train_step_in_dev", "asr_burn_in_in", "asr_compute_gradients_in",
    "asr_valid_loss_in", "asr_valid_output_in", "asr_valid_output_in_dev",
    "asr_comm_unique_id", "asr_comm_init", "asr_comm_init_custom", "asr_comm_destroy", "asr_comm_info", "asr_comm_stats", "asr_comm_timing", "asr_comm_library",
    "asr_comm_allreduce_dev", "asr_comm_allgather_dev",
    "asr_rank_sharded_dev", "asr_slice_windows_dev", "asr_piece_vote_dev", "asr_piece_vote_batch_dev", "asr_track_gate_dev", "asr_track_vote_batch_dev", "asr_gather_windows_dev", "asr_dtw_dev", "asr_dtw_batch_dev", "asr_dtw_subseq_batch_dev", "asr_dtw_follow_batch_dev", "asr_spectrogram_dev", "asr_debug_tune_report",
    "asr_seg_create", "asr_seg_set_window", "asr_seg_destroy", "asr_seg_predict_dev", "asr_systems_from_maps_dev",
    "asr_notes_from_map_dev", "asr_bars_from_map_dev",
    "asr_unroll_systems_dev", "asr_spectrogram_batch_dev", "asr_spectrogram_fft_batch_dev", "asr_resample_batch_dev", "asr_resize_pages_dev",
    "asr_audio_stream_push_dev", "asr_audio_stream_push_fft_dev", "asr_skew_estimate_dev", "asr_deskew_pages_dev",
    "asr_flatten_pages_dev", "asr_score_map_dev", "asr_crop_estimate_dev", "asr_crop_pages_dev",
    "asr_track_stream_gate_dev", "asr_track_stream_vote_dev",
    "asr_track_gate_running_dev", "asr_track_stream_gate_running_dev",
    "asr_follow_stream_windows_dev", "asr_follow_stream_log_dev",
    "asr_opt_state_size", "asr_get_opt_state", "asr_set_opt_state", "asr_debug_train_tensor", "asr_cca_train_debug",
    "asr_debug_train_candidate",
]


#: host-callback transport of asr_comm_init_custom (include/asr_hip.h)
ALLREDUCE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_int64, c_int)
ALLGATHER_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_void_p, c_int64)
COMM_ID_BYTES = 128
DTYPE_F32, DTYPE_F64, DTYPE_I32 = 0, 1, 2


class AsrLibraryError(ImportError):
    """libasr_hip.so is missing or cannot be loaded."""


class AsrError(RuntimeError):
    """An asr_* call returned a non-zero status."""

    def __init__(self, code, message):
        super().__init__("asr error %d: %s" % (code, message))
        self.code = code


class AsrConfig(ctypes.Structure):
    _fields_ = [
        ("struct_size", c_int32), ("device", c_int32), ("num_filters", c_int32), ("resize_view1", c_int32),
        ("h1", c_int32), ("w1", c_int32), ("h2", c_int32), ("w2", c_int32),
        ("dim_latent", c_int32), ("max_chunk", c_int32),
        ("r1", c_float), ("r2", c_float), ("rT", c_float), ("alpha", c_float), ("gamma", c_float), ("l2", c_float),
        ("pool_ties", c_int32),
    ]


# asr_config.pool_ties: which elements of a 2x2 pooling window with several equal maxima receive the gradient
POOL_TIES = {"all": 0, "first": 1}


_lib = None


def load_library(path=None):
    """dlopen libasr_hip.so and declare the prototypes; raises AsrLibraryError."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    # multi-process GPU work on this platform (RCCL at world > 1, IPC handles) needs dmabuf IPC: the variable has to be
    # in place before the HSA runtime initialises, i.e. before the first HIP call of the process - this is that point.
    # An explicit setting of the caller wins.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not os.path.exists(p):
        raise AsrLibraryError(
            "%s not found - build it with `python -m audio_sheet_retrieval_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback." % p)
    try:
        lib = ctypes.CDLL(p)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise AsrLibraryError("cannot load %s: %s" % (p, e))
    fpp = POINTER(POINTER(c_float))
    i64p = POINTER(c_int64)
    proto = {
        "asr_create": (c_int, [POINTER(AsrConfig), POINTER(c_void_p)]),
        "asr_destroy": (None, [c_void_p]),
        "asr_last_error": (c_char_p, [c_void_p]),
        "asr_version": (c_char_p, []),
        "asr_sync": (c_int, [c_void_p]),
        "asr_set_input_size": (c_int, [c_void_p, c_int, c_int, c_int]),
        "asr_param_count": (c_int, [c_void_p]),
        "asr_param_size": (c_int, [c_void_p, c_int, i64p]),
        "asr_set_params": (c_int, [c_void_p, fpp, i64p, c_int]),
        "asr_get_params": (c_int, [c_void_p, fpp, i64p, c_int]),
        "asr_set_cca": (c_int, [c_void_p] + [c_void_p] * 4),
        "asr_embed_view1": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p]),
        "asr_embed_view2": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
        "asr_embed_view1_dev": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p]),
        "asr_embed_view2_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
        "asr_rank": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int,
                             c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
        "asr_rank_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int,
                                 c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
        "asr_topk": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_int,
                             c_int64, c_void_p, c_void_p]),
        "asr_topk_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_int,
                                 c_int64, c_void_p, c_void_p]),
        "asr_db_create": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, POINTER(c_void_p)]),
        "asr_db_refresh": (c_int, [c_void_p, c_void_p]),
        "asr_db_destroy": (c_int, [c_void_p, c_void_p]),
        "asr_db_size": (c_int, [c_void_p, c_void_p, i64p, POINTER(c_int)]),
        "asr_topk_db_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int64, c_void_p, c_void_p]),
        "asr_rank_db_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                    c_void_p]),
        "asr_topk_rank_db_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int64, c_void_p, c_void_p,
                                         c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
        "asr_rank_dstar_db_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                          c_void_p, c_void_p]),
        "asr_topk_count_db_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int64, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
        "asr_topk_merge_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_void_p,
                                       c_void_p]),
        "asr_rank_finish_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
        "asr_cca_fit": (c_int, [c_void_p, c_void_p, c_void_p, c_int64] + [c_void_p] * 5),
        "asr_cca_fit_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64] + [c_void_p] * 4),
        "asr_host_alloc": (c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
        "asr_host_free": (c_int, [c_void_p, c_void_p]),
        "asr_eval_batches": (c_int, [c_void_p, POINTER(c_void_p), c_int, POINTER(c_void_p), c_int, c_int64,
                                     POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                     POINTER(c_void_p)]),
        "asr_dev_alloc": (c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
        "asr_dev_free": (c_int, [c_void_p, c_void_p]),
        "asr_dev_upload": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
        "asr_dev_download": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
        "asr_profile_enable": (c_int, [c_void_p, c_int]),
        "asr_profile_filter": (c_int, [c_void_p, c_char_p]),
        "asr_profile_reset": (c_int, [c_void_p]),
        "asr_profile_count": (c_int, [c_void_p]),
        "asr_profile_get": (c_int, [c_void_p, c_int, c_char_p, c_int, i64p, POINTER(c_double),
                                    POINTER(c_double), POINTER(c_double)]),
        "asr_profile_symbol": (c_int, [c_void_p, c_int, c_char_p, c_int]),
        "asr_debug_activation": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p,
                                         POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
        "asr_train_begin": (c_int, [c_void_p, c_int]),
        "asr_train_end": (c_int, [c_void_p]),
        "asr_train_set_global_batch": (c_int, [c_void_p, c_int64]),
        "asr_train_step": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, POINTER(c_float), c_void_p]),
        "asr_train_step_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, POINTER(c_float), c_void_p]),
        "asr_valid_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(c_float)]),
        "asr_set_objective": (c_int, [c_void_p, c_float, c_float, c_int]),
        "asr_burn_in": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
        "asr_compute_gradients": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, POINTER(c_float)]),
        "asr_train_step_in": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_float, POINTER(c_float), c_void_p]),
        "asr_train_step_in_dev": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_float, POINTER(c_float),
                                          c_void_p]),
        "asr_burn_in_in": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
        "asr_compute_gradients_in": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64,
                                             POINTER(c_float)]),
        "asr_valid_loss_in": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, POINTER(c_float)]),
        "asr_valid_output_in": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, POINTER(c_float), c_void_p,
                                        c_void_p]),
        "asr_valid_output_in_dev": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
        "asr_slice_windows_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_int,
                                          c_void_p]),
        "asr_piece_vote_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int, c_void_p, c_void_p,
                                       POINTER(c_int32)]),
        "asr_seg_create": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, POINTER(c_void_p)]),
        "asr_seg_set_window": (c_int, [c_void_p, c_void_p, c_void_p]),
        "asr_seg_destroy": (c_int, [c_void_p, c_void_p]),
        "asr_seg_predict_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                        c_double, c_void_p]),
        "asr_systems_from_maps_dev": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
        "asr_notes_from_map_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_double, c_double,
                                           c_int, c_int, c_void_p, c_void_p, c_void_p]),
        "asr_bars_from_map_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
        "asr_piece_vote_batch_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int32, c_int]
                                     + [c_void_p] * 6),
        "asr_track_gate_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int] + [c_void_p] * 5 + [c_int] + [c_void_p] * 3),
        "asr_track_vote_batch_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                             c_void_p, c_int64, c_int32, c_int, c_void_p, c_void_p, c_void_p]),
        "asr_track_stream_gate_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int] + [c_void_p] * 4 + [c_int, c_int, c_void_p,
                                              c_int64, c_void_p, c_void_p, c_int64] + [c_void_p] * 3),
        "asr_track_stream_vote_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int, c_int,
                                              c_void_p, c_int64, c_int32, c_int, c_void_p, c_int64] + [c_void_p] * 4),
        "asr_track_gate_running_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int] + [c_void_p] * 3 +
                                       [c_int, c_int, ctypes.c_float] + [c_void_p] * 3),
        "asr_track_stream_gate_running_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int] + [c_void_p] * 3 +
                                              [c_int, ctypes.c_float, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p,
                                               c_int64, c_void_p, c_void_p, c_int64] + [c_void_p] * 4),
        "asr_follow_stream_windows_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int] + [c_void_p] * 3 +
                                          [c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
        "asr_follow_stream_log_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int, c_int,
                                              c_void_p, c_int64, c_void_p]),
        "asr_gather_windows_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_void_p]),
        "asr_dtw_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                POINTER(c_int32), POINTER(c_double)]),
        "asr_dtw_batch_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 7),
        "asr_dtw_subseq_batch_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64] + [c_void_p] * 4 +
                                     [c_int, c_int] + [c_void_p] * 5),
        "asr_dtw_follow_batch_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64] + [c_void_p] * 5 +
                                     [c_int, c_int, c_void_p, c_void_p, c_int64] + [c_void_p] * 4),
        "asr_spectrogram_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int, c_float, c_float, c_int64, c_int, c_void_p]),
        "asr_unroll_systems_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                           c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int64]),
        "asr_spectrogram_batch_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                              c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                              c_float, c_int, c_void_p, c_int64]),
        "asr_spectrogram_fft_batch_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                                  c_float, c_float, c_int, c_void_p, c_int64]),
        "asr_resample_batch_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                           c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int64]),
        "asr_resize_pages_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_int64]),
        "asr_skew_estimate_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                          c_void_p, c_void_p]),
        "asr_deskew_pages_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                         c_int, c_void_p, c_int64]),
        "asr_flatten_pages_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                          c_int, c_void_p, c_int64, c_void_p]),
        "asr_crop_estimate_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
        "asr_crop_pages_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                       c_void_p, c_int64]),
        "asr_score_map_dev": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                      c_int, c_int, c_double, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
        "asr_audio_stream_push_dev": (c_int, [c_void_p, c_void_p, c_int64] + [c_void_p] * 7 + [c_int, c_int, c_int,
                                              c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64,
                                              c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                              c_float, c_int, c_void_p, c_int64]),
        "asr_audio_stream_push_fft_dev": (c_int, [c_void_p, c_void_p, c_int64] + [c_void_p] * 7 + [c_int, c_int, c_int,
                                                  c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64,
                                                  c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                                  c_float, c_int, c_void_p, c_int64]),
        "asr_debug_tune_report": (c_int, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_float)]),
        "asr_comm_unique_id": (c_int, [c_void_p]),
        "asr_comm_init": (c_int, [c_void_p, c_int, c_int, c_void_p]),
        "asr_comm_init_custom": (c_int, [c_void_p, c_int, c_int, ALLREDUCE_FN, ALLGATHER_FN, c_void_p]),
        "asr_comm_destroy": (c_int, [c_void_p]),
        "asr_comm_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
        "asr_comm_stats": (c_int, [c_void_p, i64p, c_int]),
        "asr_comm_timing": (c_int, [c_void_p, c_int, POINTER(ctypes.c_double), i64p]),
        "asr_comm_library": (c_int, [c_void_p, c_char_p, c_int]),
        "asr_comm_allreduce_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int]),
        "asr_comm_allgather_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
        "asr_rank_sharded_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
        "asr_embed_both": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
        "asr_opt_state_size": (c_int, [c_void_p, i64p]),
        "asr_get_opt_state": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(c_int32)]),
        "asr_set_opt_state": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32]),
        "asr_debug_train_tensor": (c_int, [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_int64, i64p]),
        "asr_cca_train_debug": (c_int, [c_void_p, c_void_p, c_void_p, c_int64] + [c_void_p] * 7),
        "asr_debug_train_candidate": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                              c_int64, c_void_p, c_void_p, c_void_p, c_int64]),
    }
    for name, (res, args) in proto.items():
        fn = getattr(lib, name)      # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path is None and os.environ.get("ASR_ALLOW_STALE_LIB") != "1":
        # a stale binary next to newer sources would silently run old kernels: asr_version() carries the hash
        from . import build as _build
        built = (lib.asr_version() or b"").decode()
        want = _build.source_hash()
        if "src:" + want not in built:
            raise AsrLibraryError("%s was built from other sources (%s, sources now %s): re-run "
                                  "`python -m audio_sheet_retrieval_amd.build`" % (p, built, want))
    if path is None:
        _lib = lib
    return lib


#: reference model modules -> library configuration (models/mutopia_ccal_cont*.py)
MODEL_CONFIGS = {
    "mutopia_ccal_cont": dict(num_filters=12, resize_view1=0),
    "mutopia_ccal_cont_rsz": dict(num_filters=24, resize_view1=1),
}


def _f32c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class DeviceBuffer(object):
    """A library-owned device allocation (plain pointer + size)."""

    def __init__(self, engine, nbytes):
        self.engine, self.nbytes = engine, int(nbytes)
        p = c_void_p()
        engine._check(engine.lib.asr_dev_alloc(engine.ctx, self.nbytes, byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.engine._check(self.engine.lib.asr_dev_upload(self.engine.ctx, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.engine._check(self.engine.lib.asr_dev_download(self.engine.ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def offset(self, nbytes):
        return self.ptr + int(nbytes)

    def free(self):
        if self.ptr:
            self.engine._check(self.engine.lib.asr_dev_free(self.engine.ctx, self.ptr))
            self.ptr = None


class CodeDB(object):
    """asr_db handle: a resident candidate pool.  The rows stay in the caller's device buffer (keep it alive);
    refresh() after changing them in place."""

    def __init__(self, engine, codes_ptr, n, dim=32, ld=32):
        self.engine, self.n, self.dim = engine, int(n), int(dim)
        h = c_void_p()
        engine._check(engine.lib.asr_db_create(engine.ctx, codes_ptr, self.n, int(ld), self.dim, byref(h)))
        self.handle = h
        # the context owns the handle's device buffers (norms, reciprocal norms, unit rows: ~136 B per row): the engine
        # destroys the data bases that are still open when IT closes, whatever order the caller drops things in.  The
        # registry is a WeakSet: a handle the caller simply drops is collected (and __del__ frees its buffers) instead
        # of living until Engine.close() - a server that builds a data base per request must not pile them up
        engine._open_dbs.add(self)

    def refresh(self):
        self.engine._check(self.engine.lib.asr_db_refresh(self.engine.ctx, self.handle))

    def topk_dev(self, q_ptr, n_q, k, idx_ptr, dist_ptr, ld=32, idx_offset=0):
        self.engine._check(self.engine.lib.asr_topk_db_dev(self.engine.ctx, self.handle, q_ptr, n_q, ld, k, idx_offset,
                                                           idx_ptr, dist_ptr))

    def rank_dev(self, lv1_ptr, n1, ranks_ptr, dstar_ptr, ties_ptr, ld=32, query_offset=0, n1_global=None):
        self.engine._check(self.engine.lib.asr_rank_db_dev(self.engine.ctx, self.handle, lv1_ptr, n1, ld, query_offset,
                                                           n1 if n1_global is None else n1_global, ranks_ptr, dstar_ptr,
                                                           ties_ptr))

    def topk_rank_dev(self, q_ptr, n_q, k, idx_ptr, dist_ptr, ranks_ptr, dstar_ptr, ties_ptr, ld=32, idx_offset=0,
                      query_offset=0, n1_global=None):
        self.engine._check(self.engine.lib.asr_topk_rank_db_dev(
            self.engine.ctx, self.handle, q_ptr, n_q, ld, k, idx_offset, idx_ptr, dist_ptr, query_offset,
            n_q if n1_global is None else n1_global, ranks_ptr, dstar_ptr, ties_ptr))

    # -- this data base as one shard of a larger pool (query-sharded retrieval) --
    def rank_dstar_dev(self, q_ptr, n_q, item_offset, n2_global, query_offset, n1_global, dstar_ptr, jstar_ptr, ld=32):
        self.engine._check(self.engine.lib.asr_rank_dstar_db_dev(self.engine.ctx, self.handle, q_ptr, n_q, ld, item_offset,
                                                                 n2_global, query_offset, n1_global, dstar_ptr, jstar_ptr))

    def topk_count_dev(self, q_ptr, n_q, k, item_offset, idx_ptr, dist_ptr, dstar_ptr, jstar_ptr, counts_ptr, ld=32):
        self.engine._check(self.engine.lib.asr_topk_count_db_dev(self.engine.ctx, self.handle, q_ptr, n_q, ld, k, item_offset,
                                                                 idx_ptr, dist_ptr, dstar_ptr, jstar_ptr, counts_ptr))

    def topk(self, queries, k, idx_offset=0):
        """host queries (Q, dim) -> (idx (Q,k) int32, dist (Q,k) float64), like Engine.topk against the pool"""
        q = _f32c(queries)
        eng = self.engine
        dq = eng.alloc(max(q.nbytes, 4)).upload(q)
        di, dd = eng.alloc(max(q.shape[0] * k * 4, 4)), eng.alloc(max(q.shape[0] * k * 8, 8))
        try:
            self.topk_dev(dq.ptr, q.shape[0], k, di.ptr, dd.ptr, ld=q.shape[1], idx_offset=idx_offset)
            return di.download((q.shape[0], k), np.int32), dd.download((q.shape[0], k), np.float64)
        finally:
            for b in (dq, di, dd):
                b.free()

    def close(self):
        if getattr(self, "handle", None) is not None and getattr(self.engine, "ctx", None):
            self.engine.lib.asr_db_destroy(self.engine.ctx, self.handle)
        self.handle = None
        try:
            self.engine._open_dbs.discard(self)
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(object):
    """One asr_ctx: network state on one GPU.  Mirrors what build_model() +
    theano.function(...) give the reference (models/mutopia_ccal_cont.py:61-149,
    run_eval.py:92-95)."""

    def __init__(self, model_name="mutopia_ccal_cont", device=0, h1=160, w1=200, h2=92, w2=42,
                 max_chunk=0, r1=1e-3, r2=1e-3, rT=1e-3, alpha=1.0, gamma=0.7, l2=1e-5, lib=None, pool_ties=None):
        if model_name not in MODEL_CONFIGS:
            raise ValueError("unknown model %r (have %s)" % (model_name, sorted(MODEL_CONFIGS)))
        self.lib = lib or load_library()
        self._open_dbs = weakref.WeakSet()
        mc = MODEL_CONFIGS[model_name]
        self.model_name = model_name
        # pool_ties: "all" (default; Theano's CPU MaxPoolGrad - every element equal to the window maximum receives the
        # gradient) or "first"; ASR_POOL_TIES in the environment sets the default of a process
        if pool_ties is None:
            pool_ties = os.environ.get("ASR_POOL_TIES", "all")
        if pool_ties not in POOL_TIES:
            raise ValueError("pool_ties must be one of %s, got %r" % (sorted(POOL_TIES), pool_ties))
        self.pool_ties = pool_ties
        cfg = AsrConfig(ctypes.sizeof(AsrConfig), device, mc["num_filters"], mc["resize_view1"],
                        h1, w1, h2, w2, 32, max_chunk, r1, r2, rT, alpha, gamma, l2, POOL_TIES[pool_ties])
        self.cfg = cfg
        ctx = c_void_p()
        rc = self.lib.asr_create(byref(cfg), byref(ctx))
        if rc != ASR_OK:
            raise AsrError(rc, (self.lib.asr_last_error(None) or b"").decode())
        self.ctx = ctx
        self.net_h1 = h1 // 2 if mc["resize_view1"] else h1
        self.net_w1 = w1 // 2 if mc["resize_view1"] else w1

    # -- plumbing ---------------------------------------------------------
    def _check(self, rc):
        if rc != ASR_OK:
            raise AsrError(rc, (self.lib.asr_last_error(self.ctx) or b"").decode())

    def close(self):
        if getattr(self, "ctx", None):
            for db in list(getattr(self, "_open_dbs", ())):     # before asr_destroy: afterwards their buffers could not be freed
                db.close()
            for p in list(getattr(self, "_pinned", {}).values()):
                self.lib.asr_host_free(self.ctx, p)
            self._pinned = {}
            self.lib.asr_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self.lib.asr_sync(self.ctx))

    # -- piece identification (audio_sheet_server.py:213-300) ----------------------
    def slice_windows_dev(self, src_ptr, rows, T, r0, win_h, win_w, starts, out_ptr):
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        self._check(self.lib.asr_slice_windows_dev(self.ctx, src_ptr, rows, T, r0, win_h, win_w, starts.ctypes.data,
                                                   starts.size, out_ptr))

    def piece_vote_dev(self, idx_ptr, n_idx, ids_ptr, n_db, n_pieces, top_k):
        pieces, counts = np.empty(top_k, np.int32), np.empty(top_k, np.int32)
        m = c_int32()
        self._check(self.lib.asr_piece_vote_dev(self.ctx, idx_ptr, n_idx, ids_ptr, n_db, n_pieces, top_k,
                                                pieces.ctypes.data, counts.ctypes.data, byref(m)))
        return pieces[:m.value], counts[:m.value]

    def piece_vote_batch_dev(self, idx_ptr, n_groups, per_group, ids_ptr, n_db, n_pieces, top_k, targets=None):
        """piece_vote_dev for n_groups groups of per_group top-k indices in one call (asr_piece_vote_batch_dev) ->
        (pieces (n_groups, top_k) int32, counts (n_groups, top_k) int32, n_out (n_groups,) int32, ranks, ratios);
        row g holds piece_vote_dev's result on group g in its first n_out[g] slots (piece -1 / count 0 after them).
        With targets (one piece id per group): ranks int32 / ratios float64 of the reference's full-eval rule, else
        None."""
        n_groups, top_k = int(n_groups), int(top_k)
        pieces = np.empty((max(n_groups, 0), max(top_k, 0)), np.int32)
        counts = np.empty_like(pieces)
        n_out = np.empty(max(n_groups, 0), np.int32)
        ranks = ratios = t = None
        if targets is not None:
            t = np.ascontiguousarray(targets, dtype=np.int32)
            if t.shape != (n_groups,):
                raise ValueError("piece_vote_batch_dev: %d targets for %d groups" % (t.size, n_groups))
            ranks, ratios = np.empty(n_groups, np.int32), np.empty(n_groups, np.float64)
        ptr = lambda x: None if x is None else x.ctypes.data
        self._check(self.lib.asr_piece_vote_batch_dev(self.ctx, idx_ptr, n_groups, per_group, ids_ptr, n_db, n_pieces,
                                                      top_k, ptr(t), ptr(pieces), ptr(counts), ptr(n_out), ptr(ranks),
                                                      ptr(ratios)))
        return pieces, counts, n_out, ranks, ratios

    def track_gate_dev(self, src_ptr, src_floats, offsets, shapes, width, norm=None, frame0=None):
        """the music gate of the reference's live loop (asr_track_gate_dev) for recordings of `shapes` (bins, frames) at
        float `offsets` of the device buffer -> (m_prob float32, voiced bool, level float32 per recording); the per-frame
        arrays hold the recordings one after the other.  norm: per recording a level that replaces its column-sum
        maximum (NaN: keep the maximum); frame0: per recording the stream position of its column 0."""
        n = len(shapes)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        bins = np.ascontiguousarray([s[0] for s in shapes], dtype=np.int32)
        frames = np.ascontiguousarray([s[1] for s in shapes], dtype=np.int32)
        if off.shape != (n,):
            raise ValueError("track_gate_dev: %d offsets for %d recordings" % (off.size, n))
        nrm = None if norm is None else np.ascontiguousarray(norm, dtype=np.float32)
        f0 = None if frame0 is None else np.ascontiguousarray(frame0, dtype=np.int64)
        for name, x in (("norm", nrm), ("frame0", f0)):
            if x is not None and x.shape != (n,):
                raise ValueError("track_gate_dev: %d %s values for %d recordings" % (x.size, name, n))
        total = int(np.maximum(frames, 0).sum())
        m_prob, voiced, level = np.empty(total, np.float32), np.empty(total, np.uint8), np.empty(n, np.float32)
        ptr = lambda x: None if x is None else x.ctypes.data
        self._check(self.lib.asr_track_gate_dev(self.ctx, src_ptr, src_floats, n, ptr(off), ptr(bins), ptr(frames), ptr(f0),
                                                ptr(nrm), width, ptr(m_prob), ptr(voiced), ptr(level)))
        return m_prob, voiced.astype(bool), level

    def track_vote_batch_dev(self, idx_ptr, n_rows, row_first, row_count, n_candidates, running_frames, ids_ptr, n_db,
                             n_pieces, top_k, emit_from=None):
        """the sliding vote over the (n_rows, n_candidates) top-k table of all voiced frames (asr_track_vote_batch_dev):
        recording r owns rows row_first[r] .. + row_count[r]; per frame from emit_from[r] on (default 0) the vote over
        its last running_frames frames -> (pieces (E, top_k) int32, counts (E, top_k) int32, n_out (E,) int32), E = the
        emitted frames of all recordings one after the other; piece -1 / count 0 past n_out."""
        first = np.ascontiguousarray(row_first, dtype=np.int64)
        count = np.ascontiguousarray(row_count, dtype=np.int64)
        n = first.size
        if first.ndim != 1 or count.shape != (n,):
            raise ValueError("track_vote_batch_dev: %d row ranges, %d row counts" % (n, count.size))
        emit = None if emit_from is None else np.ascontiguousarray(emit_from, dtype=np.int64)
        if emit is not None and emit.shape != (n,):
            raise ValueError("track_vote_batch_dev: %d emit_from values for %d recordings" % (emit.size, n))
        e = int(np.maximum(count - (0 if emit is None else emit), 0).sum())
        k = max(int(top_k), 0)
        pieces, counts, n_out = np.empty((e, k), np.int32), np.empty((e, k), np.int32), np.empty(e, np.int32)
        ptr = lambda x: None if x is None else x.ctypes.data
        self._check(self.lib.asr_track_vote_batch_dev(self.ctx, idx_ptr, n_rows, n, ptr(first), ptr(count), ptr(emit),
                                                      n_candidates, running_frames, ids_ptr, n_db, n_pieces, top_k,
                                                      ptr(pieces), ptr(counts), ptr(n_out)))
        return pieces, counts, n_out

    def track_stream_gate_dev(self, cols_ptr, cols_floats, col_off, n_new, frames_before, level, bins, width, tail_ptr,
                              tail_floats, tail_off, win_ptr, win_cap):
        """the music gate and the windows of the voiced frames for parallel streams whose last width - 1 columns stay on
        the device (asr_track_stream_gate_dev): stream s brings n_new[s] columns as a (bins, n_new[s]) block at float
        col_off[s] of the buffer at cols_ptr and has frames_before[s] frames behind it; its tail at float tail_off[s] of
        the buffer at tail_ptr is updated in place.  -> (m_prob float32, voiced bool, n_voiced int32 per stream); the
        per-frame arrays hold the streams one after the other, and the windows of the voiced frames stand in that order
        at win_ptr (room for win_cap windows)."""
        new = np.ascontiguousarray(n_new, dtype=np.int32)
        n = new.size
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        before = np.ascontiguousarray(frames_before, dtype=np.int64)
        lvl = np.ascontiguousarray(level, dtype=np.float32)
        t_off = np.ascontiguousarray(tail_off, dtype=np.int64)
        if new.ndim != 1 or not (off.shape == before.shape == lvl.shape == t_off.shape == (n,)):
            raise ValueError("track_stream_gate_dev: the per-stream tables differ in length")
        total = int(np.maximum(new, 0).sum())
        m_prob, voiced, n_voiced = np.empty(total, np.float32), np.empty(total, np.uint8), np.zeros(n, np.int32)
        self._check(self.lib.asr_track_stream_gate_dev(
            self.ctx, cols_ptr, int(cols_floats), n, off.ctypes.data, new.ctypes.data, before.ctypes.data, lvl.ctypes.data,
            int(bins), int(width), tail_ptr, int(tail_floats), t_off.ctypes.data, win_ptr, int(win_cap),
            m_prob.ctypes.data, voiced.ctypes.data, n_voiced.ctypes.data))
        return m_prob, voiced.astype(bool), n_voiced

    def track_stream_vote_dev(self, idx_ptr, n_rows, row_count, voiced_before, n_candidates, running_frames, ids_ptr, n_db,
                              n_pieces, top_k, hist_ptr, hist_len, hist_off):
        """the sliding vote for parallel streams whose history stays on the device (asr_track_stream_vote_dev): stream s
        owns row_count[s] consecutive rows of the (n_rows, n_candidates) index table at idx_ptr and has voiced_before[s]
        voiced frames behind it; its ring of running_frames - 1 rows at entry hist_off[s] of the buffer at hist_ptr is
        updated in place.  -> (pieces (n_rows, top_k) int32, counts (n_rows, top_k) int32, n_out (n_rows,) int32)."""
        count = np.ascontiguousarray(row_count, dtype=np.int32)
        n = count.size
        before = np.ascontiguousarray(voiced_before, dtype=np.int64)
        h_off = None if hist_off is None else np.ascontiguousarray(hist_off, dtype=np.int64)
        if count.ndim != 1 or before.shape != (n,) or (h_off is not None and h_off.shape != (n,)):
            raise ValueError("track_stream_vote_dev: the per-stream tables differ in length")
        e, k = max(int(n_rows), 0), max(int(top_k), 0)
        pieces, counts, n_out = np.empty((e, k), np.int32), np.empty((e, k), np.int32), np.empty(e, np.int32)
        self._check(self.lib.asr_track_stream_vote_dev(
            self.ctx, idx_ptr, int(n_rows), n, count.ctypes.data, before.ctypes.data, int(n_candidates),
            int(running_frames), ids_ptr, int(n_db), int(n_pieces), int(top_k), hist_ptr, int(hist_len),
            None if h_off is None else h_off.ctypes.data, pieces.ctypes.data, counts.ctypes.data, n_out.ctypes.data))
        return pieces, counts, n_out

    def track_gate_running_dev(self, src_ptr, src_floats, offsets, shapes, width, memory=0, floor=-np.inf):
        """track_gate_dev at the level of what has been heard so far (asr_track_gate_running_dev): frame i is gated with
        max(floor, the largest column sum of its last `memory` columns up to its own; memory 0: of all so far)
        -> (m_prob float32, voiced bool, level float32), all per frame."""
        n = len(shapes)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        bins = np.ascontiguousarray([s[0] for s in shapes], dtype=np.int32)
        frames = np.ascontiguousarray([s[1] for s in shapes], dtype=np.int32)
        if off.shape != (n,):
            raise ValueError("track_gate_running_dev: %d offsets for %d recordings" % (off.size, n))
        total = int(np.maximum(frames, 0).sum())
        m_prob, voiced, level = np.empty(total, np.float32), np.empty(total, np.uint8), np.empty(total, np.float32)
        self._check(self.lib.asr_track_gate_running_dev(
            self.ctx, src_ptr, int(src_floats), n, off.ctypes.data, bins.ctypes.data, frames.ctypes.data, int(width),
            int(memory), float(floor), m_prob.ctypes.data, voiced.ctypes.data, level.ctypes.data))
        return m_prob, voiced.astype(bool), level

    def track_stream_gate_running_dev(self, cols_ptr, cols_floats, col_off, n_new, frames_before, memory, floor, bins,
                                      width, tail_ptr, tail_floats, tail_off, level_ptr, level_floats, level_off, win_ptr,
                                      win_cap):
        """track_stream_gate_dev at the level of what each stream has brought so far
        (asr_track_stream_gate_running_dev): `memory` and `floor` take the place of the levels, and stream s carries its
        level state - memory - 1 floats, or one with memory 0 - at float level_off[s] of the buffer at level_ptr, updated
        in place.  -> (m_prob float32, voiced bool, n_voiced int32 per stream, level float32 per frame)."""
        new = np.ascontiguousarray(n_new, dtype=np.int32)
        n = new.size
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        before = np.ascontiguousarray(frames_before, dtype=np.int64)
        t_off = np.ascontiguousarray(tail_off, dtype=np.int64)
        l_off = np.ascontiguousarray(level_off, dtype=np.int64)
        if new.ndim != 1 or not (off.shape == before.shape == t_off.shape == l_off.shape == (n,)):
            raise ValueError("track_stream_gate_running_dev: the per-stream tables differ in length")
        total = int(np.maximum(new, 0).sum())
        m_prob, voiced, n_voiced = np.empty(total, np.float32), np.empty(total, np.uint8), np.zeros(n, np.int32)
        level = np.empty(total, np.float32)
        self._check(self.lib.asr_track_stream_gate_running_dev(
            self.ctx, cols_ptr, int(cols_floats), n, off.ctypes.data, new.ctypes.data, before.ctypes.data, int(memory),
            float(floor), int(bins), int(width), tail_ptr, int(tail_floats), t_off.ctypes.data, level_ptr,
            int(level_floats), l_off.ctypes.data, win_ptr, int(win_cap), m_prob.ctypes.data, voiced.ctypes.data,
            n_voiced.ctypes.data, level.ctypes.data))
        return m_prob, voiced.astype(bool), n_voiced, level

    def follow_stream_windows_dev(self, cols_ptr, cols_floats, col_off, n_new, cols_before, bins, width, step, tail_ptr,
                                  tail_floats, tail_off, win_ptr, win_cap):
        """the query windows of score following for parallel streams whose last width - 1 columns stay on the device
        (asr_follow_stream_windows_dev): stream s brings n_new[s] columns as a (bins, n_new[s]) block at float col_off[s]
        of the buffer at cols_ptr and has cols_before[s] columns behind it; the windows that begin at its columns
        k * step and end in this block are written to win_ptr (room for win_cap windows) in stream order, and its tail
        at float tail_off[s] of the buffer at tail_ptr is updated in place.  -> n_win int32 per stream"""
        new = np.ascontiguousarray(n_new, dtype=np.int32)
        n = new.size
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        before = np.ascontiguousarray(cols_before, dtype=np.int64)
        t_off = np.ascontiguousarray(tail_off, dtype=np.int64)
        if new.ndim != 1 or not (off.shape == before.shape == t_off.shape == (n,)):
            raise ValueError("follow_stream_windows_dev: the per-stream tables differ in length")
        n_win = np.zeros(n, np.int32)
        self._check(self.lib.asr_follow_stream_windows_dev(
            self.ctx, cols_ptr, int(cols_floats), n, off.ctypes.data, new.ctypes.data, before.ctypes.data, int(bins),
            int(width), int(step), tail_ptr, int(tail_floats), t_off.ctypes.data, win_ptr, int(win_cap),
            n_win.ctypes.data))
        return n_win

    def follow_stream_log_dev(self, codes_ptr, n_rows, row_count, rows_in_log, keep, dim, log_ptr, log_floats, log_off):
        """the code logs of score following for parallel streams (asr_follow_stream_log_dev): stream s owns row_count[s]
        consecutive rows of the (n_rows, dim) code table at codes_ptr; where it brings rows, the last
        min(rows_in_log[s], keep) rows of its log at float log_off[s] of the buffer at log_ptr move to the log's front
        and the new rows are copied behind them.  -> rows_in_log int32 per stream after the call"""
        count = np.ascontiguousarray(row_count, dtype=np.int32)
        n = count.size
        in_log = np.ascontiguousarray(rows_in_log, dtype=np.int32)
        l_off = np.ascontiguousarray(log_off, dtype=np.int64)
        if count.ndim != 1 or in_log.shape != (n,) or l_off.shape != (n,):
            raise ValueError("follow_stream_log_dev: the per-stream tables differ in length")
        self._check(self.lib.asr_follow_stream_log_dev(
            self.ctx, codes_ptr, int(n_rows), n, count.ctypes.data, in_log.ctypes.data, int(keep), int(dim), log_ptr,
            int(log_floats), l_off.ctypes.data))
        return np.where(count > 0, np.minimum(in_log, int(keep)) + count, in_log).astype(np.int32)

    def dtw(self, a, b, want_dists=True):
        """cosine distance matrix + DTW of two code sequences, rows = a (utils/dtw_by_dist.py:5-34 on
        cdist(a, b, "cosine")) -> (min_dist, dists (n_a,n_b) float64 or None, path_a, path_b)."""
        a, b = _f32c(a), _f32c(b)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
            raise ValueError("dtw expects (n_a,d) and (n_b,d) arrays")
        n_a, n_b, dim = a.shape[0], b.shape[0], a.shape[1]
        da, db = self.alloc(a.nbytes).upload(a), self.alloc(b.nbytes).upload(b)
        dists = np.empty((n_a, n_b), np.float64) if want_dists else None
        pa, pb = np.empty(n_a + n_b, np.int32), np.empty(n_a + n_b, np.int32)
        ln, md = c_int32(), c_double()
        try:
            self._check(self.lib.asr_dtw_dev(self.ctx, da.ptr, n_a, db.ptr, n_b, dim,
                                             dists.ctypes.data if want_dists else None, pa.ctypes.data, pb.ctypes.data,
                                             byref(ln), byref(md)))
        finally:
            da.free()
            db.free()
        return float(md.value), dists, pa[:ln.value].copy(), pb[:ln.value].copy()

    def dtw_batch(self, pairs, want_dists=False, first_of=None, want_path=True):
        """Engine.dtw for a list of (a, b) code-sequence pairs in one library call (asr_dtw_batch_dev) -> one
        (min_dist, dists or None, path_a, path_b) per pair, each bit-identical with dtw(a, b).  first_of "a" / "b"
        (or one such value per pair) appends the first-entry projection of that side: per row of a the column of the
        first path entry in it ("a"), per row of b the row of a of the first path entry at it ("b").  want_path=False
        computes only the distances (min_dist / paths are None)."""
        pairs = [(_f32c(a), _f32c(b)) for a, b in pairs]
        if not pairs:
            return []
        dim = pairs[0][0].shape[1] if pairs[0][0].ndim == 2 else -1
        for a, b in pairs:
            if a.ndim != 2 or b.ndim != 2 or a.shape[1] != dim or b.shape[1] != dim:
                raise ValueError("dtw_batch expects (n_a,d) and (n_b,d) arrays of one d")
        sides = [first_of] * len(pairs) if first_of is None or isinstance(first_of, str) else list(first_of)
        if len(sides) != len(pairs) or any(s not in (None, "a", "b") for s in sides):
            raise ValueError("first_of must be None, 'a', 'b' or one of those per pair")
        n_a = np.array([a.shape[0] for a, _ in pairs], np.int64)
        n_b = np.array([b.shape[0] for _, b in pairs], np.int64)
        cat_a, cat_b = np.concatenate([a for a, _ in pairs]), np.concatenate([b for _, b in pairs])
        cells, paths = n_a * n_b, n_a + n_b
        want_a, want_b = "a" in sides, "b" in sides
        md = np.empty(len(pairs), np.float64) if want_path else None
        ln = np.empty(len(pairs), np.int32) if want_path else None
        pa = np.empty(int(paths.sum()), np.int32) if want_path else None
        pb = np.empty(int(paths.sum()), np.int32) if want_path else None
        dists = np.empty(int(cells.sum()), np.float64) if want_dists else None
        fa = np.empty(int(n_a.sum()), np.int32) if want_a else None
        fb = np.empty(int(n_b.sum()), np.int32) if want_b else None
        ptr = lambda x: None if x is None else x.ctypes.data
        da = self.alloc(max(cat_a.nbytes, 4)).upload(cat_a)
        db = self.alloc(max(cat_b.nbytes, 4)).upload(cat_b)
        try:
            self._check(self.lib.asr_dtw_batch_dev(self.ctx, da.ptr, db.ptr, n_a.ctypes.data, n_b.ctypes.data,
                                                   len(pairs), dim, ptr(md), ptr(ln), ptr(pa), ptr(pb), ptr(dists),
                                                   ptr(fa), ptr(fb)))
        finally:
            da.free()
            db.free()
        out = []
        o_cell = o_path = o_a = o_b = 0
        for p, side in enumerate(sides):
            R, C = int(n_a[p]), int(n_b[p])
            d = dists[o_cell:o_cell + R * C].reshape(R, C) if want_dists else None
            if want_path:
                L = int(ln[p])
                item = (float(md[p]), d, pa[o_path:o_path + L].copy(), pb[o_path:o_path + L].copy())
            else:
                item = (None, d, None, None)
            if first_of is not None:
                item += ((fa[o_a:o_a + R].copy() if side == "a" else fb[o_b:o_b + C].copy()) if side else None,)
            out.append(item)
            o_cell, o_path, o_a, o_b = o_cell + R * C, o_path + R + C, o_a + R, o_b + C
        return out

    def dtw_subseq_batch_dev(self, q_ptr, q_rows, r_ptr, r_rows, q_row, n_q, r_row, n_r, dim, want_pos=True):
        """asr_dtw_subseq_batch_dev on device buffers: q_ptr (q_rows, dim) / r_ptr (r_rows, dim) float32 code rows;
        q_row, n_q, r_row, n_r: per pair the first row and the length in either buffer -> (cost float64 [n], start,
        end, path_len int32 [n], pos: list of int32 [n_q[p]] or None)"""
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
        q_row, n_q, r_row, n_r = map(i64, (q_row, n_q, r_row, n_r))
        n = n_q.size
        if not (q_row.size == r_row.size == n_r.size == n):
            raise ValueError("dtw_subseq_batch_dev: the per-pair tables differ in length")
        cost = np.empty(n, np.float64)
        start, end, ln = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        pos = np.empty(int(np.maximum(n_q, 0).sum()), np.int32) if want_pos else None
        self._check(self.lib.asr_dtw_subseq_batch_dev(self.ctx, q_ptr, int(q_rows), r_ptr, int(r_rows), q_row.ctypes.data,
                                                      n_q.ctypes.data, r_row.ctypes.data, n_r.ctypes.data, n, int(dim),
                                                      cost.ctypes.data, start.ctypes.data, end.ctypes.data, ln.ctypes.data,
                                                      pos.ctypes.data if want_pos else None))
        if want_pos:
            at = np.concatenate([[0], np.cumsum(n_q)])
            pos = [pos[at[p]:at[p + 1]].copy() for p in range(n)]
        return cost, start, end, ln, pos

    def dtw_subseq_batch(self, queries, refs, pairs):
        """Subsequence DTW (free start and end on the reference axis; include/asr_hip.h: asr_dtw_subseq_batch_dev) of
        pairs = [(query index, reference index)] over lists of host (n, d) float32 code arrays, each uploaded once
        -> [(cost, start, end, path_len, pos)] per pair"""
        queries, refs = [_f32c(a) for a in queries], [_f32c(a) for a in refs]
        pairs = [(int(a), int(b)) for a, b in pairs]
        if not pairs:
            return []
        if not queries or not refs or queries[0].ndim != 2:
            raise ValueError("dtw_subseq_batch expects lists of (n,d) arrays")
        dim = queries[0].shape[1]
        if any(a.ndim != 2 or a.shape[1] != dim for a in queries + refs):
            raise ValueError("dtw_subseq_batch expects (n,d) arrays of one d")
        if any(not (0 <= a < len(queries) and 0 <= b < len(refs)) for a, b in pairs):
            raise ValueError("dtw_subseq_batch: a pair names a sequence that is not there")
        nq, nr = np.array([a.shape[0] for a in queries], np.int64), np.array([a.shape[0] for a in refs], np.int64)
        q0, r0 = np.concatenate([[0], np.cumsum(nq)]), np.concatenate([[0], np.cumsum(nr)])
        cat_q, cat_r = np.concatenate(queries), np.concatenate(refs)
        qi, ri = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
        dq = self.alloc(max(cat_q.nbytes, 4)).upload(cat_q)
        dr = self.alloc(max(cat_r.nbytes, 4)).upload(cat_r)
        try:
            cost, start, end, ln, pos = self.dtw_subseq_batch_dev(dq.ptr, cat_q.shape[0], dr.ptr, cat_r.shape[0], q0[qi],
                                                                  nq[qi], r0[ri], nr[ri], dim)
        finally:
            dq.free()
            dr.free()
        return [(float(cost[p]), int(start[p]), int(end[p]), int(ln[p]), pos[p]) for p in range(len(pairs))]

    def dtw_follow_batch_dev(self, q_ptr, q_rows, r_ptr, r_rows, q_row, n_q, r_row, n_r, rows_before, dim, acc_ptr,
                             org_ptr, state_len, state_off, want=True):
        """asr_dtw_follow_batch_dev on device buffers: every pair's state (n_r[p] entries at state_off[p] of the float64
        buffer acc_ptr and the int32 buffer org_ptr, state_len elements each) advances by the n_q[p] query rows at
        q_row[p]; rows_before: the rows the state has consumed (0: fresh) -> per pair (cost float64 [n_q[p]], start,
        pos int32 [n_q[p]]), or None with want=False (the state advances all the same)"""
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
        q_row, n_q, r_row, n_r, rows_before, state_off = map(i64, (q_row, n_q, r_row, n_r, rows_before, state_off))
        n = n_q.size
        if not (q_row.size == r_row.size == n_r.size == rows_before.size == state_off.size == n):
            raise ValueError("dtw_follow_batch_dev: the per-pair tables differ in length")
        tot = int(np.maximum(n_q, 0).sum())
        cost = np.empty(tot, np.float64) if want else None
        start, pos = (np.empty(tot, np.int32), np.empty(tot, np.int32)) if want else (None, None)
        self._check(self.lib.asr_dtw_follow_batch_dev(self.ctx, q_ptr, int(q_rows), r_ptr, int(r_rows), q_row.ctypes.data,
                                                      n_q.ctypes.data, r_row.ctypes.data, n_r.ctypes.data,
                                                      rows_before.ctypes.data, n, int(dim), acc_ptr, org_ptr,
                                                      int(state_len), state_off.ctypes.data,
                                                      cost.ctypes.data if want else None,
                                                      start.ctypes.data if want else None,
                                                      pos.ctypes.data if want else None))
        if not want:
            return None
        at = np.concatenate([[0], np.cumsum(n_q)])
        return [(cost[at[p]:at[p + 1]], start[at[p]:at[p + 1]], pos[at[p]:at[p + 1]]) for p in range(n)]

    def dtw_follow_batch(self, queries, refs, pairs, states=None):
        """Streaming subsequence DTW (include/asr_hip.h: asr_dtw_follow_batch_dev) of pairs = [(query index, reference
        index)] over lists of host (n, d) float32 code arrays, each uploaded once.  states: per pair None (fresh) or
        (acc float64 [S], org int32 [S], rows consumed).  A query longer than 1024 rows runs as consecutive calls.
        -> [(cost, start, pos, (acc, org, rows))] per pair"""
        queries, refs = [_f32c(a) for a in queries], [_f32c(a) for a in refs]
        pairs = [(int(a), int(b)) for a, b in pairs]
        if not pairs:
            return []
        if not queries or not refs or queries[0].ndim != 2:
            raise ValueError("dtw_follow_batch expects lists of (n,d) arrays")
        dim = queries[0].shape[1]
        if any(a.ndim != 2 or a.shape[1] != dim for a in queries + refs):
            raise ValueError("dtw_follow_batch expects (n,d) arrays of one d")
        if any(not (0 <= a < len(queries) and 0 <= b < len(refs)) for a, b in pairs):
            raise ValueError("dtw_follow_batch: a pair names a sequence that is not there")
        states = [None] * len(pairs) if states is None else list(states)
        if len(states) != len(pairs):
            raise ValueError("dtw_follow_batch: one state (or None) per pair")
        nq, nr = np.array([a.shape[0] for a in queries], np.int64), np.array([a.shape[0] for a in refs], np.int64)
        q0, r0 = np.concatenate([[0], np.cumsum(nq)]), np.concatenate([[0], np.cumsum(nr)])
        cat_q, cat_r = np.concatenate(queries), np.concatenate(refs)
        qi, ri = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
        if (nq[qi] < 1).any():
            raise ValueError("dtw_follow_batch: an empty query")
        s_off = np.concatenate([[0], np.cumsum(nr[ri])])
        acc, org = np.full(int(s_off[-1]), np.nan), np.zeros(int(s_off[-1]), np.int32)
        before = np.zeros(len(pairs), np.int64)
        for p, st in enumerate(states):
            if st is not None and int(st[2]) > 0:
                a, o = np.asarray(st[0], np.float64), np.asarray(st[1], np.int32)
                if a.shape != (nr[ri[p]],) or o.shape != a.shape:
                    raise ValueError("dtw_follow_batch: pair %d's state does not have its reference's length" % p)
                acc[s_off[p]:s_off[p + 1]], org[s_off[p]:s_off[p + 1]], before[p] = a, o, int(st[2])
        dq = self.alloc(max(cat_q.nbytes, 4)).upload(cat_q)
        dr = self.alloc(max(cat_r.nbytes, 4)).upload(cat_r)
        da, do = self.alloc(max(acc.nbytes, 8)).upload(acc), self.alloc(max(org.nbytes, 4)).upload(org)
        parts = [[] for _ in pairs]
        try:
            for c0 in range(0, int(nq[qi].max()), 1024):
                live = np.flatnonzero(nq[qi] > c0)
                n_now = np.minimum(nq[qi][live] - c0, 1024)
                res = self.dtw_follow_batch_dev(dq.ptr, cat_q.shape[0], dr.ptr, cat_r.shape[0], q0[qi][live] + c0, n_now,
                                                r0[ri][live], nr[ri][live], before[live] + c0, dim, da.ptr, do.ptr,
                                                acc.size, s_off[:-1][live])
                for p, item in zip(live, res):
                    parts[p].append(item)
            acc, org = da.download(acc.shape, np.float64), do.download(org.shape, np.int32)
        finally:
            for b in (dq, dr, da, do):
                b.free()
        return [(np.concatenate([c for c, _, _ in parts[p]]), np.concatenate([s for _, s, _ in parts[p]]),
                 np.concatenate([e for _, _, e in parts[p]]),
                 (acc[s_off[p]:s_off[p + 1]].copy(), org[s_off[p]:s_off[p + 1]].copy(), int(before[p] + nq[qi[p]])))
                for p in range(len(pairs))]

    def spectrogram_dev(self, samples_ptr, n_samples, frame_size, hop, window, fb_start, fb_len, fb_weights, n_frames,
                        out_ptr, mul=1.0, add=1.0, transposed=True):
        window = np.ascontiguousarray(window, np.float32)
        fb_start = np.ascontiguousarray(fb_start, np.int32)
        fb_len = np.ascontiguousarray(fb_len, np.int32)
        fb_weights = np.ascontiguousarray(fb_weights, np.float32)
        self._check(self.lib.asr_spectrogram_dev(self.ctx, samples_ptr, n_samples, frame_size, hop, window.ctypes.data,
                                                 fb_start.ctypes.data, fb_len.ctypes.data, fb_weights.ctypes.data,
                                                 fb_start.size, mul, add, n_frames, 1 if transposed else 0, out_ptr))

    def _spectrogram_batch(self, fn, samples_ptr, samples_floats, sample_offsets, sample_counts, n_frames, out_offsets,
                           frame_size, hop, window, fb_start, fb_len, fb_weights, out_ptr, out_floats, mul, add, transposed):
        """the argument marshalling asr_spectrogram_batch_dev and asr_spectrogram_fft_batch_dev (fn) share"""
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        sample_offsets, sample_counts, n_frames, out_offsets = map(i64, (sample_offsets, sample_counts, n_frames,
                                                                         out_offsets))
        n = sample_counts.size
        if not (sample_offsets.size == n_frames.size == out_offsets.size == n):
            raise ValueError("spectrogram_batch_dev: the per-recording tables differ in length")
        window = np.ascontiguousarray(window, np.float32)
        fb_start = np.ascontiguousarray(fb_start, np.int32)
        fb_len = np.ascontiguousarray(fb_len, np.int32)
        fb_weights = np.ascontiguousarray(fb_weights, np.float32)
        self._check(fn(
            self.ctx, samples_ptr, int(samples_floats), sample_offsets.ctypes.data, sample_counts.ctypes.data,
            n_frames.ctypes.data, out_offsets.ctypes.data, n, frame_size, hop, window.ctypes.data, fb_start.ctypes.data,
            fb_len.ctypes.data, fb_weights.ctypes.data, fb_start.size, mul, add, 1 if transposed else 0, out_ptr,
            int(out_floats)))

    def spectrogram_batch_dev(self, samples_ptr, samples_floats, sample_offsets, sample_counts, n_frames, out_offsets,
                              frame_size, hop, window, fb_start, fb_len, fb_weights, out_ptr, out_floats, mul=1.0,
                              add=1.0, transposed=True):
        """spectrogram_dev for many recordings of one concatenated sample buffer in one launch
        (asr_spectrogram_batch_dev); per recording bit-identical with spectrogram_dev on it alone"""
        self._spectrogram_batch(self.lib.asr_spectrogram_batch_dev, samples_ptr, samples_floats, sample_offsets,
                                sample_counts, n_frames, out_offsets, frame_size, hop, window, fb_start, fb_len,
                                fb_weights, out_ptr, out_floats, mul, add, transposed)

    def spectrogram_fft_batch_dev(self, samples_ptr, samples_floats, sample_offsets, sample_counts, n_frames, out_offsets,
                                  frame_size, hop, window, fb_start, fb_len, fb_weights, out_ptr, out_floats, mul=1.0,
                                  add=1.0, transposed=True):
        """spectrogram_batch_dev with the magnitudes from a real-input FFT (asr_spectrogram_fft_batch_dev; frame_size
        2048 only): within float32 rounding of the DFT, not bit-identical with spectrogram_batch_dev; per recording
        bit-identical whatever else is in the call, in either layout"""
        self._spectrogram_batch(self.lib.asr_spectrogram_fft_batch_dev, samples_ptr, samples_floats, sample_offsets,
                                sample_counts, n_frames, out_offsets, frame_size, hop, window, fb_start, fb_len,
                                fb_weights, out_ptr, out_floats, mul, add, transposed)

    def resample_batch_dev(self, in_ptr, in_floats, in_offsets, in_counts, out_offsets, out_counts, up, down,
                           taps_phase_major, half, round_int16, out_ptr, out_floats):
        """recordings of one input rate resampled by up / down in one launch (asr_resample_batch_dev): recording i is
        in_counts[i] floats at in_offsets[i] of the buffer at in_ptr, its out_counts[i] outputs go to out_offsets[i]
        of the buffer at out_ptr.  taps_phase_major: float64 (up, taps per phase), audio_frontend.resample_plan's.
        Bit-identical per recording with audio_frontend.resample_host"""
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        in_offsets, in_counts, out_offsets, out_counts = map(i64, (in_offsets, in_counts, out_offsets, out_counts))
        n = in_counts.size
        if not (in_offsets.size == out_offsets.size == out_counts.size == n):
            raise ValueError("resample_batch_dev: the per-recording tables differ in length")
        taps = np.ascontiguousarray(taps_phase_major, dtype=np.float64)
        if taps.ndim != 2 or taps.shape[0] < up:
            raise ValueError("resample_batch_dev: taps of shape %r for %d phases" % (taps.shape, up))
        self._check(self.lib.asr_resample_batch_dev(
            self.ctx, in_ptr, int(in_floats), in_offsets.ctypes.data, in_counts.ctypes.data, out_offsets.ctypes.data,
            out_counts.ctypes.data, n, int(up), int(down), taps.ctypes.data, taps.shape[1], int(half),
            1 if round_int16 else 0, out_ptr, int(out_floats)))

    def _audio_stream_push(self, fn, blocks_ptr, blocks_floats, block_offsets, block_counts, samples_before, final,
                           first_frames, n_new_frames, out_offsets, up, down, taps_phase_major, half, round_int16,
                           state_ptr, state_floats, state_offsets, state_cap, frame_size, hop, window, fb_start,
                           fb_len, fb_weights, out_ptr, out_floats, mul, add, transposed):
        """the argument marshalling asr_audio_stream_push_dev and asr_audio_stream_push_fft_dev (fn) share: stream i
        gets block_counts[i] floats at block_offsets[i] of the buffer at blocks_ptr
        after samples_before[i] earlier ones, its n_new_frames[i] frames from frame first_frames[i] on
        (audio_frontend.audio_stream_plan) go to out_offsets[i] of the buffer at out_ptr, and its carried input samples
        live in state_cap floats at state_offsets[i] of the buffer at state_ptr.  taps_phase_major: float64 (up, taps per
        phase), audio_frontend.resample_plan's, or None with up == down == 1 for the front-end's own rate."""
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        block_offsets, block_counts, samples_before, first_frames, n_new_frames, out_offsets, state_offsets = map(
            i64, (block_offsets, block_counts, samples_before, first_frames, n_new_frames, out_offsets, state_offsets))
        final = np.ascontiguousarray(final, dtype=np.int32)
        n = block_counts.size
        if not (block_offsets.size == samples_before.size == final.size == first_frames.size == n_new_frames.size ==
                out_offsets.size == state_offsets.size == n):
            raise ValueError("audio_stream_push_dev: the per-stream tables differ in length")
        if taps_phase_major is None:
            taps_ptr, taps_per_phase = None, 0
        else:
            taps = np.ascontiguousarray(taps_phase_major, dtype=np.float64)
            if taps.ndim != 2 or taps.shape[0] < up:
                raise ValueError("audio_stream_push_dev: taps of shape %r for %d phases" % (taps.shape, up))
            taps_ptr, taps_per_phase = taps.ctypes.data, taps.shape[1]
        window = np.ascontiguousarray(window, np.float32)
        fb_start = np.ascontiguousarray(fb_start, np.int32)
        fb_len = np.ascontiguousarray(fb_len, np.int32)
        fb_weights = np.ascontiguousarray(fb_weights, np.float32)
        self._check(fn(
            self.ctx, blocks_ptr, int(blocks_floats), block_offsets.ctypes.data, block_counts.ctypes.data,
            samples_before.ctypes.data, final.ctypes.data, first_frames.ctypes.data, n_new_frames.ctypes.data,
            out_offsets.ctypes.data, n, int(up), int(down), taps_ptr, taps_per_phase, int(half), 1 if round_int16 else 0,
            state_ptr, int(state_floats), state_offsets.ctypes.data, int(state_cap), int(frame_size), hop,
            window.ctypes.data, fb_start.ctypes.data, fb_len.ctypes.data, fb_weights.ctypes.data, fb_start.size, mul, add,
            1 if transposed else 0, out_ptr, int(out_floats)))

    def audio_stream_push_dev(self, blocks_ptr, blocks_floats, block_offsets, block_counts, samples_before, final,
                              first_frames, n_new_frames, out_offsets, up, down, taps_phase_major, half, round_int16,
                              state_ptr, state_floats, state_offsets, state_cap, frame_size, hop, window, fb_start,
                              fb_len, fb_weights, out_ptr, out_floats, mul=1.0, add=1.0, transposed=True):
        """one block of new input samples per stream -> the spectrogram frames those samples complete
        (asr_audio_stream_push_dev; the arguments: _audio_stream_push).  Whatever the cut into calls, the concatenated
        frames are bit-identical with resample_batch_dev + spectrogram_batch_dev on the whole recording"""
        self._audio_stream_push(self.lib.asr_audio_stream_push_dev, blocks_ptr, blocks_floats, block_offsets,
                                block_counts, samples_before, final, first_frames, n_new_frames, out_offsets, up, down,
                                taps_phase_major, half, round_int16, state_ptr, state_floats, state_offsets, state_cap,
                                frame_size, hop, window, fb_start, fb_len, fb_weights, out_ptr, out_floats, mul, add,
                                transposed)

    def audio_stream_push_fft_dev(self, blocks_ptr, blocks_floats, block_offsets, block_counts, samples_before, final,
                                  first_frames, n_new_frames, out_offsets, up, down, taps_phase_major, half, round_int16,
                                  state_ptr, state_floats, state_offsets, state_cap, frame_size, hop, window, fb_start,
                                  fb_len, fb_weights, out_ptr, out_floats, mul=1.0, add=1.0, transposed=True):
        """audio_stream_push_dev with the magnitudes from the real-input FFT (asr_audio_stream_push_fft_dev; frame_size
        2048 only; same state, same plan).  Whatever the cut into calls and whatever the other streams, the concatenated
        frames are bit-identical with resample_batch_dev + spectrogram_fft_batch_dev on the whole recording, in either
        layout; not bit-identical with audio_stream_push_dev"""
        self._audio_stream_push(self.lib.asr_audio_stream_push_fft_dev, blocks_ptr, blocks_floats, block_offsets,
                                block_counts, samples_before, final, first_frames, n_new_frames, out_offsets, up, down,
                                taps_phase_major, half, round_int16, state_ptr, state_floats, state_offsets, state_cap,
                                frame_size, hop, window, fb_start, fb_len, fb_weights, out_ptr, out_floats, mul, add,
                                transposed)

    def resize_pages_dev(self, pages_ptr, pages_bytes, page_offsets, heights, widths, out_offsets, out_heights,
                         out_widths, out_ptr, out_bytes):
        """uint8 pages of any sizes resampled to out_heights x out_widths in one launch (asr_resize_pages_dev): page i is
        heights[i] x widths[i] bytes at byte page_offsets[i] of the buffer at pages_ptr, its result goes to byte
        out_offsets[i] of the buffer at out_ptr in the same layout.  Exact integer area resampling: byte for byte
        sheet_utils.omr.resize_page_host per page"""
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        page_offsets, out_offsets = i64(page_offsets), i64(out_offsets)
        heights, widths, out_heights, out_widths = map(i32, (heights, widths, out_heights, out_widths))
        n = heights.size
        if not (page_offsets.size == widths.size == out_offsets.size == out_heights.size == out_widths.size == n):
            raise ValueError("resize_pages_dev: the per-page tables differ in length")
        self._check(self.lib.asr_resize_pages_dev(
            self.ctx, pages_ptr, int(pages_bytes), page_offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data, n,
            out_offsets.ctypes.data, out_heights.ctypes.data, out_widths.ctypes.data, out_ptr, int(out_bytes)))

    def skew_estimate_dev(self, pages_ptr, pages_bytes, page_offsets, heights, widths, max_slope=64, return_scores=False):
        """the slope of the staves of every uint8 page, in 1/1024 pixel per pixel, from the projection profiles of the
        slopes -max_slope .. max_slope in one call (asr_skew_estimate_dev; the pages as resize_pages_dev reads them).
        -> int32 (n,); with return_scores also the int64 (n, 2 * max_slope + 1) scores, slope k in column k + max_slope.
        The integers of sheet_utils.omr.estimate_skew_host / skew_scores_host per page"""
        page_offsets = np.ascontiguousarray(page_offsets, dtype=np.int64)
        heights = np.ascontiguousarray(heights, dtype=np.int32)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        n = heights.size
        if not (page_offsets.size == widths.size == n):
            raise ValueError("skew_estimate_dev: the per-page tables differ in length")
        max_slope = int(max_slope)
        slopes = np.zeros(n, np.int32)
        scores = np.zeros((n, 2 * max(max_slope, 0) + 1), np.int64) if return_scores else None
        self._check(self.lib.asr_skew_estimate_dev(
            self.ctx, pages_ptr, int(pages_bytes), page_offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data, n,
            max_slope, slopes.ctypes.data, scores.ctypes.data if return_scores else None))
        return (slopes, scores) if return_scores else slopes

    def deskew_pages_dev(self, pages_ptr, pages_bytes, page_offsets, heights, widths, slopes, out_ptr, out_bytes, fill=255):
        """every uint8 page sheared by its slope (1/1024 pixel per pixel) in one launch (asr_deskew_pages_dev): the
        result of page i goes to byte page_offsets[i] of the buffer at out_ptr, in the shape of the page.  Byte for byte
        sheet_utils.omr.shear_page_host per page"""
        page_offsets = np.ascontiguousarray(page_offsets, dtype=np.int64)
        heights = np.ascontiguousarray(heights, dtype=np.int32)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        slopes = np.ascontiguousarray(slopes, dtype=np.int32)
        n = heights.size
        if not (page_offsets.size == widths.size == slopes.size == n):
            raise ValueError("deskew_pages_dev: the per-page tables differ in length")
        self._check(self.lib.asr_deskew_pages_dev(
            self.ctx, pages_ptr, int(pages_bytes), page_offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data, n,
            slopes.ctypes.data, int(fill), out_ptr, int(out_bytes)))

    def flatten_pages_dev(self, pages_ptr, pages_bytes, page_offsets, heights, widths, radii, out_ptr, out_bytes, floor=64,
                          background_ptr=None):
        """every uint8 page divided by the grey closing of its paper by a (2 * radii[i] + 1)-square, where that is at
        least `floor`, in two launches (asr_flatten_pages_dev): the result of page i goes to byte page_offsets[i] of the
        buffer at out_ptr, in the shape of the page, and the closing itself to the same place of the buffer at
        background_ptr, if one is given.  Byte for byte sheet_utils.omr.flatten_page_host / page_background_host per page"""
        page_offsets = np.ascontiguousarray(page_offsets, dtype=np.int64)
        heights = np.ascontiguousarray(heights, dtype=np.int32)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        radii = np.ascontiguousarray(radii, dtype=np.int32)
        n = heights.size
        if not (page_offsets.size == widths.size == radii.size == n):
            raise ValueError("flatten_pages_dev: the per-page tables differ in length")
        self._check(self.lib.asr_flatten_pages_dev(
            self.ctx, pages_ptr, int(pages_bytes), page_offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data, n,
            radii.ctypes.data, int(floor), out_ptr, int(out_bytes), background_ptr))

    def crop_estimate_dev(self, pages_ptr, pages_bytes, page_offsets, heights, widths, margins, floor=64, share=512,
                          return_counts=False):
        """the paper's rectangle inside a scanner's black border, for every uint8 page in two launches
        (asr_crop_estimate_dev; the pages as resize_pages_dev reads them; margins: int32 per page).
        -> rects int32 (n, 4): r0 r1 c0 c1, status int32 (n,): 1 where the page is undecided and the rect is the whole
        page; with return_counts also the row counts and the column counts, int32, the pages back to back.  The integers
        of sheet_utils.omr.crop_rect_host / crop_counts_host per page"""
        page_offsets = np.ascontiguousarray(page_offsets, dtype=np.int64)
        heights = np.ascontiguousarray(heights, dtype=np.int32)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        margins = np.ascontiguousarray(margins, dtype=np.int32)
        n = heights.size
        if not (page_offsets.size == widths.size == margins.size == n):
            raise ValueError("crop_estimate_dev: the per-page tables differ in length")
        rects = np.zeros((n, 4), np.int32)
        status = np.zeros(n, np.int32)
        rows = np.zeros(max(int(heights.astype(np.int64).clip(0).sum()), 1), np.int32) if return_counts else None
        cols = np.zeros(max(int(widths.astype(np.int64).clip(0).sum()), 1), np.int32) if return_counts else None
        self._check(self.lib.asr_crop_estimate_dev(
            self.ctx, pages_ptr, int(pages_bytes), page_offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data, n,
            int(floor), int(share), margins.ctypes.data, rects.ctypes.data, status.ctypes.data,
            rows.ctypes.data if return_counts else None, cols.ctypes.data if return_counts else None))
        if return_counts:
            return rects, status, rows[:int(heights.astype(np.int64).sum())], cols[:int(widths.astype(np.int64).sum())]
        return rects, status

    def crop_pages_dev(self, pages_ptr, pages_bytes, page_offsets, heights, widths, rects, out_offsets, out_ptr, out_bytes):
        """rows r0 .. r1 - 1 x columns c0 .. c1 - 1 of every uint8 page (rects: int32 (n, 4)) copied in one launch
        (asr_crop_pages_dev): the rect of page i goes to byte out_offsets[i] of the buffer at out_ptr, its rows back to
        back.  Byte for byte page[r0:r1, c0:c1]"""
        page_offsets = np.ascontiguousarray(page_offsets, dtype=np.int64)
        heights = np.ascontiguousarray(heights, dtype=np.int32)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        rects = np.ascontiguousarray(rects, dtype=np.int32)
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.int64)
        n = heights.size
        if not (page_offsets.size == widths.size == out_offsets.size == n and rects.size == 4 * n):
            raise ValueError("crop_pages_dev: the per-page tables differ in length")
        self._check(self.lib.asr_crop_pages_dev(
            self.ctx, pages_ptr, int(pages_bytes), page_offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data, n,
            rects.ctypes.data, out_offsets.ctypes.data, out_ptr, int(out_bytes)))

    def unroll_systems_dev(self, pages_ptr, pages_bytes, page_offsets, heights, widths, systems, system_height,
                           strip_offsets, strip_widths, strips_ptr, strips_floats):
        """the systems of `systems` ((n, 8) int32: page, r0, r1, c0, c1, pad, piece, dst_col) copied out of the uint8
        pages into the pieces' float32 strips in one launch (asr_unroll_systems_dev)"""
        page_offsets = np.ascontiguousarray(page_offsets, dtype=np.int64)
        heights = np.ascontiguousarray(heights, dtype=np.int32)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        systems = np.ascontiguousarray(systems, dtype=np.int32).reshape(-1, 8)
        strip_offsets = np.ascontiguousarray(strip_offsets, dtype=np.int64)
        strip_widths = np.ascontiguousarray(strip_widths, dtype=np.int32)
        if not (page_offsets.size == heights.size == widths.size) or strip_offsets.size != strip_widths.size:
            raise ValueError("unroll_systems_dev: the per-page / per-piece tables differ in length")
        self._check(self.lib.asr_unroll_systems_dev(
            self.ctx, pages_ptr, int(pages_bytes), page_offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data,
            heights.size, systems.ctypes.data, systems.shape[0], int(system_height), strip_offsets.ctypes.data,
            strip_widths.ctypes.data, strip_widths.size, strips_ptr, int(strips_floats)))

    def score_map_dev(self, maps_ptr, heights, widths, page_in_piece, systems, system_index, n_pieces, threshold=0.5,
                      min_rows=60, tol=10, max_lines=64):
        """the measures of every piece in strip coordinates from the bar network's float64 maps, which lie back to back
        on the device, and the table unroll_systems_dev takes, in three launches (asr_score_map_dev).  page_in_piece:
        (n_pages,) the page's index within its piece; system_index: (n_systems,) the system's index on its page.  ->
        (measures (n, 8) int32 rows of x0, x1, page, system, col0, col1, row0, row1, piece_first (n_pieces + 1,) int32).
        Integer for integer sheet_utils.omr.score_map_host.  ValueError when a system has more than max_lines interior
        bar lines."""
        heights, widths = self._map_tables("score_map_dev", heights, widths)
        page_in_piece = np.ascontiguousarray(page_in_piece, dtype=np.int32)
        systems = np.ascontiguousarray(systems, dtype=np.int32).reshape(-1, 8)
        system_index = np.ascontiguousarray(system_index, dtype=np.int32)
        if page_in_piece.shape != heights.shape or system_index.shape != (systems.shape[0],):
            raise ValueError("score_map_dev: the per-page / per-system tables differ in length")
        n_pieces, max_lines = int(n_pieces), int(max_lines)
        if n_pieces < 0 or max_lines < 0:
            raise ValueError("score_map_dev: n_pieces %d / max_lines %d" % (n_pieces, max_lines))
        measures = np.zeros((systems.shape[0] * (max_lines + 1), 8), np.int32)
        piece_first = np.zeros(n_pieces + 1, np.int32)
        n, over = c_int32(0), c_int32(-1)
        self._check(self.lib.asr_score_map_dev(
            self.ctx, maps_ptr, int((heights.astype(np.int64) * widths).sum()), heights.ctypes.data, widths.ctypes.data,
            heights.size, page_in_piece.ctypes.data, systems.ctypes.data, system_index.ctypes.data, systems.shape[0],
            n_pieces, float(threshold), int(min_rows), int(tol), max_lines, measures.ctypes.data, piece_first.ctypes.data,
            byref(n), byref(over)))
        if over.value >= 0:
            page, _, _, c0, c1 = systems[over.value, :5]
            raise ValueError("score_map_dev: system %d (page %d, columns %d:%d) has more than max_lines = %d interior bar "
                             "lines" % (over.value, page, c0, c1, max_lines))
        return measures[:n.value].copy(), piece_first

    def systems_from_maps_dev(self, pages_ptr, in_mode, page_offsets, heights, widths, system_maps_ptr,
                              bar_maps_ptr=None, max_systems=None, system_seg=None, bar_seg=None):
        """systems_from_maps of sheet_utils/omr.py for all pages in one call, on maps that are on the device
        (asr_systems_from_maps_dev).  Pages as seg_predict reads them; the float64 maps back to back.  ->
        (status (n,), counts (n,), systems (n, max_systems, 4) int32 rows of min_row, max_row, min_col, max_col,
        labelling passes).  status 0 ok, 1 the host's IndexError, 2 its ValueError, 3 not decided on the device."""
        page_offsets = np.ascontiguousarray(page_offsets, dtype=np.int64)
        heights = np.ascontiguousarray(heights, dtype=np.int32)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        if not (page_offsets.ndim == heights.ndim == widths.ndim == 1) or \
                not (page_offsets.size == heights.size == widths.size):
            raise ValueError("systems_from_maps_dev: the per-page tables differ in length")
        n = int(heights.size)
        need = int((heights.astype(np.int64) * widths // SYSTEM_MIN_AREA).max()) if n else 0
        if max_systems is None:
            max_systems = max(need, 1)
        max_systems = int(max_systems)
        if max_systems < need:
            raise ValueError("systems_from_maps_dev: a page can hold %d systems of %d pixels, max_systems is %d"
                             % (need, SYSTEM_MIN_AREA, max_systems))
        status = np.full(n, 3, np.int32)
        counts = np.zeros(n, np.int32)
        systems = np.zeros((n, max_systems, 4), np.int32)
        passes = c_int32(0)
        self._check(self.lib.asr_systems_from_maps_dev(
            self.ctx, pages_ptr, int(in_mode), page_offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data, n,
            system_maps_ptr, bar_maps_ptr, system_seg, bar_seg, max_systems, status.ctypes.data, counts.ctypes.data,
            systems.ctypes.data, byref(passes)))
        return status, counts, systems, int(passes.value)

    @staticmethod
    def _map_tables(who, heights, widths):
        heights = np.ascontiguousarray(heights, dtype=np.int32)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        if not (heights.ndim == widths.ndim == 1) or heights.size != widths.size:
            raise ValueError("%s: the per-page tables differ in length" % who)
        return heights, widths

    def notes_from_map_dev(self, maps_ptr, heights, widths, threshold_abs=0.5, threshold_rel=None, min_distance=3,
                           max_peaks=4096, seg=None):
        """notes_from_map of sheet_utils/omr.py (peak_local_max in two dimensions) for all pages in one call, on
        float64 maps that lie back to back on the device (asr_notes_from_map_dev).  None for a threshold: not given.
        -> (status (n,), counts (n,), coords (n, max_peaks, 2) int32 (row, col) in the host's order).  status 0
        decided, 3 not decided on the device, 4 more than max_peaks peaks (counts holds the true number)."""
        heights, widths = self._map_tables("notes_from_map_dev", heights, widths)
        n, max_peaks = int(heights.size), int(max_peaks)
        status = np.full(n, 3, np.int32)
        counts = np.zeros(n, np.int32)
        coords = np.zeros((n, max(max_peaks, 0), 2), np.int32)
        nan = float("nan")
        self._check(self.lib.asr_notes_from_map_dev(
            self.ctx, maps_ptr, heights.ctypes.data, widths.ctypes.data, n, seg,
            nan if threshold_abs is None else float(threshold_abs), nan if threshold_rel is None else float(threshold_rel),
            int(min_distance), max_peaks, status.ctypes.data, counts.ctypes.data, coords.ctypes.data))
        return status, counts, coords

    def bars_from_map_dev(self, maps_ptr, heights, widths, max_blobs=16384, seg=None):
        """bar_blobs_from_map of sheet_utils/omr.py (Otsu, 8-connected labels, blob_stats) for all pages in one call
        (asr_bars_from_map_dev).  -> (status (n,), counts (n,), blobs (n, max_blobs, 10) int64 in label order,
        labelling passes).  status 0 decided, 3 not decided on the device, 4 more than max_blobs blobs."""
        heights, widths = self._map_tables("bars_from_map_dev", heights, widths)
        n, max_blobs = int(heights.size), int(max_blobs)
        status = np.full(n, 3, np.int32)
        counts = np.zeros(n, np.int32)
        blobs = np.zeros((n, max(max_blobs, 0), 10), np.int64)
        passes = c_int32(0)
        self._check(self.lib.asr_bars_from_map_dev(
            self.ctx, maps_ptr, heights.ctypes.data, widths.ctypes.data, n, seg, max_blobs, status.ctypes.data,
            counts.ctypes.data, blobs.ctypes.data, byref(passes)))
        return status, counts, blobs, int(passes.value)

    def tune_report(self):
        """(comparisons, mismatches, max deviation) of the autotuner's self-check (ASR_TUNE_VERIFY=1)."""
        a, b, d = c_int32(), c_int32(), c_float()
        self._check(self.lib.asr_debug_tune_report(self.ctx, byref(a), byref(b), byref(d)))
        return int(a.value), int(b.value), float(d.value)

    def gather_windows_dev(self, src_ptr, src_floats, desc, out_h, out_w, out_ptr):
        desc = np.ascontiguousarray(desc, dtype=np.float64).reshape(-1, 9)
        self._check(self.lib.asr_gather_windows_dev(self.ctx, src_ptr, src_floats, desc.ctypes.data, desc.shape[0],
                                                    out_h, out_w, out_ptr))

    # -- multi-GPU (one context per GPU) ----------------------------
    def comm_unique_id(self):
        """rank 0: the RCCL unique id (128 bytes) every rank passes to comm_init."""
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        rc = self.lib.asr_comm_unique_id(buf)
        if rc != ASR_OK:
            raise AsrError(rc, (self.lib.asr_last_error(None) or b"").decode())
        return buf.raw

    def comm_init(self, rank, world, unique_id):
        assert len(unique_id) == COMM_ID_BYTES
        self._check(self.lib.asr_comm_init(self.ctx, rank, world, ctypes.c_char_p(unique_id)))

    def comm_init_custom(self, rank, world, allreduce, allgather):
        """allreduce(buf_dev, count, dtype) / allgather(send_dev, recv_dev, bytes_per_rank): host-synchronous
        Python callables returning 0; the library drains its stream before calling them."""
        self._comm_cbs = (ALLREDUCE_FN(lambda user, buf, count, dtype: int(allreduce(buf, count, dtype))),
                          ALLGATHER_FN(lambda user, send, recv, nbytes: int(allgather(send, recv, nbytes))))
        self._check(self.lib.asr_comm_init_custom(self.ctx, rank, world, self._comm_cbs[0], self._comm_cbs[1], None))

    def comm_destroy(self):
        self._check(self.lib.asr_comm_destroy(self.ctx))

    def comm_info(self):
        r, w = c_int(), c_int()
        self._check(self.lib.asr_comm_info(self.ctx, byref(r), byref(w)))
        return int(r.value), int(w.value)

    def comm_stats(self, reset=False):
        """collectives issued since the last reset: dict(allreduce_calls, allreduce_bytes, allgather_calls,
        allgather_bytes_per_rank)"""
        c = (c_int64 * 4)()
        self._check(self.lib.asr_comm_stats(self.ctx, c, 1 if reset else 0))
        return dict(allreduce_calls=int(c[0]), allreduce_bytes=int(c[1]), allgather_calls=int(c[2]),
                    allgather_bytes_per_rank=int(c[3]))

    def comm_timing(self, enable=True):
        """(ms, calls) spent in collectives since the previous call (asr_comm_timing); switches the bracketing on / off"""
        ms, calls = ctypes.c_double(), c_int64()
        self._check(self.lib.asr_comm_timing(self.ctx, 1 if enable else 0, byref(ms), byref(calls)))
        return float(ms.value), int(calls.value)

    def comm_library(self):
        """path of the librccl the communicator's entry points were bound from ('' without an RCCL communicator)"""
        buf = ctypes.create_string_buffer(1024)
        self._check(self.lib.asr_comm_library(self.ctx, buf, 1024))
        return buf.value.decode()

    def comm_allreduce_dev(self, buf_ptr, count, dtype=DTYPE_F64):
        self._check(self.lib.asr_comm_allreduce_dev(self.ctx, buf_ptr, count, dtype))

    def comm_allgather_dev(self, send_ptr, recv_ptr, bytes_per_rank):
        self._check(self.lib.asr_comm_allgather_dev(self.ctx, send_ptr, recv_ptr, bytes_per_rank))

    def allreduce_host(self, values):
        """sum of a small float64 host vector over all ranks of the communicator (staged through the device)"""
        v = np.ascontiguousarray(values, dtype=np.float64)
        buf = self.alloc(max(v.nbytes, 8)).upload(v)
        try:
            self.comm_allreduce_dev(buf.ptr, v.size, DTYPE_F64)
            return buf.download(v.shape, np.float64)
        finally:
            buf.free()

    def allgather_host(self, arr):
        """every rank's (equal-sized) host array, stacked along a new leading axis in rank order"""
        a = np.ascontiguousarray(arr)
        _, world = self.comm_info()
        send = self.alloc(max(a.nbytes, 1)).upload(a)
        recv = self.alloc(max(a.nbytes * world, 1))
        try:
            self.comm_allgather_dev(send.ptr, recv.ptr, a.nbytes)
            return recv.download((world,) + a.shape, a.dtype)
        finally:
            send.free()
            recv.free()

    def topk_merge_dev(self, part_idx_ptr, part_dist_ptr, n_parts, n_q_total, q_lo, n_q, k, idx_ptr, dist_ptr):
        self._check(self.lib.asr_topk_merge_dev(self.ctx, part_idx_ptr, part_dist_ptr, n_parts, n_q_total, q_lo, n_q, k,
                                                idx_ptr, dist_ptr))

    def rank_finish_dev(self, counts_ptr, dstar_ptr, n, ranks_ptr, dstar_out_ptr, ties_ptr):
        self._check(self.lib.asr_rank_finish_dev(self.ctx, counts_ptr, dstar_ptr, n, ranks_ptr, dstar_out_ptr, ties_ptr))

    def rank_sharded_dev(self, lv1_ptr, lv2_ptr, n_local, lv2_all_ptr, ranks_ptr, dstar_ptr, ties_ptr):
        self._check(self.lib.asr_rank_sharded_dev(self.ctx, lv1_ptr, lv2_ptr, n_local, lv2_all_ptr, ranks_ptr,
                                                  dstar_ptr, ties_ptr))

    def raw_download(self, ptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self._check(self.lib.asr_dev_download(self.ctx, out.ctypes.data, ptr, out.nbytes))
        return out

    def raw_upload(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._check(self.lib.asr_dev_upload(self.ctx, ptr, arr.ctypes.data, arr.nbytes))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    # -- host-buffer pipeline (run_eval.py:102-108,174 over a stream of host batches) ---------------
    def host_array(self, shape, dtype):
        """A NumPy array in page-locked host memory (asr_host_alloc); released with the engine or host_free()."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = c_void_p()
        self._check(self.lib.asr_host_alloc(self.ctx, nbytes, byref(p)))
        buf = (ctypes.c_char * max(nbytes, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None and self.ctx:
            self._check(self.lib.asr_host_free(self.ctx, p))

    def eval_batches(self, sheets, specs, prepared=False, want_embeddings=False, out=None):
        """sheets[k] (n,1,H,W) uint8 / float32, specs[k] (n,1,92,42) float32 in host memory -> per batch the integer
        ranks, d*, tie counts (and the embeddings) of its all-pairs ranking; inputs double-buffered against
        compute.  out: optional dict of pre-allocated lists (ranks, dstar, ties[, lv1, lv2])."""
        nb = len(sheets)
        if nb != len(specs):
            raise ValueError("eval_batches: %d sheet batches but %d spectrogram batches" % (nb, len(specs)))
        if nb == 0:
            return dict(ranks=[], dstar=[], ties=[], lv1=[], lv2=[])
        xs, mode = [], None
        for a in sheets:
            a, m = self._view1_mode(a, prepared)
            if mode is not None and m != mode:
                raise ValueError("eval_batches: sheet batches of mixed dtype")
            xs.append(a)
            mode = m
        zs = [_f32c(z) for z in specs]
        n = xs[0].shape[0]
        if any(a.shape != xs[0].shape for a in xs) or any(z.shape != zs[0].shape for z in zs) or zs[0].shape[0] != n:
            raise ValueError("eval_batches: all batches must have the same shape")
        if zs[0].shape[2:] != (self.cfg.h2, self.cfg.w2):
            self.set_input_size(2, zs[0].shape[2], zs[0].shape[3])
        out = out or {}

        def outputs(key, shape, dtype):
            # the C side writes n (or n x 32) values through every pointer: a short, strided or wrong-typed array
            # would be a host heap overflow, so caller-supplied buffers are checked here
            arrs = out.get(key)
            if not arrs:
                return [np.empty(shape, dtype) for _ in range(nb)]
            if len(arrs) != nb:
                raise ValueError("eval_batches: out[%r] holds %d arrays for %d batches" % (key, len(arrs), nb))
            for a in arrs:
                if not isinstance(a, np.ndarray) or a.dtype != np.dtype(dtype) or a.shape != shape or \
                        not a.flags.c_contiguous or not a.flags.writeable:
                    raise ValueError("eval_batches: out[%r] needs writable C-contiguous %s arrays of shape %r"
                                     % (key, np.dtype(dtype).name, shape))
            return list(arrs)
        res = dict(ranks=outputs("ranks", (n,), np.int32), dstar=outputs("dstar", (n,), np.float64),
                   ties=outputs("ties", (n,), np.int32))
        if want_embeddings:
            res["lv1"] = outputs("lv1", (n, 32), np.float32)
            res["lv2"] = outputs("lv2", (n, 32), np.float32)

        def ptrs(arrs):
            return (c_void_p * nb)(*[a.ctypes.data for a in arrs])
        self._check(self.lib.asr_eval_batches(
            self.ctx, ptrs(xs), mode, ptrs(zs), nb, n, ptrs(res["ranks"]), ptrs(res["dstar"]), ptrs(res["ties"]),
            ptrs(res["lv1"]) if want_embeddings else None, ptrs(res["lv2"]) if want_embeddings else None))
        return res

    # -- parameters -------------------------------------------------------
    def param_sizes(self):
        n = self.lib.asr_param_count(self.ctx)
        out = []
        for i in range(n):
            v = c_int64()
            self._check(self.lib.asr_param_size(self.ctx, i, byref(v)))
            out.append(v.value)
        return out

    def set_params(self, params):
        """lasagne.layers.set_all_param_values(layers, params)."""
        arrs = [_f32c(p) for p in params]
        n = len(arrs)
        ptrs = (POINTER(c_float) * n)(*[a.ctypes.data_as(POINTER(c_float)) for a in arrs])
        sizes = (c_int64 * n)(*[a.size for a in arrs])
        self._check(self.lib.asr_set_params(self.ctx, ptrs, sizes, n))
        self._shapes = [a.shape for a in arrs]

    def get_params(self):
        """lasagne.layers.get_all_param_values(layers)."""
        sizes = self.param_sizes()
        shapes = getattr(self, "_shapes", [(s,) for s in sizes])
        arrs = [np.empty(shp, np.float32) for shp in shapes]
        n = len(arrs)
        ptrs = (POINTER(c_float) * n)(*[a.ctypes.data_as(POINTER(c_float)) for a in arrs])
        csz = (c_int64 * n)(*sizes)
        self._check(self.lib.asr_get_params(self.ctx, ptrs, csz, n))
        return arrs

    def set_cca(self, U, V, mean1, mean2):
        U, V, m1, m2 = _f32c(U), _f32c(V), _f32c(mean1), _f32c(mean2)
        assert U.shape == (32, 32) and V.shape == (32, 32) and m1.shape == (32,) and m2.shape == (32,)
        self._check(self.lib.asr_set_cca(self.ctx, U.ctypes.data, V.ctypes.data, m1.ctypes.data, m2.ctypes.data))

    # -- embedding ----------------------------------------------------------
    def set_input_size(self, view, h, w):
        """raw input size of `view`; the network is shape-agnostic (global pooling)."""
        self._check(self.lib.asr_set_input_size(self.ctx, view, h, w))
        if view == 1:
            self.cfg.h1, self.cfg.w1 = h, w
            rsz = MODEL_CONFIGS[self.model_name]["resize_view1"]
            self.net_h1, self.net_w1 = (h // 2, w // 2) if rsz else (h, w)
        else:
            self.cfg.h2, self.cfg.w2 = h, w

    def _view1_mode(self, x, prepared):
        if x.ndim != 4 or x.shape[1] != 1:
            raise ValueError("view-1 input must be (n, 1, H, W), got %r" % (x.shape,))
        rsz = MODEL_CONFIGS[self.model_name]["resize_view1"]
        if prepared:
            x = _f32c(x)
            if x.shape[2:] != (self.net_h1, self.net_w1):
                self.set_input_size(1, x.shape[2] * (2 if rsz else 1), x.shape[3] * (2 if rsz else 1))
            return x, IN_F32_PREPARED
        if x.shape[2:] != (self.cfg.h1, self.cfg.w1):
            self.set_input_size(1, x.shape[2], x.shape[3])
        if x.dtype == np.uint8:
            return np.ascontiguousarray(x), IN_U8_RAW
        return _f32c(x), IN_F32_RAW

    def embed_view1(self, x, prepared=True, features=False):
        """compute_v1_latent (run_eval.py:92-93); prepared=False folds
        model.prepare into the first kernel; features=True returns the
        pre-CCA tower output (refine_cca.py:86-87)."""
        x, mode = self._view1_mode(x, prepared)
        out = np.empty((x.shape[0], 32), np.float32)
        self._check(self.lib.asr_embed_view1(self.ctx, x.ctypes.data, mode, x.shape[0],
                                             OUT_FEATURES if features else OUT_LATENT, out.ctypes.data))
        return out

    def embed_view2(self, z, features=False):
        """compute_v2_latent (run_eval.py:94-95)."""
        z = _f32c(z)
        if z.ndim != 4 or z.shape[1] != 1:
            raise ValueError("view-2 input must be (n, 1, H, W), got %r" % (z.shape,))
        if z.shape[2:] != (self.cfg.h2, self.cfg.w2):
            self.set_input_size(2, z.shape[2], z.shape[3])
        out = np.empty((z.shape[0], 32), np.float32)
        self._check(self.lib.asr_embed_view2(self.ctx, z.ctypes.data, z.shape[0],
                                             OUT_FEATURES if features else OUT_LATENT, out.ctypes.data))
        return out

    def embed_both(self, x, z, prepared=False, features=False):
        """compute_output(X1, X2) -> [v1 latent, v2 latent] (utils/train_dcca_pool.py:158)."""
        x, mode = self._view1_mode(x, prepared)
        z = _f32c(z)
        if x.shape[0] != z.shape[0]:
            raise ValueError("embed_both: %d sheets but %d spectrograms" % (x.shape[0], z.shape[0]))
        if z.shape[2:] != (self.cfg.h2, self.cfg.w2):
            self.set_input_size(2, z.shape[2], z.shape[3])
        n = x.shape[0]
        o1, o2 = np.empty((n, 32), np.float32), np.empty((n, 32), np.float32)
        self._check(self.lib.asr_embed_both(self.ctx, x.ctypes.data, mode, z.ctypes.data, n,
                                            OUT_FEATURES if features else OUT_LATENT, o1.ctypes.data, o2.ctypes.data))
        return o1, o2

    def embed_view1_dev(self, x_ptr, mode, n, out_ptr, features=False):
        self._check(self.lib.asr_embed_view1_dev(self.ctx, x_ptr, mode, n,
                                                 OUT_FEATURES if features else OUT_LATENT, out_ptr))

    def embed_view2_dev(self, z_ptr, n, out_ptr, features=False):
        self._check(self.lib.asr_embed_view2_dev(self.ctx, z_ptr, n,
                                                 OUT_FEATURES if features else OUT_LATENT, out_ptr))

    # -- ranking -----------------------------------------------------------
    def rank(self, lv1, lv2, query_offset=0, n1_global=None):
        """Integer ranks / d* / tie counts of eval_retrieval
        (utils/train_dcca_pool.py:28-82) by counting, float64 distances."""
        lv1, lv2 = _f32c(lv1), _f32c(lv2)
        n1, dim = lv1.shape
        n2 = lv2.shape[0]
        assert lv2.shape[1] == dim
        ranks = np.empty(n1, np.int32)
        dstar = np.empty(n1, np.float64)
        ties = np.empty(n1, np.int32)
        self._check(self.lib.asr_rank(self.ctx, lv1.ctypes.data, n1, dim, lv2.ctypes.data, n2, dim, dim,
                                      query_offset, n1 if n1_global is None else n1_global,
                                      ranks.ctypes.data, dstar.ctypes.data, ties.ctypes.data))
        return ranks, dstar, ties

    def rank_dev(self, lv1_ptr, n1, lv2_ptr, n2, ranks_ptr, dstar_ptr, ties_ptr, dim=32, ld=32,
                 query_offset=0, n1_global=None):
        self._check(self.lib.asr_rank_dev(self.ctx, lv1_ptr, n1, ld, lv2_ptr, n2, ld, dim, query_offset,
                                          n1 if n1_global is None else n1_global, ranks_ptr, dstar_ptr, ties_ptr))

    def topk(self, db_codes, query_codes, k, idx_offset=0):
        """k nearest database codes per query by float64 cosine distance
        (audio_sheet_server.py:530-563) -> (idx (Q,k) int32, dist (Q,k) float64)."""
        db, q = _f32c(db_codes), _f32c(query_codes)
        if db.ndim != 2 or q.ndim != 2 or db.shape[1] != q.shape[1]:
            raise ValueError("topk expects (N,d) and (Q,d) arrays, got %r and %r" % (db.shape, q.shape))
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float64)
        self._check(self.lib.asr_topk(self.ctx, db.ctypes.data, db.shape[0], db.shape[1], q.ctypes.data, q.shape[0],
                                      q.shape[1], q.shape[1], k, idx_offset, idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def topk_dev(self, db_ptr, n_db, q_ptr, n_q, k, idx_ptr, dist_ptr, dim=32, ld=32, idx_offset=0):
        self._check(self.lib.asr_topk_dev(self.ctx, db_ptr, n_db, ld, q_ptr, n_q, ld, dim, k, idx_offset,
                                          idx_ptr, dist_ptr))

    # -- resident code data base (audio_sheet_server.py:496-522, 530-563) ---------------------------------------
    def db_create(self, codes_ptr, n, dim=32, ld=None):
        """CodeDB over caller-owned device rows: norms / reciprocal norms / unit-length copy computed once."""
        return CodeDB(self, codes_ptr, n, dim, dim if ld is None else ld)

    # -- CCA re-estimation ------------------------------------------------------
    def cca_fit(self, H1, H2):
        """CCA('svd').fit (utils/cca.py:25-53,199-211) -> (U, V, m1, m2, coeffs);
        U, V, m1, m2 float32 as written back by refine_cca.py:104-107."""
        H1, H2 = _f32c(H1), _f32c(H2)
        if H1.ndim != 2 or H1.shape[1] != 32 or H2.shape != H1.shape:
            raise ValueError("cca_fit expects two (n, 32) arrays, got %r and %r" % (H1.shape, H2.shape))
        U, V = np.empty((32, 32), np.float32), np.empty((32, 32), np.float32)
        m1, m2 = np.empty(32, np.float32), np.empty(32, np.float32)
        coeffs = np.empty(32, np.float64)
        self._check(self.lib.asr_cca_fit(self.ctx, H1.ctypes.data, H2.ctypes.data, H1.shape[0], U.ctypes.data,
                                         V.ctypes.data, m1.ctypes.data, m2.ctypes.data, coeffs.ctypes.data))
        return U, V, m1, m2, coeffs

    def cca_fit_dev(self, h1_ptr, h2_ptr, n, u_ptr, v_ptr, means_ptr, coeffs_ptr):
        self._check(self.lib.asr_cca_fit_dev(self.ctx, h1_ptr, h2_ptr, n, u_ptr, v_ptr, means_ptr, coeffs_ptr))

    # -- training -------------------------------------------------------------
    def train_begin(self, batch_size):
        """allocate the device training state (Adam moments start at zero)."""
        self._check(self.lib.asr_train_begin(self.ctx, int(batch_size)))

    def train_end(self):
        self._check(self.lib.asr_train_end(self.ctx))

    def train_set_global_batch(self, n_global):
        """data parallel: the next steps carry this rank's distributed.shard_range(n_global, rank, world) rows of one
        batch of n_global rows (0: equal shards of batch * world rows)."""
        self._check(self.lib.asr_train_set_global_batch(self.ctx, int(n_global)))

    def _train_inputs(self, x1, x2, prepared, who, check=True):
        """(x1, in_mode, x2) for the training entry points.  prepared=True: x1 is model.prepare's output (float32 at
        the network size); False: the raw window at the context's raw size (cfg.h1 x cfg.w1), uint8 -> ASR_IN_U8_RAW,
        any other dtype -> float32 ASR_IN_F32_RAW - model.prepare then runs on the device."""
        x2 = _f32c(x2)
        if prepared:
            x1, mode, want = _f32c(x1), IN_F32_PREPARED, (self.net_h1, self.net_w1)
        else:
            x1 = np.ascontiguousarray(x1) if x1.dtype == np.uint8 else _f32c(x1)
            mode, want = (IN_U8_RAW if x1.dtype == np.uint8 else IN_F32_RAW), (self.cfg.h1, self.cfg.w1)
        if check and x1.shape[0] != x2.shape[0]:
            raise ValueError("%s: batch sizes differ" % who)
        if check and x1.shape[2:] != want or x2.shape[2:] != (self.cfg.h2, self.cfg.w2):
            raise ValueError("%s: input sizes %r / %r do not match the context's %s size (%d,%d)/(%d,%d); call "
                             "set_input_size before train_begin" % (who, x1.shape, x2.shape,
                                                                   "network" if prepared else "raw", want[0], want[1],
                                                                   self.cfg.h2, self.cfg.w2))
        return x1, mode, x2

    def train_step(self, x1_prepared, x2, lr, prepared=True):
        """iter_funcs['train'](X1, X2) -> (loss, corr) (utils/train_dcca_pool.py:154).  prepared=False: x1 is the
        pool's raw window (uint8 or float32 0..255) and model.prepare runs on the device (asr_train_step_in)."""
        x1, mode, x2 = self._train_inputs(x1_prepared, x2, prepared, "train_step")
        loss = c_float()
        corr = np.empty(32, np.float32)
        if prepared:
            self._check(self.lib.asr_train_step(self.ctx, x1.ctypes.data, x2.ctypes.data, x1.shape[0], lr,
                                                byref(loss), corr.ctypes.data))
        else:
            self._check(self.lib.asr_train_step_in(self.ctx, x1.ctypes.data, mode, x2.ctypes.data, x1.shape[0], lr,
                                                   byref(loss), corr.ctypes.data))
        return float(loss.value), corr

    def train_step_in_dev(self, x1_ptr, mode, x2_ptr, n, lr):
        """asr_train_step_in_dev on device buffers (e.g. AudioScoreRetrievalPool.get_device: IN_F32_RAW)."""
        loss = c_float()
        corr = np.empty(32, np.float32)
        self._check(self.lib.asr_train_step_in_dev(self.ctx, x1_ptr, mode, x2_ptr, n, lr, byref(loss), corr.ctypes.data))
        return float(loss.value), corr

    def burn_in(self, x1_prepared, x2, prepared=True):
        """iter_funcs['init_cca'](X1, X2) -> [v1 latent, v2 latent] of the train-mode graph
        (utils/train_dcca_pool.py:160-162): updates the BN / CCALayer running values only."""
        x1, mode, x2 = self._train_inputs(x1_prepared, x2, prepared, "burn_in", check=not prepared)
        n = x1.shape[0]
        lv1, lv2 = np.empty((n, 32), np.float32), np.empty((n, 32), np.float32)
        if prepared:
            self._check(self.lib.asr_burn_in(self.ctx, x1.ctypes.data, x2.ctypes.data, n, lv1.ctypes.data,
                                             lv2.ctypes.data))
        else:
            self._check(self.lib.asr_burn_in_in(self.ctx, x1.ctypes.data, mode, x2.ctypes.data, n, lv1.ctypes.data,
                                                lv2.ctypes.data))
        return lv1, lv2

    def compute_gradients(self, x1_prepared, x2, prepared=True):
        """iter_funcs['compute_gradients'](X1, X2) (utils/train_dcca_pool.py:164): the gradients of the train loss
        wrt the trainable parameters as one flat array (order of get_params, other slots zero) and the loss."""
        x1, mode, x2 = self._train_inputs(x1_prepared, x2, prepared, "compute_gradients", check=not prepared)
        n = c_int64()
        self._check(self.lib.asr_opt_state_size(self.ctx, byref(n)))
        g = np.empty(n.value, np.float32)
        loss = c_float()
        if prepared:
            self._check(self.lib.asr_compute_gradients(self.ctx, x1.ctypes.data, x2.ctypes.data, x1.shape[0],
                                                       g.ctypes.data, n.value, byref(loss)))
        else:
            self._check(self.lib.asr_compute_gradients_in(self.ctx, x1.ctypes.data, mode, x2.ctypes.data, x1.shape[0],
                                                          g.ctypes.data, n.value, byref(loss)))
        return g, float(loss.value)

    def set_objective(self, weight=1.0, gamma=0.7, symmetric=False):
        """objectives() = get_contrastive_cos_loss(weight, gamma, symmetric) (models/objectives.py:30-69)"""
        self._check(self.lib.asr_set_objective(self.ctx, float(weight), float(gamma), 1 if symmetric else 0))

    def valid_loss(self, x1_prepared, x2, prepared=True):
        """iter_funcs['valid'](X1, X2) -> loss (utils/train_dcca_pool.py:155)."""
        if prepared:
            x1, x2 = _f32c(x1_prepared), _f32c(x2)
            loss = c_float()
            self._check(self.lib.asr_valid_loss(self.ctx, x1.ctypes.data, x2.ctypes.data, x1.shape[0], byref(loss)))
            return float(loss.value)
        x1, mode = self._view1_mode(x1_prepared, False)
        x2 = _f32c(x2)
        loss = c_float()
        self._check(self.lib.asr_valid_loss_in(self.ctx, x1.ctypes.data, mode, x2.ctypes.data, x1.shape[0],
                                               byref(loss)))
        return float(loss.value)

    def valid_output(self, x1, x2, prepared=True):
        """iter_funcs['valid'] + iter_funcs['compute_output'] on the same batch (utils/train_dcca_pool.py:155,158) ->
        (loss, v1 latent, v2 latent) from one forward of both towers (asr_valid_output_in): the loss of valid_loss and
        the latents of embed_both, bit for bit.  prepared=False: x1 is the raw window, as embed_both takes it."""
        x1, mode = self._view1_mode(x1, prepared)
        x2 = _f32c(x2)
        if x1.shape[0] != x2.shape[0]:
            raise ValueError("valid_output: %d sheets but %d spectrograms" % (x1.shape[0], x2.shape[0]))
        if x2.shape[2:] != (self.cfg.h2, self.cfg.w2):
            self.set_input_size(2, x2.shape[2], x2.shape[3])
        n = x1.shape[0]
        loss = c_float()
        o1, o2 = np.empty((n, 32), np.float32), np.empty((n, 32), np.float32)
        self._check(self.lib.asr_valid_output_in(self.ctx, x1.ctypes.data, mode, x2.ctypes.data, n, byref(loss),
                                                 o1.ctypes.data, o2.ctypes.data))
        return float(loss.value), o1, o2

    def valid_output_dev(self, x1_ptr, mode, x2_ptr, n, loss_ptr, lv1_ptr=None, lv2_ptr=None):
        """asr_valid_output_in_dev: enqueue one batch on device buffers (loss_ptr: one float slot; latent pointers
        (n,32) or None).  Ordered inside the context: a later gather into the same windows or a download waits for it."""
        self._check(self.lib.asr_valid_output_in_dev(self.ctx, x1_ptr, mode, x2_ptr, n, loss_ptr, lv1_ptr, lv2_ptr))

    def get_opt_state(self):
        n = c_int64()
        self._check(self.lib.asr_opt_state_size(self.ctx, byref(n)))
        m, v = np.empty(n.value, np.float32), np.empty(n.value, np.float32)
        t = c_int32()
        self._check(self.lib.asr_get_opt_state(self.ctx, m.ctypes.data, v.ctypes.data, n.value, byref(t)))
        return dict(m=m, v=v, t=int(t.value))

    def set_opt_state(self, state):
        m, v = _f32c(state["m"]), _f32c(state["v"])
        self._check(self.lib.asr_set_opt_state(self.ctx, m.ctypes.data, v.ctypes.data, m.size, int(state["t"])))

    def debug_train_tensor(self, kind, view=0, index=0, batch=0):
        kinds = dict(z=0, x=1, stats=2, H=3, dH=4, lv=5, grad=6, master=7, loss=8, zsel=9, pool_mask=10)
        n = c_int64()
        self._check(self.lib.asr_debug_train_tensor(self.ctx, kinds[kind], view, index, batch, None, 0, byref(n)))
        out = np.empty(n.value, np.float32)
        self._check(self.lib.asr_debug_train_tensor(self.ctx, kinds[kind], view, index, batch, out.ctypes.data,
                                                    n.value, byref(n)))
        return out

    def debug_train_candidate(self, view, block, kind, index, a=None, b=None, batch=None):
        """asr_debug_train_candidate: candidate `index` of the training tuner's list for 3x3 block `block` (1..7) of
        `view`, alone, from NaN-filled outputs.  kind 0: a = x (n,H,W,cin) -> z; 1: a = dz (n,H,W,cout) -> dx; 2: a = x,
        b = dz -> dW (cout,cin,3,3).  An index past the end raises AsrError (ASR_ERR_INVALID, "... has <n> candidates").
        Returns a dict: out, launched, desc, family, variant, tile (TH, TW), work_items, workgroups, shape (H, W, cin,
        cout) and, for kind 0, stats_rows, mu, inv_std.  a = None: nothing runs - the description of the candidate for
        a batch of `batch` samples, without out / launched / statistics."""
        info = np.zeros(12, np.int32)
        desc = ctypes.create_string_buffer(128)
        n = int(batch) if a is None else np.shape(a)[0]
        self._check(self.lib.asr_debug_train_candidate(self.ctx, view, block, kind, index, n, None, None, None, 0, None,
                                                       info.ctypes.data, desc, 128))             # the block's shapes
        h, w, cin, cout = (int(v) for v in info[8:12])
        if a is None:
            return dict(desc=desc.value.decode(), family=("direct", "winog", "wino", "wino4")[int(info[4])],
                        variant=int(info[5]), tile=(int(info[6]), int(info[7])), work_items=int(info[2]),
                        workgroups=int(info[3]), shape=(h, w, cin, cout))
        a = _f32c(a)
        b = _f32c(b) if b is not None else None
        if a.shape != (n, h, w, cout if kind == 1 else cin) or (kind == 2 and (b is None or b.shape != (n, h, w, cout))):
            raise ValueError("debug_train_candidate: kind %d of a %d->%d block on %dx%d maps, got %s%s" %
                             (kind, cin, cout, h, w, a.shape, "" if b is None else " and %s" % (b.shape,)))
        out = np.empty((n, h, w, cout) if kind == 0 else (n, h, w, cin) if kind == 1 else (cout, cin, 3, 3), np.float32)
        stats = np.full(2 * cout, np.nan, np.float32)
        self._check(self.lib.asr_debug_train_candidate(self.ctx, view, block, kind, index, n, a.ctypes.data,
                                                       b.ctypes.data if b is not None else None, out.ctypes.data,
                                                       out.size, stats.ctypes.data, info.ctypes.data, desc, 128))
        res = dict(out=out, launched=bool(info[0]), desc=desc.value.decode(),
                   family=("direct", "winog", "wino", "wino4")[int(info[4])], variant=int(info[5]),
                   tile=(int(info[6]), int(info[7])), work_items=int(info[2]), workgroups=int(info[3]),
                   shape=(h, w, cin, cout))
        if kind == 0:
            res.update(stats_rows=int(info[1]), mu=stats[:cout], inv_std=stats[cout:])
        return res

    def cca_train_debug(self, H1, H2, cca_in, backward=True):
        H1, H2 = _f32c(H1), _f32c(H2)
        cin = np.concatenate([_f32c(a).ravel() for a in cca_in])
        assert cin.size == 5184
        B = H1.shape[0]
        cout = np.empty(5184, np.float32)
        lc = np.empty(33, np.float32)
        lv1, lv2 = np.empty((B, 32), np.float32), np.empty((B, 32), np.float32)
        dH1, dH2 = np.empty((B, 32), np.float32), np.empty((B, 32), np.float32)
        self._check(self.lib.asr_cca_train_debug(self.ctx, H1.ctypes.data, H2.ctypes.data, B, cin.ctypes.data,
                                                 cout.ctypes.data, lc.ctypes.data, lv1.ctypes.data, lv2.ctypes.data,
                                                 dH1.ctypes.data if backward else None,
                                                 dH2.ctypes.data if backward else None))
        new = [cout[0:1024].reshape(32, 32), cout[1024:2048].reshape(32, 32), cout[2048:2080], cout[2080:2112],
               cout[2112:3136].reshape(32, 32), cout[3136:4160].reshape(32, 32), cout[4160:5184].reshape(32, 32)]
        return dict(loss=float(lc[0]), corr=lc[1:], cca=new, lv1=lv1, lv2=lv2, dH1=dH1, dH2=dH2)

    # -- profiling -----------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self.lib.asr_profile_enable(self.ctx, 1 if on else 0))

    def profile_filter(self, symbol=None):
        """only launches of this kernel symbol are timed (None: every kernel)"""
        self._check(self.lib.asr_profile_filter(self.ctx, (symbol or "").encode()))

    def profile_reset(self):
        self._check(self.lib.asr_profile_reset(self.ctx))

    def profile(self):
        """[{name, launches, total_ms, flops, bytes}] per kernel label."""
        out = []
        for i in range(self.lib.asr_profile_count(self.ctx)):
            name = ctypes.create_string_buffer(64)
            launches, ms, fl, by = c_int64(), c_double(), c_double(), c_double()
            self._check(self.lib.asr_profile_get(self.ctx, i, name, 64, byref(launches), byref(ms),
                                                 byref(fl), byref(by)))
            sym = ctypes.create_string_buffer(256)
            self._check(self.lib.asr_profile_symbol(self.ctx, i, sym, 256))
            out.append(dict(name=name.value.decode(), symbol=sym.value.decode(), launches=launches.value,
                            total_ms=ms.value, flops=fl.value, bytes=by.value))
        return out

    # -- debugging ------------------------------------------------------------
    def debug_activation(self, view, block, n):
        h, w, c = c_int(), c_int(), c_int()
        self._check(self.lib.asr_debug_activation(self.ctx, view, block, 0, None, byref(h), byref(w), byref(c)))
        out = np.empty((n, h.value, w.value, c.value), np.float32)
        self._check(self.lib.asr_debug_activation(self.ctx, view, block, n, out.ctypes.data,
                                                  byref(h), byref(w), byref(c)))
        return out
