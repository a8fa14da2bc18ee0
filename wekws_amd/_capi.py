"""ctypes binding of libwekws_hip.so (include/wekws_hip.h).  This is the ONLY compute path of the package:
there is no CPU / PyTorch fallback, and a missing or stale library is a hard error."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_LIB_PATH = os.environ.get("WEKWS_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                      "libwekws_hip.so")  # override: kernel experiments only
ABI_VERSION = 2


class HipLibraryError(RuntimeError):
    pass


class Desc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "backbone", "idim", "hdim", "odim", "num_layers", "num_stack", "stack_size", "kernel_size",
        "preproc_relu", "head", "head_hidden", "activation", "precision", "aux0", "aux1")]


class FbankCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_bins", "sample_rate", "frame_length", "frame_shift", "window")] + \
               [("reserved", C.c_int32 * 3)]


class CtcKwsDesc(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("score_beam", C.c_int32), ("path_beam", C.c_int32), ("num_keywords", C.c_int32),
                ("keyword_tokens", C.c_void_p), ("keyword_offsets", C.c_void_p), ("token_set", C.c_void_p),
                ("token_set_len", C.c_int32), ("min_frames", C.c_int32), ("max_frames", C.c_int32),
                ("interval_frames", C.c_int32), ("downsampling", C.c_int32), ("max_streams", C.c_int32),
                ("prefix_capacity", C.c_int32), ("device", C.c_int32), ("threshold", C.c_double)]


class StreamFrontendCfg(C.Structure):
    _fields_ = [("fbank", FbankCfg)] + [(n, C.c_int32) for n in ("left", "right", "skip", "max_streams", "max_chunk", "device")] + \
               [("reserved", C.c_int32 * 2)]


class ResampleCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("orig_freq", "new_freq", "lowpass_filter_width", "out_dtype")] + [("rolloff", C.c_double)] + \
               [(n, C.c_int32) for n in ("max_streams", "max_chunk", "device")] + [("reserved", C.c_int32 * 3)]


class CtcKwsResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("status", "valid", "state", "keyword", "start", "end")] + [("score", C.c_double)]


class ThresholdKwsSlot(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("seen", "resume", "best_frame")] + [("best", C.c_float)]


# name -> (restype, argtypes); the CPU test-suite checks every symbol of the header is exported
SIGNATURES = {
    "wekws_hip_last_error": (C.c_char_p, []),
    "wekws_hip_abi_version": (C.c_int, []),
    "wekws_hip_blob_elems": (C.c_size_t, [C.POINTER(Desc)]),
    "wekws_hip_create": (C.c_int, [C.POINTER(Desc), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "wekws_hip_destroy": (None, [C.c_void_p]),
    "wekws_hip_cache_dim": (C.c_int, [C.c_void_p]),
    "wekws_hip_cache_len": (C.c_int, [C.c_void_p]),
    "wekws_hip_cache_elems": (C.c_size_t, [C.c_void_p, C.c_int]),
    "wekws_hip_output_elems": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "wekws_hip_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "wekws_hip_effective_precision": (C.c_int, [C.c_void_p]),
    "wekws_hip_weight_spread_log2": (C.c_float, [C.c_void_p]),
    "wekws_hip_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "wekws_hip_reserve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "wekws_hip_release": (C.c_int, [C.c_void_p, C.c_void_p]),
    "wekws_hip_forward_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "wekws_hip_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_void_p]),
    "wekws_hip_stream_cache_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "wekws_hip_stream_cache_destroy": (None, [C.c_void_p]),
    "wekws_hip_stream_cache_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "wekws_hip_stream_cache_read": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_stream_cache_write": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_forward_streams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p]),
    "wekws_hip_fbank_create": (C.c_int, [C.POINTER(FbankCfg), C.c_int, C.POINTER(C.c_void_p)]),
    "wekws_hip_fbank_destroy": (None, [C.c_void_p]),
    "wekws_hip_fbank_num_frames": (C.c_int, [C.c_void_p, C.c_int]),
    "wekws_hip_fbank_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_fbank_compute_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_fbank_compute_dither": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_uint64,
                                                 C.c_int64, C.c_void_p]),
    "wekws_hip_fbank_compute_dither_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_uint64,
                                                     C.c_int64, C.c_void_p]),
    "wekws_hip_dither_noise": (C.c_int, [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_splice_frames": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "wekws_hip_dct_lifter": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "wekws_hip_softmax_topk": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wekws_hip_score_maxpool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wekws_hip_det_false_alarms": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_det_false_alarms_text": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_splice": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "wekws_hip_ctc_kws_create": (C.c_int, [C.POINTER(CtcKwsDesc), C.POINTER(C.c_void_p)]),
    "wekws_hip_ctc_kws_destroy": (None, [C.c_void_p]),
    "wekws_hip_ctc_kws_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "wekws_hip_ctc_kws_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "wekws_hip_ctc_kws_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "wekws_hip_ctc_kws_beam_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "wekws_hip_ctc_kws_read_beam": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_ctc_kws_status": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_void_p]),
    "wekws_hip_ctc_kws_add_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double,
                                            C.POINTER(C.c_int32), C.c_void_p]),
    "wekws_hip_ctc_kws_drop_set": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "wekws_hip_ctc_kws_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "wekws_hip_ctc_kws_stream_set": (C.c_int, [C.c_void_p, C.c_int]),
    "wekws_hip_ctc_kws_search_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "wekws_hip_criterion_max_pooling": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wekws_hip_criterion_ce": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "wekws_hip_ctc_loss_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "wekws_hip_ctc_loss": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wekws_hip_ctc_edit_distance": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "wekws_hip_criterion_max_pooling_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_criterion_ce_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_ctc_loss_grad_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "wekws_hip_ctc_loss_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wekws_hip_stream_frontend_create": (C.c_int, [C.POINTER(StreamFrontendCfg), C.POINTER(C.c_void_p)]),
    "wekws_hip_stream_frontend_create_mfcc": (C.c_int, [C.POINTER(StreamFrontendCfg), C.c_int, C.c_float, C.POINTER(C.c_void_p)]),
    "wekws_hip_stream_frontend_destroy": (None, [C.c_void_p]),
    "wekws_hip_stream_frontend_plan": (C.c_int, [C.POINTER(StreamFrontendCfg), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32)]),
    "wekws_hip_stream_frontend_max_frames": (C.c_int, [C.c_void_p, C.c_int]),
    "wekws_hip_stream_frontend_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_stream_frontend_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "wekws_hip_stream_frontend_counts": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "wekws_hip_resample_create": (C.c_int, [C.POINTER(ResampleCfg), C.POINTER(C.c_void_p)]),
    "wekws_hip_resample_destroy": (None, [C.c_void_p]),
    "wekws_hip_resample_num_samples": (C.c_int64, [C.c_int, C.c_int, C.c_int64]),
    "wekws_hip_resample_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "wekws_hip_resample_compute_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "wekws_hip_resample_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_resample_max_out": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "wekws_hip_resample_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "wekws_hip_resample_counts": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    "wekws_hip_resample_bank_create": (C.c_int, [C.POINTER(ResampleCfg), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "wekws_hip_resample_bank_destroy": (None, [C.c_void_p]),
    "wekws_hip_resample_bank_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_void_p]),
    "wekws_hip_resample_bank_compute_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_int, C.c_void_p]),
    "wekws_hip_resample_bank_set_rate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "wekws_hip_resample_bank_rate_of": (C.c_int, [C.c_void_p, C.c_int]),
    "wekws_hip_resample_bank_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_resample_bank_max_out": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "wekws_hip_resample_bank_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "wekws_hip_resample_bank_counts": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    "wekws_hip_wire_sample_bytes": (C.c_int, [C.c_int]),
    "wekws_hip_wire_decode": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "wekws_hip_resample_bank_create_wire": (C.c_int, [C.POINTER(ResampleCfg), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "wekws_hip_resample_bank_compute_wire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_int, C.c_void_p]),
    "wekws_hip_resample_bank_push_wire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_resample_bank_encoding_of": (C.c_int, [C.c_void_p, C.c_int]),
    "wekws_hip_threshold_kws_create": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "wekws_hip_threshold_kws_destroy": (None, [C.c_void_p]),
    "wekws_hip_threshold_kws_max_hits": (C.c_int, [C.c_void_p, C.c_int]),
    "wekws_hip_threshold_kws_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wekws_hip_threshold_kws_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "wekws_hip_threshold_kws_state": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(ThresholdKwsSlot), C.c_void_p]),
    "wekws_hip_reverb_hop": (C.c_int, []),
    "wekws_hip_reverb_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "wekws_hip_reverb_check": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_reverb_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "wekws_hip_reverb_destroy": (None, [C.c_void_p]),
    "wekws_hip_reverb_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "wekws_hip_reverb_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wekws_hip_noise_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "wekws_hip_noise_destroy": (None, [C.c_void_p]),
    "wekws_hip_noise_check": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_double]),
    "wekws_hip_noise_mix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_double, C.c_void_p, C.c_void_p]),
    "wekws_hip_spec_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p]),
    "wekws_hip_cmvn_stats_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "wekws_hip_cmvn_stats_destroy": (None, [C.c_void_p]),
    "wekws_hip_cmvn_stats_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "wekws_hip_cmvn_stats_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_cmvn_stats_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "wekws_hip_cmvn_stats_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "wekws_hip_optim_plan": (C.c_int, [C.c_int64, C.POINTER(C.c_int64)]),
    "wekws_hip_optim_state_bytes": (C.c_size_t, []),
    "wekws_hip_clip_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_double,
                                           C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wekws_hip_grad_norm": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wekws_hip_fsmn_memory_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wekws_hip_fsmn_memory_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_fsmn_memory_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wekws_hip_depthwise_conv1d_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wekws_hip_depthwise_conv1d_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                     C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_depthwise_conv1d_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wekws_hip_batchnorm_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "wekws_hip_batchnorm_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wekws_hip_batchnorm_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_size_t, C.c_void_p]),
    "wekws_hip_gru_scan_reserve_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "wekws_hip_gru_scan_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "wekws_hip_gru_scan_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wekws_hip_linear_wgrad_plan": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "wekws_hip_linear_wgrad_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "wekws_hip_linear_wgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]),
    "wekws_hip_pointwise_conv1d_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "wekws_hip_pointwise_conv1d_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "wekws_hip_pointwise_conv1d_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                     C.c_void_p]),
    "wekws_hip_pointwise_conv1d_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wekws_hip_dense_conv1d_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "wekws_hip_dense_conv1d_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wekws_hip_dense_conv1d_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, C.c_void_p, C.c_void_p]),
    "wekws_hip_dense_conv1d_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

OPTIONS = {"w16": 0, "mdtc16": 1, "stream": 2, "mm": 3, "head_slices": 4, "g16": 5, "envelope": 6, "gru_pipe": 7}   # enum wekws_hip_option

_lib: Optional[C.CDLL] = None


def lib_path() -> str:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load (once) and type the library.  Raises HipLibraryError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise HipLibraryError(
            f"{_LIB_PATH} is missing: build it with `make -C wekws_amd/csrc` (or __graft_entry__.build()). "
            "wekws_amd has no CPU fallback.")
    try:
        lib = C.CDLL(_LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 not found
        raise HipLibraryError(f"cannot load {_LIB_PATH}: {e}") from e
    # the version first: a stale library then fails with the ABI message, not with a missing-symbol error of a newer entry
    try:
        lib.wekws_hip_abi_version.restype = C.c_int
        lib.wekws_hip_abi_version.argtypes = []
        have = lib.wekws_hip_abi_version()
    except AttributeError as e:
        raise HipLibraryError(f"{_LIB_PATH} does not export wekws_hip_abi_version; rebuild it") from e
    if have != ABI_VERSION:
        raise HipLibraryError(f"ABI version mismatch: library {have}, binding {ABI_VERSION}; rebuild with `make -C wekws_amd/csrc`")
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{_LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().wekws_hip_last_error().decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise HipLibraryError(f"{what} failed (code {rc}): {last_error()}")


def make_desc(fields: dict) -> Desc:
    d = Desc()
    for n, _ in Desc._fields_:
        setattr(d, n, int(fields.get(n, 0)))
    return d
