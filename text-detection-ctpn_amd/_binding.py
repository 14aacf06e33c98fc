"""ctypes binding of libctpn_hip.so (C ABI declared in include/ctpn_hip.h).

`cffi` is what BASELINE.json names but it is not installed in this image (and there is no network), so the
binding uses `ctypes`; the declarations below are a 1:1 transcription of the header and
tests/test_abi.py checks that every symbol the header declares is exported.
"""
import collections
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

CTPN_OK = 0
CTPN_ERR_UNSUPPORTED = -6
CTPN_ERR_CAPACITY = -4
PREC_FP32, PREC_BF16, PREC_FP16, PREC_SPLIT = 0, 1, 2, 3
PRECISIONS = {"fp32": PREC_FP32, "f32": PREC_FP32, "bf16": PREC_BF16, "fp16": PREC_FP16, "f16": PREC_FP16, "split": PREC_SPLIT}


def precision_code(p):
    if isinstance(p, int) and p in (PREC_FP32, PREC_BF16, PREC_FP16, PREC_SPLIT):
        return p
    try:
        return PRECISIONS[p]
    except KeyError:
        raise ValueError("unknown precision %r (fp32 | bf16 | fp16 | split)" % (p,))


# Per-ctx options of the C ABI (ctpn_set_option). The library itself reads none of them from the environment; for command-line use the
# BINDING maps these variables onto the option of every Context it creates (explicit options= win):
OPTION_ENV = {"keep_acts": "CTPN_KEEP_ACTS", "conv1_kernel": "CTPN_CONV1_MFMA", "conv1_fuse": "CTPN_CONV1_FUSE", "lstm_split": "CTPN_LSTM_SPLIT", "nms_columns": "CTPN_NMS_COLUMNS",
              "nms_check": "CTPN_NMS_CHECK", "connect_device": "CTPN_CONNECT_DEVICE", "tail_overlap": "CTPN_TAIL_OVERLAP", "conv_p64": "CTPN_CONV_P64",
              "tail_confine": "CTPN_TAIL_CONFINE", "nms_prefix": "CTPN_NMS_PREFIX", "debug_hog": "CTPN_DEBUG_HOG", "debug_nms": "CTPN_DEBUG_NMS", "split_edge": "CTPN_SPLIT_EDGE"}
MODE_H, MODE_O = 0, 1
KIND_NAMES = ["conv_first", "conv_gemm", "pool", "gemm", "bilstm", "decode", "sort", "nms"]


class CtpnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libctpn_hip error %d: %s" % (code, msg))
        self.code = code


def lib_path():
    # CTPN_LIB_PATH: an alternative build of the same library (kernel A/B experiments); the default is the in-tree build
    return os.environ.get("CTPN_LIB_PATH") or os.path.join(_HERE, "libctpn_hip.so")


def _declare(lib):
    u8p, f32p, f64p, i32p = (C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int))
    vp = C.c_void_p
    sig = {
        "ctpn_abi_version": (C.c_int, []),
        "ctpn_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
        "ctpn_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
        "ctpn_option_count": (C.c_int, []),
        "ctpn_option_name": (C.c_char_p, [C.c_int]),
        "ctpn_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
        "ctpn_get_param": (C.c_int, [C.c_void_p, C.c_char_p, f64p]),
        "ctpn_param_count": (C.c_int, []),
        "ctpn_param_name": (C.c_char_p, [C.c_int]),
        "ctpn_param_default": (C.c_int, [C.c_char_p, f64p]),
        "ctpn_reserve_proposals": (C.c_int, [vp, C.c_int]),
        "ctpn_proposal_capacity": (C.c_int, [vp, i32p]),
        "ctpn_debug_text_line_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, i32p]),
        "ctpn_last_error": (C.c_char_p, []),
        "ctpn_device_count": (C.c_int, []),
        "ctpn_create": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "ctpn_create_postproc": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int]),
        "ctpn_host_thread_budget": (C.c_int, [C.c_int, C.c_int, C.c_int]),
        "ctpn_host_threads": (C.c_int, [vp, i32p]),
        "ctpn_proposal_anchors": (C.c_int, [vp, i32p, C.c_int]),
        "ctpn_debug_connect": (C.c_int, [C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, f64p, C.c_int, i32p]),
        "ctpn_debug_text_lines": (C.c_int, [vp, f32p, i32p, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f64p, C.c_int, i32p, i32p, i32p]),
        "ctpn_destroy": (C.c_int, [vp]),
        "ctpn_sync": (C.c_int, [vp]),
        "ctpn_stream": (C.c_int, [vp, C.POINTER(vp)]),
        "ctpn_weight_manifest": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), i32p, i32p, C.POINTER(C.c_size_t)]),
        "ctpn_weight_count": (C.c_int, []),
        "ctpn_load_weights_host": (C.c_int, [vp, f32p]),
        "ctpn_load_weights_device": (C.c_int, [vp, vp]),
        "ctpn_broadcast_weights": (C.c_int, [C.POINTER(vp), C.c_int]),
        "ctpn_comm_unique_id": (C.c_int, [C.c_char_p, C.c_size_t]),
        "ctpn_broadcast_weights_rank": (C.c_int, [vp, C.c_char_p, C.c_int, C.c_int, C.c_int]),
        "ctpn_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "ctpn_forward_blob": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "ctpn_ragged_valid_rows": (C.c_int, [C.c_int, C.c_int]),
        "ctpn_forward_ragged": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p]),
        "ctpn_detect_ragged": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p, f32p, C.c_int, f64p, C.c_int, i32p, f32p, i32p]),
        "ctpn_detect_submit_ragged": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p, f32p, C.c_int]),
        "ctpn_feat_shape": (C.c_int, [vp, i32p, i32p, i32p]),
        "ctpn_get_tensor": (C.c_int, [vp, C.c_char_p, f32p, C.c_size_t, i32p]),
        "ctpn_proposals": (C.c_int, [vp, f32p, C.c_int, C.c_int, C.c_float, C.c_float, f32p, i32p]),
        "ctpn_proposals_from_host": (C.c_int, [vp, f32p, f32p, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_int,
                                               C.c_float, C.c_float, f32p, i32p]),
        "ctpn_nms": (C.c_int, [i32p, i32p, f32p, C.c_int, C.c_int, C.c_float, C.c_int]),
        "ctpn_resize_dims": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, i32p, i32p]),
        "ctpn_resize": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, vp, C.c_int,
                                  C.c_longlong, i32p, i32p]),
        "ctpn_result_text": (C.c_int, [f64p, C.c_int, C.c_double, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), i32p]),
        "ctpn_write_result_file": (C.c_int, [C.c_char_p, f64p, C.c_int, C.c_double, i32p]),
        "ctpn_draw_boxes": (C.c_int, [u8p, C.c_int, C.c_int, f64p, C.c_int]),
        "ctpn_text_lines": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f64p, C.c_int, i32p]),
        "ctpn_text_lines_cfg": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f64p, f64p, C.c_int, i32p]),
        "ctpn_connector_constants": (C.c_int, [f64p]),
        "ctpn_page_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.c_int, i32p, i32p]),
        "ctpn_page_cut": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_longlong, i32p, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_longlong]),
        "ctpn_page_merge": (C.c_int, [i32p, C.c_int, f32p, C.c_int, i32p, C.c_int, C.c_int, C.c_float, f32p, f32p, i32p, C.c_int, i32p]),
        "ctpn_page_nms": (C.c_int, [i32p, i32p, f32p, C.c_int, C.c_int, C.c_float, C.c_int]),
        "ctpn_page_text_lines": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f64p, C.c_int, f64p, C.c_int, i32p]),
        "ctpn_target_config_default": (C.c_int, [f64p]),
        "ctpn_bbox_overlaps": (C.c_int, [C.c_int, f64p, C.c_int, f64p, C.c_int, f64p, C.c_int]),
        "ctpn_anchor_targets": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, f32p, vp, i32p, vp, vp, i32p, f64p, C.c_ulonglong, C.c_int, vp, vp, vp, vp, i32p,
                                          vp, vp, vp]),
        "ctpn_rpn_loss": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, f64p, i32p, vp]),
        "ctpn_tail_saved_floats": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
        "ctpn_tail_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]),
        "ctpn_tail_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp]),
        "ctpn_debug_tail_bptt": (C.c_int, [C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, f32p]),
        "ctpn_conv3x3_backward": (C.c_int, [C.c_int] * 6 + [vp, vp, vp, vp, C.c_int, vp, vp, vp]),
        "ctpn_maxpool2x2_backward": (C.c_int, [C.c_int] * 5 + [vp, vp, C.c_int, vp]),
        "ctpn_conv3x3_backward_plan": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
        "ctpn_solver_plan": (C.c_int, [C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
        "ctpn_solver_defaults": (C.c_int, [C.c_int, f64p]),
        "ctpn_solver_step": (C.c_int, [C.c_int, C.c_int, C.c_longlong, vp, vp, vp, vp, C.POINTER(C.c_longlong), f32p, C.c_int, f64p, C.c_longlong,
                                       C.c_int, f64p]),
        "ctpn_detect": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f64p, C.c_int, i32p,
                                  f32p, i32p]),
        "ctpn_detect_submit": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int]),
        "ctpn_detect_collect": (C.c_int, [vp, C.c_int, C.c_int, f64p, C.c_int, i32p, f32p, i32p]),
        "ctpn_debug_cvt_bf16": (C.c_int, [C.c_int, f32p, C.POINTER(C.c_uint16), C.c_int, C.c_int]),
        "ctpn_debug_lds_dma": (C.c_int, [C.c_int, u8p, C.c_size_t, u8p, u8p]),
        "ctpn_debug_conv3x3": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, f32p, f32p]),
        "ctpn_debug_conv3x3_plan": (C.c_int, [C.c_int] * 13 + [i32p]),
        "ctpn_debug_conv3x3_form_name": (C.c_char_p, [C.c_int, C.c_int]),
        "ctpn_debug_conv3x3_walk_plan": (C.c_int, [C.c_int] * 13 + [i32p]),
        "ctpn_debug_conv3x3_walk": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, f32p, f32p]),
        "ctpn_debug_lstm_pre_plan": (C.c_int, [C.c_longlong, C.c_int, i32p]),
        "ctpn_debug_forward_sets": (C.c_int, [vp, C.POINTER(C.c_longlong)]),
        "ctpn_debug_live_resources": (C.c_int, [C.POINTER(C.c_longlong)]),
        "ctpn_debug_lstm_pre": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
        "ctpn_debug_bilstm": (C.c_int, [C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, i32p]),
        "ctpn_debug_gemm": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
        "ctpn_debug_proposal_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                               f32p, i32p]),
        "ctpn_debug_proposal_fetch": (C.c_int, [vp, C.c_int, C.c_void_p, C.c_size_t]),
        "ctpn_debug_sort_keys": (C.c_int, [C.c_int, C.POINTER(C.c_ulonglong), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]),
        "ctpn_debug_proposals_from_heads": (C.c_int, [vp, f32p, C.c_int, C.c_int, C.c_int, f32p, i32p, C.c_int, C.c_int, C.c_float, C.c_float, f32p, i32p,
                                                      f32p, f32p]),
        "ctpn_debug_conv1": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p,
                                       C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]),
        "ctpn_debug_conv1_fused": (C.c_int, [C.c_int, u8p, C.c_int, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.POINTER(C.c_uint16)]),
        "ctpn_debug_conv1_fused_walk": (C.c_int, [C.c_int, u8p, C.c_int, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p,
                                                  C.POINTER(C.c_uint16)]),
        "ctpn_jpeg_probe": (C.c_int, [u8p, C.c_size_t, i32p, i32p, i32p, i32p]),
        "ctpn_jpeg_coef_capacity": (C.c_size_t, [C.c_int, C.c_int]),
        "ctpn_jpeg_entropy_decode": (C.c_int, [u8p, C.c_size_t, C.POINTER(C.c_int16), C.c_size_t, C.POINTER(C.c_uint16), i32p]),
        "ctpn_decode_jpeg_batch": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                             C.POINTER(vp), i32p, i32p]),
        "ctpn_jpeg_batch_fetch": (C.c_int, [vp, vp, u8p, C.c_size_t]),
        "ctpn_decode_jpeg_files": (C.c_int, [vp, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(vp), i32p, i32p]),
        "ctpn_jpeg_probe_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, i32p, C.c_int]),
        "ctpn_decode_jpeg_batch_device": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                    C.POINTER(vp), i32p, i32p]),
        "ctpn_decode_jpeg_files_device": (C.c_int, [vp, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(vp), i32p, i32p]),
        "ctpn_jpeg_entropy_decode_device": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_int16), C.c_size_t,
                                                      C.POINTER(C.c_uint16), i32p, i32p]),
        "ctpn_jpeg_entropy_device_stats": (C.c_int, [vp, C.POINTER(C.c_longlong)]),
        "ctpn_decode_jpeg_batch_ragged": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(C.c_size_t), C.c_int, i32p, i32p, f64p, C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(vp), i32p]),
        "ctpn_decode_jpeg_files_ragged": (C.c_int, [vp, C.POINTER(C.c_char_p), C.c_int, i32p, i32p, f64p, C.c_int, C.c_int, C.c_int, C.POINTER(vp), i32p]),
        "ctpn_pack_canvas": (C.c_int, [vp, C.POINTER(vp), i32p, i32p, C.POINTER(C.c_longlong), C.c_int, C.c_int, f64p, C.c_int, C.c_int, C.POINTER(vp), i32p]),
        "ctpn_decode_png_files_ragged": (C.c_int, [vp, C.POINTER(C.c_char_p), C.c_int, i32p, i32p, f64p, C.c_int, C.c_int, C.POINTER(vp), i32p]),
        "ctpn_jpeg_encode_capacity": (C.c_size_t, [C.c_int, C.c_int]),
        "ctpn_jpeg_entropy_encode": (C.c_int, [C.POINTER(C.c_int16), i32p, C.POINTER(C.c_uint16), u8p, C.c_size_t, C.POINTER(C.c_size_t)]),
        "ctpn_encode_jpeg_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t),
                                             C.POINTER(C.c_size_t)]),
        "ctpn_write_annotated_files": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, f64p, C.c_int, i32p, C.c_double, C.POINTER(C.c_char_p), C.c_int]),
        "ctpn_encode_jpeg_batch_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t),
                                                    C.POINTER(C.c_size_t)]),
        "ctpn_write_annotated_files_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, f64p, C.c_int, i32p, C.c_double, C.POINTER(C.c_char_p), C.c_int]),
        "ctpn_jpeg_entropy_encode_device": (C.c_int, [vp, C.POINTER(C.POINTER(C.c_int16)), i32p, C.POINTER(C.c_uint16), C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t),
                                                      C.POINTER(C.c_size_t), i32p]),
        "ctpn_jpeg_entropy_encode_device_stats": (C.c_int, [vp, C.POINTER(C.c_longlong)]),
        "ctpn_line_crop_width": (C.c_int, [f64p, C.c_int, C.c_int, i32p]),
        "ctpn_crop_lines": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f64p, C.c_int, i32p, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_size_t,
                                      i32p, i32p]),
        "ctpn_encode_jpeg_mixed": (C.c_int, [vp, vp, C.c_int, C.c_size_t, C.c_int, i32p, i32p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_int,
                                             C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "ctpn_encode_jpeg_mixed_device": (C.c_int, [vp, vp, C.c_int, C.c_size_t, C.c_int, i32p, i32p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_int,
                                                    C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "ctpn_write_line_crops": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f64p, C.c_int, i32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(C.c_char_p), i32p, i32p]),
        "ctpn_write_line_crops_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f64p, C.c_int, i32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.POINTER(C.c_char_p), i32p, i32p]),
        "ctpn_write_annotated_files_ragged": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p, f64p, C.c_int, i32p, f64p, C.POINTER(C.c_char_p),
                                                        C.c_int]),
        "ctpn_write_annotated_files_ragged_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p, f64p, C.c_int, i32p, f64p,
                                                               C.POINTER(C.c_char_p), C.c_int]),
        "ctpn_crop_lines_ragged": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p, f64p, C.c_int, i32p, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                             C.c_size_t, i32p, i32p]),
        "ctpn_write_line_crops_ragged": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p, f64p, C.c_int, i32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.POINTER(C.c_char_p), i32p, i32p]),
        "ctpn_write_line_crops_ragged_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p, f64p, C.c_int, i32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                          C.POINTER(C.c_char_p), i32p, i32p]),
        "ctpn_debug_png_backend": (C.c_int, [C.c_int]),
        "ctpn_png_probe": (C.c_int, [u8p, C.c_size_t, i32p, i32p, i32p, i32p]),
        "ctpn_png_decode": (C.c_int, [u8p, C.c_size_t, u8p, C.c_size_t]),
        "ctpn_png_encode_capacity": (C.c_size_t, [C.c_int, C.c_int]),
        "ctpn_png_encode": (C.c_int, [u8p, C.c_int, C.c_int, u8p, C.c_size_t, C.POINTER(C.c_size_t)]),
        "ctpn_encode_png_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "ctpn_write_annotated_png_files": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f64p, C.c_int, i32p, C.c_double, C.POINTER(C.c_char_p)]),
        "ctpn_png_encode_device_stats": (C.c_int, [vp, C.POINTER(C.c_longlong)]),
        "ctpn_encode_png_mixed": (C.c_int, [vp, vp, C.c_int, C.c_size_t, C.c_int, i32p, i32p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(vp),
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "ctpn_write_annotated_png_files_ragged": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p, f64p, C.c_int, i32p, f64p, C.POINTER(C.c_char_p)]),
        "ctpn_write_line_crops_png": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f64p, C.c_int, i32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p),
                                                i32p, i32p]),
        "ctpn_write_line_crops_png_ragged": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i32p, f64p, C.c_int, i32p, C.c_int, C.c_int, C.c_int,
                                                       C.POINTER(C.c_char_p), i32p, i32p]),
        "ctpn_png_probe_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, i32p, C.c_int]),
        "ctpn_decode_png_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, u8p, C.c_int]),
        "ctpn_profile_enable": (C.c_int, [vp, C.c_int]),
        "ctpn_profile_reset": (C.c_int, [vp]),
        "ctpn_profile_read": (C.c_int, [vp, C.c_int, f64p, C.POINTER(C.c_longlong), f64p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return sig


def _declare_train(lib):
    """include/ctpn_hip_train.h: the training-side calls that take a ctx"""
    sig = {"ctpn_get_tensor_device": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)])}
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return sig


def _declare_data_layer(lib):
    """include/ctpn_hip_data_layer.h (which ctpn_hip_train.h includes): the training data layer's three stateless calls"""
    i32p = C.POINTER(C.c_int)
    sig = {"ctpn_split_labels": (C.c_int, [C.c_int, C.c_int, i32p, C.c_void_p, i32p, C.c_int, C.c_void_p, C.c_longlong, i32p, C.c_void_p]),
           "ctpn_train_page": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int]),
           "ctpn_train_boxes": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p])}
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return sig


def load_library():
    """Load libctpn_hip.so once. Raises CtpnError if it has not been built (no silent fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise CtpnError(-5, "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    # torch bundles its own libamdhip64 (soname libamdhip64.so.7). If torch is (going to be) in this process,
    # it must be loaded first so that both share ONE HIP runtime; see DESIGN.md "HIP runtime sharing".
    if "torch" not in sys.modules and os.environ.get("CTPN_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    _LIB = C.CDLL(path, mode=C.RTLD_GLOBAL)
    _declare(_LIB)
    _declare_train(_LIB)
    _declare_data_layer(_LIB)
    return _LIB


def _check(rc):
    if rc != CTPN_OK:
        raise CtpnError(rc, load_library().ctpn_last_error().decode("utf-8", "replace"))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


def device_count():
    return load_library().ctpn_device_count()


def option_names():
    lib = load_library()
    return [lib.ctpn_option_name(i).decode() for i in range(lib.ctpn_option_count())]


def param_names():
    """Names of a ctx's detection-tail parameters (ctpn_param_name), in ABI order."""
    lib = load_library()
    return [lib.ctpn_param_name(i).decode() for i in range(lib.ctpn_param_count())]


def param_default(name):
    v = C.c_double(0.0)
    _check(load_library().ctpn_param_default(name.encode(), C.byref(v)))
    return v.value


def manifest_from_library():
    lib = load_library()
    out = []
    for i in range(lib.ctpn_weight_count()):
        name = C.c_char_p()
        rank = C.c_int()
        shape = (C.c_int * 4)()
        off = C.c_size_t()
        _check(lib.ctpn_weight_manifest(i, C.byref(name), C.byref(rank), shape, C.byref(off)))
        out.append((name.value.decode(), tuple(shape[: rank.value]), off.value))
    return out


def nms_sorted(boxes_sorted, thresh, device_id=0):
    """B1 seam: same contract as the reference `_nms` (lib/utils/gpu_nms.hpp:1-2) on score-sorted rows."""
    lib = load_library()
    b = _f32(boxes_sorted)
    n = int(b.shape[0])
    if n == 0:
        return np.zeros((0,), np.int32)
    keep = np.zeros((n,), np.int32)
    num = C.c_int(0)
    _check(lib.ctpn_nms(_ptr(keep, C.c_int), C.byref(num), _ptr(b, C.c_float), n, int(b.shape[1]), float(thresh),
                        int(device_id)))
    return keep[: num.value]


def resize_dims(h, w, fx, fy):
    """Output size of cv2.resize(fx, fy): round-half-even(src * f). Host arithmetic of the library, needs no GPU."""
    lib = load_library()
    oh, ow = C.c_int(0), C.c_int(0)
    _check(lib.ctpn_resize_dims(int(h), int(w), float(fx), float(fy), C.byref(oh), C.byref(ow)))
    return oh.value, ow.value


def resize_linear(im, fx, fy, device_id=0):
    """cv2.resize(im, None, None, fx=fx, fy=fy, interpolation=cv2.INTER_LINEAR) on the GPU (ctpn_resize): im is (h,w,3) or
    (n,h,w,3), uint8 or float32; returns the same rank and dtype."""
    lib = load_library()
    a = np.ascontiguousarray(im)
    if a.dtype not in (np.uint8, np.float32):
        a = a.astype(np.float32)
    single = a.ndim == 3
    if single:
        a = a[None]
    if a.ndim != 4 or a.shape[3] != 3:
        raise ValueError("resize_linear wants (h,w,3) or (n,h,w,3)")
    n, h, w, _ = a.shape
    oh, ow = C.c_int(0), C.c_int(0)
    _check(lib.ctpn_resize_dims(h, w, float(fx), float(fy), C.byref(oh), C.byref(ow)))
    out = np.empty((n, oh.value, ow.value, 3), a.dtype)
    _check(lib.ctpn_resize(int(device_id), a.ctypes.data_as(C.c_void_p), 1 if a.dtype == np.float32 else 0, 0, n, h, w, float(fx), float(fy),
                           out.ctypes.data_as(C.c_void_p), 0, out.size, C.byref(oh), C.byref(ow)))
    return out[0] if single else out


def _bytes_ptr(data):
    """bytes / bytearray / uint8 array -> (keep-alive object, POINTER(c_uint8), length) without copying bytes objects."""
    if isinstance(data, bytes):
        return data, C.cast(C.c_char_p(data), C.POINTER(C.c_uint8)), len(data)
    a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.size


def jpeg_probe(data):
    """(h, w, components, layout) of one JPEG file's bytes (ctpn_jpeg_probe; host only). h, w: the size cv2.imread returns (an EXIF
    orientation 5 .. 8 swaps the stored ones). layout & 0xff = luma sampling: 1 (4:4:4, gray), 2 (4:2:0), 0x21 (4:2:2: 2 horizontally, 1
    vertically), 0x12 (4:4:0); layout >> 8 = EXIF orientation - 1. CtpnError with code CTPN_ERR_UNSUPPORTED for well-formed files the
    device decoder does not take (CMYK, 4:1:1, arithmetic coding, 12-bit ...)."""
    lib = load_library()
    keep, ptr, n = _bytes_ptr(data)
    h, w, nc, hs = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib.ctpn_jpeg_probe(ptr, n, C.byref(h), C.byref(w), C.byref(nc), C.byref(hs)))
    return h.value, w.value, nc.value, hs.value


def _path_array(paths):
    enc = [os.fsencode(p) for p in paths]
    return enc, (C.c_char_p * len(enc))(*enc)


def jpeg_probe_files(paths, threads=0):
    """Header scan of many files in one call (ctpn_jpeg_probe_files, C++ threads): (n, 4) int32 rows (h, w, components, luma sampling);
    h = 0 for files the device decoder does not take."""
    lib = load_library()
    paths = list(paths)
    keep, arr = _path_array(paths)
    out = np.zeros((len(paths), 4), np.int32)
    _check(lib.ctpn_jpeg_probe_files(arr, len(paths), _ptr(out, C.c_int), int(threads)))
    return out


def png_probe(data):
    """(h, w, colour type, bit depth) of one PNG file's bytes (ctpn_png_probe; host only). CtpnError(CTPN_ERR_UNSUPPORTED) for 16-bit files."""
    lib = load_library()
    keep, ptr, n = _bytes_ptr(data)
    h, w, ct, bd = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib.ctpn_png_probe(ptr, n, C.byref(h), C.byref(w), C.byref(ct), C.byref(bd)))
    return h.value, w.value, ct.value, bd.value


def png_backend(zlib_only=-1):
    """'libdeflate' or 'zlib': the DEFLATE back end ctpn_png_decode uses; zlib_only = 1 / 0 forces zlib / lifts that (test hook)."""
    return "libdeflate" if load_library().ctpn_debug_png_backend(int(zlib_only)) else "zlib"


def png_decode(data):
    """cv2.imread(IMREAD_COLOR) of one PNG file's bytes: (h, w, 3) BGR uint8 (ctpn_png_decode; reading is host work by the nature of the format)."""
    lib = load_library()
    h, w, _, _ = png_probe(data)
    keep, ptr, n = _bytes_ptr(data)
    out = np.zeros((h, w, 3), np.uint8)
    _check(lib.ctpn_png_decode(ptr, n, _ptr(out, C.c_uint8), out.size))
    return out


def png_encode_capacity(h, w):
    """Upper bound of the bytes one h x w PNG file written by this library can need (ctpn_png_encode_capacity)."""
    return int(load_library().ctpn_png_encode_capacity(int(h), int(w)))


def png_encode(bgr):
    """One (h, w, 3) BGR uint8 image as a PNG file's bytes, on the host (ctpn_png_encode: Sub filter, one dynamic-Huffman DEFLATE block,
    run-length and row-above matches): lossless; byte-equal to what Context.encode_png_batch writes on the device."""
    lib = load_library()
    bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
    if bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError("png_encode wants (h,w,3) uint8")
    h, w = int(bgr.shape[0]), int(bgr.shape[1])
    size = C.c_size_t(0)
    rc = lib.ctpn_png_encode(_ptr(bgr, C.c_uint8), h, w, None, 0, C.byref(size))
    if rc != CTPN_ERR_CAPACITY:
        _check(rc)
    out = np.empty((size.value,), np.uint8)
    _check(lib.ctpn_png_encode(_ptr(bgr, C.c_uint8), h, w, _ptr(out, C.c_uint8), out.size, C.byref(size)))
    return out[: size.value].tobytes()


def png_probe_files(paths, threads=0):
    """Header scan of many PNG files in one call (ctpn_png_probe_files): (n, 4) int32 rows (h, w, colour type, bit depth); h = 0 for files
    ctpn_decode_png_files does not take."""
    lib = load_library()
    paths = list(paths)
    keep, arr = _path_array(paths)
    out = np.zeros((len(paths), 4), np.int32)
    _check(lib.ctpn_png_probe_files(arr, len(paths), _ptr(out, C.c_int), int(threads)))
    return out


def decode_png_files(paths, h, w, threads=0, out=None):
    """n PNG files of one size -> (n, h, w, 3) BGR uint8 on the host, one file per C++ thread (ctpn_decode_png_files); `out` may be a
    caller's (page-locked) batch buffer."""
    lib = load_library()
    paths = list(paths)
    keep, arr = _path_array(paths)
    if out is None:
        out = np.empty((len(paths), int(h), int(w), 3), np.uint8)
    assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.shape == (len(paths), int(h), int(w), 3)
    _check(lib.ctpn_decode_png_files(arr, len(paths), int(h), int(w), _ptr(out, C.c_uint8), int(threads)))
    return out


def pack_canvas(ctx, images, factors, hc, wc):
    """BGR uint8 images of mixed sizes, each resized by its own factor, into one ragged canvas on the device (ctpn_pack_canvas). images:
    every item an (h, w, 3) uint8 array on the host (rows may be strided), or every item a device image (pointer, (h, w)) or (pointer,
    (h, w), pitch in bytes), read in place. factors: one resize_im factor per image (<= 0 or 1: no resize); every width must map to wc and
    every height to 16 .. hc. -> ((device pointer, (n, hc, wc)), heights int32), the form Context.decode_jpeg_ragged returns. ctx: a Context
    (None: the call reports what the library says without one -- CTPN_ERR_NODEVICE where no GPU is visible; there is no host form)."""
    lib = load_library()
    items = list(images)
    n = len(items)
    on_dev = [isinstance(it, (tuple, list)) for it in items]
    if any(on_dev) and not all(on_dev):
        raise ValueError("pack_canvas wants all images as host arrays or all as device (pointer, (h, w)[, pitch]) items")
    on_dev = bool(n) and all(on_dev)
    keep, ptrs = [], (C.c_void_p * max(n, 1))()
    hw = np.zeros((max(n, 1), 2), np.int32)
    pitch = np.zeros((max(n, 1),), np.int64)
    for i, it in enumerate(items):
        if on_dev:
            ptrs[i] = int(it[0]) if it[0] else None
            hw[i] = (int(it[1][0]), int(it[1][1]))
            pitch[i] = int(it[2]) if len(it) > 2 else 3 * int(it[1][1])
            continue
        a = np.asarray(it)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("pack_canvas wants (h, w, 3) uint8 images")
        if a.size and (a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]):
            a = np.ascontiguousarray(a)
        keep.append(a)
        ptrs[i] = a.ctypes.data
        hw[i] = a.shape[:2]
        pitch[i] = a.strides[0] if a.shape[0] > 1 else 3 * a.shape[1]
    fh, fw = np.ascontiguousarray(hw[:, 0]), np.ascontiguousarray(hw[:, 1])
    fac = np.ascontiguousarray(np.asarray(factors, np.float64).reshape(n))
    fac = fac if n else np.zeros((1,), np.float64)
    hts = np.zeros((max(n, 1),), np.int32)
    out = C.c_void_p(0)
    _check(lib.ctpn_pack_canvas(ctx._h if ctx is not None else None, ptrs, _ptr(fh, C.c_int), _ptr(fw, C.c_int), _ptr(pitch, C.c_longlong), 1 if on_dev else 0, n,
                                _ptr(fac, C.c_double), int(hc), int(wc), C.byref(out), _ptr(hts, C.c_int)))
    return (out.value, (n, int(hc), int(wc))), hts[:n]


def decode_png_files_ragged(ctx, paths, shapes, factors, hc, wc):
    """PNG files of mixed sizes into one ragged canvas on the device (ctpn_decode_png_files_ragged): the library's worker threads read and
    decode the files into page-locked memory, one copy and one kernel build the canvas. shapes: one (h, w) per file as png_probe_files
    reports it; factors, hc, wc and the result: as pack_canvas."""
    lib = load_library()
    paths = list(paths)
    n = len(paths)
    keep, arr = _path_array(paths)
    hw = np.ascontiguousarray(np.asarray(shapes, np.int32).reshape(n, 2)) if n else np.zeros((1, 2), np.int32)
    fh, fw = np.ascontiguousarray(hw[:, 0]), np.ascontiguousarray(hw[:, 1])
    fac = np.ascontiguousarray(np.asarray(factors, np.float64).reshape(n)) if n else np.zeros((1,), np.float64)
    hts = np.zeros((max(n, 1),), np.int32)
    out = C.c_void_p(0)
    _check(lib.ctpn_decode_png_files_ragged(ctx._h if ctx is not None else None, arr, n, _ptr(fh, C.c_int), _ptr(fw, C.c_int), _ptr(fac, C.c_double), int(hc), int(wc),
                                            C.byref(out), _ptr(hts, C.c_int)))
    return (out.value, (n, int(hc), int(wc))), hts[:n]


def jpeg_entropy_decode(data):
    """The host half of the JPEG decoder alone (ctpn_jpeg_entropy_decode; no device): returns (planes, qt, layout) with planes = one
    (block rows, block columns, 64) int16 array of quantised coefficients in natural order per component, qt = (3, 64) uint16 and
    layout = dict(h, w, ncomp, hs, vs, orientation); h, w are the STORED size."""
    lib = load_library()
    keep, ptr, n = _bytes_ptr(data)
    h, w, nc, hs = jpeg_probe(data)
    cap = int(lib.ctpn_jpeg_coef_capacity(h, w))
    coef = np.zeros((cap,), np.int16)
    qt = np.zeros((3, 64), np.uint16)
    l8 = np.zeros((8,), np.int32)
    _check(lib.ctpn_jpeg_entropy_decode(ptr, n, _ptr(coef, C.c_int16), cap, _ptr(qt, C.c_uint16), _ptr(l8, C.c_int)))
    h, w, nc, hs, bw0, bw1, bh0, bh1 = (int(v) for v in l8)       # h, w: as STORED (the probe's are the turned image's)
    hs, orient = hs & 0xff, (hs >> 8) + 1
    planes, off = [], 0
    for c in range(nc):
        bw, bh = (bw0, bh0) if c == 0 else (bw1, bh1)
        planes.append(coef[off: off + bw * bh * 64].reshape(bh, bw, 64))
        off += bw * bh * 64
    return planes, qt, {"h": h, "w": w, "ncomp": nc, "hs": hs, "vs": (bh0 // bh1 if nc == 3 else 1), "orientation": orient}


def jpeg_entropy_decode_device(ctx, files, subseq_bits=0, capacity=None):
    """The device Huffman decoder alone (ctpn_jpeg_entropy_decode_device; synchronous): n files of any mix of sizes and layouts ->
    (coef (n, capacity) int16, qt (n, 3, 64) uint16, layout8 (n, 8) int32, status (n,) int32), each file's part as ctpn_jpeg_entropy_decode
    fills it. capacity: int16 elements per file (default: the largest ctpn_jpeg_coef_capacity of the files that parse)."""
    lib = load_library()
    files = list(files)
    keeps = [_bytes_ptr(f) for f in files]
    n = len(keeps)
    if capacity is None:
        capacity = 64
        for f in files:
            try:
                h, w = jpeg_probe(f)[:2]
                capacity = max(capacity, int(lib.ctpn_jpeg_coef_capacity(h, w)))
            except CtpnError:
                pass
    ptrs = (C.POINTER(C.c_uint8) * n)(*[k[1] for k in keeps])
    sizes = (C.c_size_t * n)(*[k[2] for k in keeps])
    coef = np.zeros((n, int(capacity)), np.int16)
    qt = np.zeros((n, 3, 64), np.uint16)
    l8 = np.zeros((n, 8), np.int32)
    st = np.zeros((n,), np.int32)
    _check(lib.ctpn_jpeg_entropy_decode_device(ctx._h, ptrs, sizes, n, int(subseq_bits), _ptr(coef, C.c_int16), int(capacity), _ptr(qt, C.c_uint16),
                                               _ptr(l8, C.c_int), _ptr(st, C.c_int)))
    return coef, qt, l8, st


def jpeg_encode_capacity(h, w):
    """Upper bound of the bytes one h x w JPEG file written by this library can need (ctpn_jpeg_encode_capacity)."""
    return int(load_library().ctpn_jpeg_encode_capacity(int(h), int(w)))


def jpeg_entropy_encode(coef, layout8, qt):
    """The host half of the JPEG encoder alone (ctpn_jpeg_entropy_encode; no device): the flat int16 coefficient array (natural order),
    the 8 layout ints and the (3, 64) quantisation tables exactly as ctpn_jpeg_entropy_decode fills them -> the file's bytes."""
    lib = load_library()
    coef = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1)
    l8 = np.ascontiguousarray(layout8, dtype=np.int32).reshape(8)
    qt = np.ascontiguousarray(qt, dtype=np.uint16).reshape(192)
    n = C.c_size_t(0)
    rc = lib.ctpn_jpeg_entropy_encode(_ptr(coef, C.c_int16), _ptr(l8, C.c_int), _ptr(qt, C.c_uint16), None, 0, C.byref(n))
    if rc != CTPN_ERR_CAPACITY:
        _check(rc)
    out = np.empty((max(int(n.value), 1),), np.uint8)
    _check(lib.ctpn_jpeg_entropy_encode(_ptr(coef, C.c_int16), _ptr(l8, C.c_int), _ptr(qt, C.c_uint16), _ptr(out, C.c_uint8), out.size, C.byref(n)))
    return out[: n.value].tobytes()


def jpeg_entropy_encode_device(ctx, coefs, layouts, qts, capacities=None):
    """The device Huffman coder alone (ctpn_jpeg_entropy_encode_device; synchronous): n coefficient sets of any mix of sizes and layouts,
    each as jpeg_entropy_encode takes it -> (files, sizes, status): files[i] = the bytes written into a buffer of capacities[i] bytes
    (default: sized by a first call with no buffers; None where capacities[i] is 0), sizes[i] = the file's size as the library reports
    it (also of a file that did not fit), status[i] = that file's status. ctpn_last_error() holds the last failed file's message."""
    lib = load_library()
    coefs = [np.ascontiguousarray(c, dtype=np.int16).reshape(-1) for c in coefs]
    n = len(coefs)
    l8 = np.ascontiguousarray(np.asarray(layouts, np.int32).reshape(n, 8))
    qt = np.ascontiguousarray(np.asarray(qts, np.uint16).reshape(n, 192))
    cptr = (C.POINTER(C.c_int16) * n)(*[_ptr(c, C.c_int16) for c in coefs])
    sizes = (C.c_size_t * n)()
    st = np.zeros((n,), np.int32)
    if capacities is None:
        _check(lib.ctpn_jpeg_entropy_encode_device(ctx._h, cptr, _ptr(l8, C.c_int), _ptr(qt, C.c_uint16), n, (C.c_void_p * n)(), (C.c_size_t * n)(), sizes, _ptr(st, C.c_int)))
        capacities = [int(sizes[i]) for i in range(n)]
        sizes = (C.c_size_t * n)()
    bufs = [np.zeros((int(cap),), np.uint8) if cap else None for cap in capacities]
    optr = (C.c_void_p * n)(*[b.ctypes.data if b is not None else None for b in bufs])
    caps = (C.c_size_t * n)(*[int(cap) for cap in capacities])
    _check(lib.ctpn_jpeg_entropy_encode_device(ctx._h, cptr, _ptr(l8, C.c_int), _ptr(qt, C.c_uint16), n, optr, caps, sizes, _ptr(st, C.c_int)))
    files = [b[: min(int(sizes[i]), b.size)].tobytes() if b is not None else None for i, b in enumerate(bufs)]
    return files, [int(sizes[i]) for i in range(n)], st


def line_crop_width(rec, crop_h=32, max_w=512):
    """Width of the crop ctpn_crop_lines cuts for one text-line record at height crop_h (ctpn_line_crop_width; needs no device)."""
    r = np.ascontiguousarray(np.asarray(rec, np.float64).reshape(-1)[:9])
    if r.size < 8:
        raise ValueError("line_crop_width wants a record of 8 coordinates (+ score)")
    r = np.concatenate([r, np.zeros(9 - r.size)]) if r.size < 9 else r
    out = C.c_int(0)
    _check(load_library().ctpn_line_crop_width(_ptr(r, C.c_double), int(crop_h), int(max_w), C.byref(out)))
    return out.value


def _pack_lines(recs, line_counts, n):
    """recs: one (M_i, 9) array per image (line_counts None), or an (n, capacity, 9) array with line_counts -> packed array, counts"""
    if line_counts is None:
        recs = [np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 9) for r in recs]
        if len(recs) != n:
            raise ValueError("one array of records per image")
        packed = np.zeros((n, max([r.shape[0] for r in recs] + [1]), 9), np.float64)
        counts = np.zeros((n,), np.int32)
        for i, r in enumerate(recs):
            packed[i, : r.shape[0]] = r
            counts[i] = r.shape[0]
        return packed, counts
    packed = np.ascontiguousarray(recs, dtype=np.float64)
    counts = np.ascontiguousarray(line_counts, dtype=np.int32).reshape(-1)
    if packed.ndim != 3 or packed.shape[0] != n or packed.shape[2] != 9 or counts.shape[0] != n:
        raise ValueError("recs with line_counts wants (n, capacity, 9) and n counts")
    return packed, counts


def connector_cfg8(config):
    """config: None, a sequence of 8 values in CONNECTOR_CONSTANT_NAMES' order, a {TextLineCfg name: value} dict (missing names: the defaults;
    MIN_LINE_WIDTH or TEXT_PROPOSALS_WIDTH / MIN_NUM_PROPOSALS for the width), or any object with TextLineCfg's attributes -> the 8 doubles
    ctpn_text_lines_cfg takes (None stays None)."""
    if config is None:
        return None
    if isinstance(config, (list, tuple, np.ndarray)):
        out = np.ascontiguousarray(config, dtype=np.float64).reshape(-1)
        if out.shape[0] != 8:
            raise ValueError("a connector configuration holds 8 values")
        return out
    get = config.get if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    if isinstance(config, dict):
        known = set(CONNECTOR_PARAM_NAMES) | {"TEXT_PROPOSALS_WIDTH", "MIN_NUM_PROPOSALS", "SCALE", "MAX_SCALE"}
        unknown = sorted(set(config) - known)
        if unknown:
            raise ValueError("unknown connector parameter(s): " + ", ".join(unknown))
    out = np.array([param_default(n) for n in CONNECTOR_PARAM_NAMES], np.float64)
    for k, name in enumerate(CONNECTOR_PARAM_NAMES):
        v = get(name, None)
        if name == "MIN_LINE_WIDTH" and v is None and (get("TEXT_PROPOSALS_WIDTH", None) is not None or get("MIN_NUM_PROPOSALS", None) is not None):
            v = float(get("TEXT_PROPOSALS_WIDTH", 16)) * float(get("MIN_NUM_PROPOSALS", 2))
        if v is not None:
            out[k] = float(v)
    return out


def text_lines(boxes, scores, size, mode="H", device_id=0, capacity=4096, config=None):
    """B4 seam: TextDetector.detect (reference lib/text_connector/detectors.py:19-35). config: see connector_cfg8 (None: the defaults)."""
    lib = load_library()
    cfg8 = connector_cfg8(config)
    b = _f32(boxes).reshape(-1, 4)
    s = _f32(scores).reshape(-1)
    recs = np.zeros((capacity, 9), np.float64)
    cnt = C.c_int(0)
    m = MODE_O if str(mode).upper().startswith("O") else MODE_H
    if cfg8 is None:
        _check(lib.ctpn_text_lines(_ptr(b, C.c_float), _ptr(s, C.c_float), int(b.shape[0]), int(size[0]), int(size[1]), m,
                                   int(device_id), _ptr(recs, C.c_double), capacity, C.byref(cnt)))
    else:
        _check(lib.ctpn_text_lines_cfg(_ptr(b, C.c_float), _ptr(s, C.c_float), int(b.shape[0]), int(size[0]), int(size[1]), m,
                                       int(device_id), _ptr(cfg8, C.c_double), _ptr(recs, C.c_double), capacity, C.byref(cnt)))
    return recs[: cnt.value].copy()


# ---- pages in tiles (ctpn_page_*; the orchestration over a ctx: page.py) ----
def page_plan(page_h, page_w, tile_h, tile_w, overlap):
    """ctpn_page_plan -> (tiles, (rows, columns)): tiles (k, 8) int32 records {oy, ox, valid_h, valid_w, own_y0, own_y1, own_x0, own_x1}, row-major.
    Host arithmetic of the library, needs no GPU."""
    lib = load_library()
    cnt, grid = C.c_int(0), np.zeros((2,), np.int32)
    args = (int(page_h), int(page_w), int(tile_h), int(tile_w), int(overlap))
    _check(lib.ctpn_page_plan(*args, None, 0, C.byref(cnt), _ptr(grid, C.c_int)))
    tiles = np.zeros((cnt.value, 8), np.int32)
    _check(lib.ctpn_page_plan(*args, _ptr(tiles, C.c_int), cnt.value, C.byref(cnt), _ptr(grid, C.c_int)))
    return tiles, (int(grid[0]), int(grid[1]))


def page_cut(page, tiles, first, n, tile_h, tile_w, device_id=0, out_ptr=None, page_ptr=None, page_shape=None, pitch=None):
    """ctpn_page_cut: tiles first .. first + n - 1 of the plan out of the page. page: an (h, w, 3) uint8 array whose rows may lie `pitch` bytes
    apart (a view of a wider buffer), or page_ptr / page_shape = (h, w) / pitch for a page in device memory. out_ptr: a device buffer of
    n x tile_h x tile_w x 3 bytes to fill (returns None); without it the tiles come back as an (n, tile_h, tile_w, 3) array."""
    lib = load_library()
    t = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 8)
    if first < 0 or n <= 0 or first + n > t.shape[0]:
        raise ValueError("page_cut: tiles %d .. %d of a plan of %d" % (first, first + n - 1, t.shape[0]))
    if page_ptr is not None:
        h, w = page_shape
        src, on_dev, pb = C.c_void_p(int(page_ptr)), 1, int(pitch if pitch is not None else 3 * w)
    else:
        if page.dtype != np.uint8 or page.ndim != 3 or page.shape[2] != 3 or page.strides[1:] != (3, 1) or (page.shape[0] > 1 and page.strides[0] < 3 * page.shape[1]):
            raise ValueError("page_cut wants an (h, w, 3) uint8 page with contiguous rows")
        h, w = page.shape[:2]
        src, on_dev, pb = C.c_void_p(page.ctypes.data), 0, int(page.strides[0])
    need = int(n) * int(tile_h) * int(tile_w) * 3
    out = None
    if out_ptr is None:
        out = np.empty((int(n), int(tile_h), int(tile_w), 3), np.uint8)
    dst, dst_dev = (C.c_void_p(int(out_ptr)), 1) if out_ptr is not None else (out.ctypes.data_as(C.c_void_p), 0)
    _check(lib.ctpn_page_cut(int(device_id), src, on_dev, int(h), int(w), pb, _ptr(t, C.c_int), int(first), int(n), int(tile_h), int(tile_w), dst, dst_dev, need))
    return out


def page_merge(tiles, rois, roi_counts, page_h, page_w, min_size):
    """ctpn_page_merge: rois (n_tiles, capacity, 5) rows [score, x1, y1, x2, y2] in tile coordinates + their counts -> (boxes (m, 4), scores (m,),
    src (m,) = tile * capacity + row) in page coordinates, each page cell's proposals from the one tile that owns it. Needs no GPU."""
    lib = load_library()
    t = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 8)
    r = _f32(rois)
    c = np.ascontiguousarray(roi_counts, dtype=np.int32).reshape(-1)
    if r.ndim != 3 or r.shape[2] != 5 or r.shape[0] != t.shape[0] or c.shape[0] != t.shape[0]:
        raise ValueError("page_merge wants rois (n_tiles, capacity, 5) and n_tiles counts")
    cap = max(int(c.clip(0, None).sum()), 1)
    boxes, scores, src = np.zeros((cap, 4), np.float32), np.zeros((cap,), np.float32), np.zeros((cap,), np.int32)
    cnt = C.c_int(0)
    _check(lib.ctpn_page_merge(_ptr(t, C.c_int), int(t.shape[0]), _ptr(r, C.c_float), int(r.shape[1]), _ptr(c, C.c_int), int(page_h), int(page_w), float(min_size),
                               _ptr(boxes, C.c_float), _ptr(scores, C.c_float), _ptr(src, C.c_int), cap, C.byref(cnt)))
    return boxes[: cnt.value].copy(), scores[: cnt.value].copy(), src[: cnt.value].copy()


def page_nms_sorted(boxes_sorted, thresh, device_id=0):
    """ctpn_page_nms: nms_sorted's contract by the page form of the column NMS (boxes on the 16-px column grid, thresh >= 0.1)."""
    lib = load_library()
    b = _f32(boxes_sorted)
    n = int(b.shape[0])
    if n == 0:
        return np.zeros((0,), np.int32)
    keep = np.zeros((n,), np.int32)
    num = C.c_int(0)
    _check(lib.ctpn_page_nms(_ptr(keep, C.c_int), C.byref(num), _ptr(b, C.c_float), n, int(b.shape[1]), float(thresh), int(device_id)))
    return keep[: num.value]


def page_text_lines(boxes, scores, size, mode="H", device_id=0, capacity=4096, config=None, nms_form=0):
    """ctpn_page_text_lines: text_lines' contract and records, the NMS inside by nms_form: 0 = ctpn_nms, 1 = ctpn_page_nms."""
    lib = load_library()
    cfg8 = connector_cfg8(config)
    b = _f32(boxes).reshape(-1, 4)
    s = _f32(scores).reshape(-1)
    m = MODE_O if str(mode).upper().startswith("O") else MODE_H
    while True:
        recs = np.zeros((capacity, 9), np.float64)
        cnt = C.c_int(0)
        rc = lib.ctpn_page_text_lines(_ptr(b, C.c_float), _ptr(s, C.c_float), int(b.shape[0]), int(size[0]), int(size[1]), m, int(device_id),
                                      None if cfg8 is None else _ptr(cfg8, C.c_double), int(nms_form), _ptr(recs, C.c_double), capacity, C.byref(cnt))
        if rc == CTPN_ERR_CAPACITY and cnt.value > capacity:      # a page holds more lines than an image: once more with room for all
            capacity = cnt.value
            continue
        _check(rc)
        return recs[: cnt.value].copy()


CONNECTOR_CONSTANT_NAMES = ("TEXT_PROPOSALS_WIDTH * MIN_NUM_PROPOSALS", "MIN_RATIO", "LINE_MIN_SCORE", "MAX_HORIZONTAL_GAP", "TEXT_PROPOSALS_MIN_SCORE",
                            "TEXT_PROPOSALS_NMS_THRESH", "MIN_V_OVERLAPS", "MIN_SIZE_SIM")
# the same eight as ctx parameters (ctpn_set_param), in the same order
CONNECTOR_PARAM_NAMES = ("MIN_LINE_WIDTH",) + CONNECTOR_CONSTANT_NAMES[1:]


def connector_constants():
    """{name: value} of the connector constants compiled into the library (ctpn_connector_constants)."""
    out = np.zeros((8,), np.float64)
    _check(load_library().ctpn_connector_constants(_ptr(out, C.c_double)))
    return dict(zip(CONNECTOR_CONSTANT_NAMES, out.tolist()))


def result_text(recs, scale):
    """bytes of res_<stem>.txt for (M,9) records (ctpn_result_text; reference ctpn/demo.py:28-49). Host C++, needs no GPU."""
    lib = load_library()
    r = np.ascontiguousarray(recs, dtype=np.float64).reshape(-1, 9)
    n = C.c_size_t(0)
    _check(lib.ctpn_result_text(_ptr(r, C.c_double), int(r.shape[0]), float(scale), None, 0, C.byref(n), None))
    buf = C.create_string_buffer(max(int(n.value), 1))
    _check(lib.ctpn_result_text(_ptr(r, C.c_double), int(r.shape[0]), float(scale), buf, len(buf), C.byref(n), None))
    return buf.raw[: n.value]


def write_result_file(path, recs, scale):
    lib = load_library()
    r = np.ascontiguousarray(recs, dtype=np.float64).reshape(-1, 9)
    cnt = C.c_int(0)
    _check(lib.ctpn_write_result_file(str(path).encode(), _ptr(r, C.c_double), int(r.shape[0]), float(scale), C.byref(cnt)))
    return cnt.value


def draw_boxes(img_bgr, recs):
    """Outlines of the text lines into a (h,w,3) uint8 BGR image, in place (ctpn_draw_boxes)."""
    lib = load_library()
    if img_bgr.dtype != np.uint8 or img_bgr.ndim != 3 or img_bgr.shape[2] != 3 or not img_bgr.flags["C_CONTIGUOUS"]:
        raise ValueError("draw_boxes wants a C-contiguous (h,w,3) uint8 image")
    r = np.ascontiguousarray(recs, dtype=np.float64).reshape(-1, 9)
    _check(lib.ctpn_draw_boxes(_ptr(img_bgr, C.c_uint8), int(img_bgr.shape[0]), int(img_bgr.shape[1]), _ptr(r, C.c_double), int(r.shape[0])))
    return img_bgr


def debug_connect(rois, size, mode="H", scale=1.0, device_id=0, capacity=512):
    """TextDetector.detect on the device connector (lines_prep -> nms 0.2 -> connect_kernel) for one image's rois (R,5)."""
    lib = load_library()
    r = _f32(rois).reshape(-1, 5)
    recs = np.zeros((capacity, 9), np.float64)
    cnt = C.c_int(0)
    m = MODE_O if str(mode).upper().startswith("O") else MODE_H
    _check(lib.ctpn_debug_connect(int(device_id), _ptr(r, C.c_float), int(r.shape[0]), int(size[0]), int(size[1]), float(scale), m,
                                  _ptr(recs, C.c_double), capacity, C.byref(cnt)))
    return recs[: cnt.value].copy()


COMM_ID_BYTES = 128


def comm_unique_id():
    """RCCL unique id (ctpn_comm_unique_id): created by the root, handed to the other ranks through any side channel."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load_library().ctpn_comm_unique_id(buf, COMM_ID_BYTES))
    return buf.raw


def broadcast_weights(contexts):
    """One process, one ctx per GPU: contexts[0]'s loaded weights reach every other ctx over RCCL (ctpn_broadcast_weights)."""
    arr = (C.c_void_p * len(contexts))(*[c._h.value for c in contexts])
    _check(load_library().ctpn_broadcast_weights(arr, len(contexts)))


def ragged_valid_rows(height, level):
    """Valid rows of an image of `height` pixel rows at pooling level 0 .. 4 (ctpn_ragged_valid_rows; needs no device)."""
    r = load_library().ctpn_ragged_valid_rows(int(height), int(level))
    if r < 0:
        raise ValueError("ragged_valid_rows: height >= 0 and 0 <= level <= 4 required")
    return r


def host_thread_budget(cpu_count, local_world_size=1, requested=0):
    """ctpn_host_thread_budget: host workers per ctx (pure function of its arguments, no GPU needed)."""
    return int(load_library().ctpn_host_thread_budget(int(cpu_count), int(local_world_size), int(requested)))


def live_resources():
    """ctpn_debug_live_resources: (device bytes, page-locked bytes, events, streams) the library's host side holds in this process right now
    (pure host read: no ctx, no GPU needed)."""
    out = (C.c_longlong * 4)()
    _check(load_library().ctpn_debug_live_resources(out))
    return tuple(int(v) for v in out)


def debug_cvt_bf16(x, use_hw=True, device_id=0):
    lib = load_library()
    x = _f32(x).reshape(-1)
    out = np.zeros((x.size,), np.uint16)
    _check(lib.ctpn_debug_cvt_bf16(int(device_id), _ptr(x, C.c_float), _ptr(out, C.c_uint16), int(x.size), 1 if use_hw else 0))
    return out


def debug_lds_dma(src, device_id=0):
    """ctpn_debug_lds_dma: (bytes through the m0-clobber form, bytes through the save / restore form) of the kernels' LDS-DMA helper."""
    lib = load_library()
    src = np.ascontiguousarray(src, np.uint8).reshape(-1)
    a, b = np.zeros_like(src), np.zeros_like(src)
    _check(lib.ctpn_debug_lds_dma(int(device_id), _ptr(src, C.c_uint8), src.size, _ptr(a, C.c_uint8), _ptr(b, C.c_uint8)))
    return a, b


def debug_conv3x3(x, w_hwio, bias, precision="fp32", impl=1, fuse_pool=False, want_full=True, device_id=0, dup_hi=False):
    """Unit-test hook (ctpn_debug_conv3x3): returns (full or None, pooled or None) as dense fp32 NHWC."""
    lib = load_library()
    x = _f32(x); w_hwio = _f32(w_hwio); bias = _f32(bias)
    n, h, w, ci = x.shape
    co = w_hwio.shape[3]
    full = np.zeros((n, h, w, co), np.float32) if want_full else None
    pooled = np.zeros((n, h // 2, w // 2, co), np.float32) if fuse_pool else None
    prec = precision_code(precision)
    if dup_hi:      # impl 3: impl 1 with the [hi | lo | hi] pixel of the layer that feeds the LSTM projection (the library compares the planes)
        assert impl == 1
        impl = 3
    _check(lib.ctpn_debug_conv3x3(int(device_id), _ptr(x, C.c_float), _ptr(w_hwio, C.c_float), _ptr(bias, C.c_float), n, h, w, ci,
                                  co, prec, int(impl), 1 if fuse_pool else 0,
                                  _ptr(full, C.c_float) if want_full else None, _ptr(pooled, C.c_float) if fuse_pool else None))
    return full, pooled


CONV_PLAN_INTS = 6      # CTPN_CONV_PLAN_INTS
ConvPlan = collections.namedtuple("ConvPlan", "main strip cols w_cover deep ks")


def conv3x3_form_names():
    """(main form names, strip kind names) by id, as ctpn_debug_conv3x3_form_name gives them."""
    lib = load_library()
    out = []
    for kind in (0, 1):
        names, i = [], 0
        while True:
            s = lib.ctpn_debug_conv3x3_form_name(kind, i)
            if s is None:
                break
            names.append(s.decode())
            i += 1
        out.append(names)
    return tuple(out)


def conv3x3_plan_sweep(precision, n, h, w_first, w_count, ci, co, pool, keep_full=True, dup_hi=False, conv_p64=1, split_edge=1, cu_count=0):
    """ctpn_debug_conv3x3_plan: int32 array [w_count, CONV_PLAN_INTS] -- the plans of the widths w_first .. w_first + w_count - 1 (ids, see
    conv3x3_form_names). cu_count 0 asks the current device; any other value needs no device."""
    lib = load_library()
    out = np.zeros((int(w_count), CONV_PLAN_INTS), np.int32)
    _check(lib.ctpn_debug_conv3x3_plan(precision_code(precision), int(n), int(h), int(w_first), int(w_count), int(ci), int(co), 1 if pool else 0,
                                       1 if keep_full else 0, 1 if dup_hi else 0, int(conv_p64), int(split_edge), int(cu_count), _ptr(out, C.c_int)))
    return out


def conv3x3_plan(precision, n, h, w, ci, co, pool, keep_full=True, dup_hi=False, conv_p64=1, split_edge=1, cu_count=0):
    """The plan of one layer shape as a ConvPlan of names and numbers: (main, strip, cols, w_cover, deep, ks)."""
    mains, strips = conv3x3_form_names()
    p = [int(v) for v in conv3x3_plan_sweep(precision, n, h, w, 1, ci, co, pool, keep_full, dup_hi, conv_p64, split_edge, cu_count)[0]]
    return ConvPlan(mains[p[0]], strips[p[1]], p[2], p[3], p[4], p[5])


CONV_WALK_INTS = 14     # CTPN_CONV_WALK_INTS
ConvWalk = collections.namedtuple("ConvWalk", "main tiles_x tiles_y tiles_n stacked total workers ht_full ht_r groups per_group grid chunks ht")


def conv3x3_walk_sweep(precision, n, h, w_first, w_count, ci, co, pool, keep_full=True, dup_hi=False, conv_p64=1, split_edge=1, cu_count=0):
    """ctpn_debug_conv3x3_walk_plan: int32 array [w_count, CONV_WALK_INTS] -- the tile walks of the main launch for the widths w_first ..
    w_first + w_count - 1 (the fields of ConvWalk; main as an id). cu_count 0 asks the current device; any other value needs no device."""
    lib = load_library()
    out = np.zeros((int(w_count), CONV_WALK_INTS), np.int32)
    _check(lib.ctpn_debug_conv3x3_walk_plan(precision_code(precision), int(n), int(h), int(w_first), int(w_count), int(ci), int(co), 1 if pool else 0,
                                            1 if keep_full else 0, 1 if dup_hi else 0, int(conv_p64), int(split_edge), int(cu_count), _ptr(out, C.c_int)))
    return out


def conv3x3_walk_plan(precision, n, h, w, ci, co, pool, keep_full=True, dup_hi=False, conv_p64=1, split_edge=1, cu_count=0):
    """The tile walk of one layer shape's main launch as a ConvWalk (main: the form's name)."""
    p = [int(v) for v in conv3x3_walk_sweep(precision, n, h, w, 1, ci, co, pool, keep_full, dup_hi, conv_p64, split_edge, cu_count)[0]]
    return ConvWalk(conv3x3_form_names()[0][p[0]], *p[1:])


def debug_conv3x3_walk(x, w_hwio, bias, precision="fp32", fuse_pool=False, want_full=True, cu_count=0, device_id=0, dup_hi=False):
    """ctpn_debug_conv3x3_walk: debug_conv3x3 through the product kernels with the main launch laid out for cu_count CUs (0: the device's own)
    and guarded output maps (a written border pixel or guard row raises CtpnError, CTPN_ERR_STATE). Returns (full or None, pooled or None)."""
    lib = load_library()
    x = _f32(x); w_hwio = _f32(w_hwio); bias = _f32(bias)
    n, h, w, ci = x.shape
    co = w_hwio.shape[3]
    full = np.zeros((n, h, w, co), np.float32) if want_full else None
    pooled = np.zeros((n, h // 2, w // 2, co), np.float32) if fuse_pool else None
    _check(lib.ctpn_debug_conv3x3_walk(int(device_id), _ptr(x, C.c_float), _ptr(w_hwio, C.c_float), _ptr(bias, C.c_float), n, h, w, ci,
                                       co, precision_code(precision), 3 if dup_hi else 1, 1 if fuse_pool else 0, int(cu_count),
                                       _ptr(full, C.c_float) if want_full else None, _ptr(pooled, C.c_float) if fuse_pool else None))
    return full, pooled


LstmPrePlan = collections.namedtuple("LstmPrePlan", "form waves workgroups idle_waves")
LSTM_PRE_FORMS = ("small", "lds")
BILSTM_FORMS = ("exact", "exact_fast_gates", "split_16", "split_few")


def lstm_pre_plan(cells, cu_count=0):
    """ctpn_debug_lstm_pre_plan: the launch shape of launch_lstm_pre for `cells` cells as (form name, waves per workgroup, workgroups, whole
    idle waves of the last workgroup). cu_count 0 asks the current device; any other value needs no device."""
    p = np.zeros(4, np.int32)
    _check(load_library().ctpn_debug_lstm_pre_plan(int(cells), int(cu_count), _ptr(p, C.c_int)))
    return LstmPrePlan(LSTM_PRE_FORMS[int(p[0])], int(p[1]), int(p[2]), int(p[3]))


def debug_lstm_pre(x, wx, bias, precision="fp16", cu_count=0, device_id=0):
    """ctpn_debug_lstm_pre: x (n, hf, wf, 512), wx (512, 1024), bias (1024,) in TF's gate order -> lstm_pre (n, hf, wf, 1024) fp32 values."""
    x = _f32(x); wx = _f32(wx); bias = _f32(bias)
    n, hf, wf, ci = x.shape
    assert ci == 512 and wx.shape == (512, 1024) and bias.shape == (1024,)
    out = np.zeros((n, hf, wf, 1024), np.float32)
    _check(load_library().ctpn_debug_lstm_pre(int(device_id), _ptr(x, C.c_float), _ptr(wx, C.c_float), _ptr(bias, C.c_float), n, hf, wf,
                                              precision_code(precision), int(cu_count), _ptr(out, C.c_float)))
    return out


def debug_bilstm(pre, wh, split=False, fast_gates=False, pre_f16=False, device_id=0):
    """ctpn_debug_bilstm: pre (rows, T, 1024) in TF's gate order, wh (2, 128, 512) -> (lstm_out (rows, T, 256), the launcher's form name)."""
    pre = _f32(pre); wh = _f32(wh)
    rows, T, c = pre.shape
    assert c == 1024 and wh.shape == (2, 128, 512)
    out = np.zeros((rows, T, 256), np.float32)
    form = C.c_int(-1)
    _check(load_library().ctpn_debug_bilstm(int(device_id), _ptr(pre, C.c_float), _ptr(wh, C.c_float), rows, T, 1 if split else 0,
                                            1 if fast_gates else 0, 1 if pre_f16 else 0, _ptr(out, C.c_float), C.byref(form)))
    return out, BILSTM_FORMS[form.value]


def debug_gemm(a, w, bias, ldc=None, precision="fp32", device_id=0):
    """ctpn_debug_gemm: a (M, K) @ w (K, Co) + bias -> (M, ldc) fp32; columns Co .. ldc - 1 hold the hook's fill (bytes 0xC3)."""
    a = _f32(a); w = _f32(w); bias = _f32(bias)
    (M, K), Co = a.shape, w.shape[1]
    assert w.shape[0] == K and bias.shape == (Co,)
    ldc = Co if ldc is None else int(ldc)
    out = np.zeros((M, ldc), np.float32)
    _check(load_library().ctpn_debug_gemm(int(device_id), _ptr(a, C.c_float), _ptr(w, C.c_float), _ptr(bias, C.c_float), M, K, Co, ldc,
                                          precision_code(precision), _ptr(out, C.c_float)))
    return out


CONV1_FORMS = ("valu", "mfma", "q")      # ctpn_debug_conv1's form 0, 1, 2


def conv1_q_shape(h, w):
    """(Hq, Wq) of the q-image of an h x w image (csrc/common.h: conv1_q_h, conv1_q_w)"""
    return (h + 7) // 8 * 8 + 4, (w + 63) // 64 * 64 + 8


def debug_conv1(images, w_hwio, bias, precision="bf16", form=0, byte_offset=0, want_bits=False, want_q=False, device_id=0):
    """ctpn_debug_conv1: one conv1_1 kernel on caller data. images (n, h, w, 3): uint8 = the uint8 feed, anything else = the float blob feed.
    Returns (conv1_1 (n, h, w, 64) fp32, the stored 16-bit values (n, h, w, 64 | 128) uint16 or None, the q-image (n, Hq, Wq, 4) uint16 or None)."""
    images = np.asarray(images)
    is_f32 = images.dtype != np.uint8
    images = np.ascontiguousarray(images, dtype=np.float32 if is_f32 else np.uint8)
    w_hwio = _f32(w_hwio); bias = _f32(bias)
    n, h, w, c = images.shape
    assert c == 3 and w_hwio.shape == (3, 3, 3, 64) and bias.shape == (64,)
    out = np.zeros((n, h, w, 64), np.float32)
    bits = np.zeros((n, h, w, 128 if precision == "split" else 64), np.uint16) if want_bits else None
    q = np.zeros((n,) + conv1_q_shape(h, w) + (4,), np.uint16) if want_q else None
    _check(load_library().ctpn_debug_conv1(int(device_id), images.ctypes.data_as(C.c_void_p), 1 if is_f32 else 0, int(byte_offset), _ptr(w_hwio, C.c_float),
                                           _ptr(bias, C.c_float), n, h, w, precision_code(precision), int(form), _ptr(out, C.c_float),
                                           _ptr(bits, C.c_uint16) if want_bits else None, _ptr(q, C.c_uint16) if want_q else None))
    return out, bits, q


def debug_conv1_fused(images, w_hwio, bias, w2_hwio, bias2, precision="bf16", byte_offset=0, device_id=0, cu_count=None):
    """ctpn_debug_conv1_fused: uint8 images -> q-image -> conv1_2 with conv1_1 in its window stage and the pool fused.
    cu_count (not None: ctpn_debug_conv1_fused_walk): conv1_2's launch laid out for that many CUs, 0 = the device's own.
    Returns (pool1 (n, h // 2, w // 2, 64) fp32, its stored 16-bit values as uint16)."""
    images = np.ascontiguousarray(images, dtype=np.uint8)
    w_hwio = _f32(w_hwio); bias = _f32(bias); w2_hwio = _f32(w2_hwio); bias2 = _f32(bias2)
    n, h, w, c = images.shape
    assert c == 3 and w_hwio.shape == (3, 3, 3, 64) and bias.shape == (64,) and w2_hwio.shape == (3, 3, 64, 64) and bias2.shape == (64,)
    out = np.zeros((n, h // 2, w // 2, 64), np.float32)
    bits = np.zeros((n, h // 2, w // 2, 64), np.uint16)
    head = (int(device_id), _ptr(images, C.c_uint8), int(byte_offset), _ptr(w_hwio, C.c_float), _ptr(bias, C.c_float), _ptr(w2_hwio, C.c_float),
            _ptr(bias2, C.c_float), n, h, w, precision_code(precision))
    if cu_count is None:
        _check(load_library().ctpn_debug_conv1_fused(*head, _ptr(out, C.c_float), _ptr(bits, C.c_uint16)))
    else:
        _check(load_library().ctpn_debug_conv1_fused_walk(*head, int(cu_count), _ptr(out, C.c_float), _ptr(bits, C.c_uint16)))
    return out, bits


ProposalPlan = collections.namedtuple("ProposalPlan", "npad fill_keys sort seg_len last_seg merge_wgs nms group_wgs prefix")
PROPOSAL_SORT_FORMS = ("one_wg", "segmented")
PROPOSAL_NMS_FORMS = ("generic", "one_wg", "groups")
PROPOSAL_PREFIX = ("none", "in_kernel", "two_launches")
SORT_POISON = 0x00000000C3C3C3C3
KEY_INVALID = 0xFFFFFFFFFFFFFFFF
# ctpn_debug_proposal_fetch: name -> (CTPN_PF_*, dtype, shape of one image from (per_img, npad, pre, post))
PROPOSAL_FETCH = {
    "boxes4": (0, np.float32, lambda a, p, pre, post: (a, 4)), "sorted_keys": (1, np.uint64, lambda a, p, pre, post: (p,)),
    "sorted_boxes": (2, np.float32, lambda a, p, pre, post: (pre, 4)), "sorted_scores": (3, np.float32, lambda a, p, pre, post: (pre,)),
    "sorted_anchor": (4, np.int32, lambda a, p, pre, post: (pre,)), "valid_counts": (5, np.int32, lambda a, p, pre, post: ()),
    "colid": (6, np.uint8, lambda a, p, pre, post: (pre,)), "keep_idx": (7, np.int32, lambda a, p, pre, post: (post,)),
    "keep_counts": (8, np.int32, lambda a, p, pre, post: ()), "mw_scratch": (9, np.uint8, lambda a, p, pre, post: (2048,)),
    "im_info": (10, np.float32, lambda a, p, pre, post: (3,)),
}


def proposal_plan_sweep(n, hf_first, hf_count, wf_first, wf_count, pre=12000, post=1000, thresh=0.7, nms_columns=1, nms_prefix=1, mw_scratch=True,
                        im_widths=None):
    """ctpn_debug_proposal_plan over a block of maps: int32 (hf_count, wf_count, 9), the raw plan of every map. No device."""
    out = np.zeros((hf_count, wf_count, 9), np.int32)
    w = None if im_widths is None else _f32(im_widths).reshape(n)
    _check(load_library().ctpn_debug_proposal_plan(int(nms_columns), int(nms_prefix), 1 if mw_scratch else 0, int(n), int(hf_first), int(hf_count),
                                                   int(wf_first), int(wf_count), int(pre), int(post), float(thresh),
                                                   None if w is None else _ptr(w, C.c_float), _ptr(out, C.c_int)))
    return out


POST_NMS_CAPACITY_MAX = 4096      # CTPN_POST_NMS_CAPACITY_MAX
TEXT_LINE_NMS_FORMS = ("generic", "one_wg", "column_groups", "one_wg_large")
TEXT_LINE_CONN_FORMS = ("host", "all_pairs", "buckets")


def text_line_plan(n, wf, rows, thresh=0.2, max_scale=1.0, nms_columns=1, connect_device=0, mw_scratch=True):
    """ctpn_debug_text_line_plan: (NMS form, connector form, column-group workgroups per image) of the text-line tail. No device."""
    out = np.zeros((3,), np.int32)
    _check(load_library().ctpn_debug_text_line_plan(int(nms_columns), int(connect_device), 1 if mw_scratch else 0, int(n), int(wf), int(rows),
                                                    float(thresh), float(max_scale), _ptr(out, C.c_int)))
    return TEXT_LINE_NMS_FORMS[out[0]], TEXT_LINE_CONN_FORMS[out[1]], int(out[2])


def check_post_nms_topn(post_nms_topn):
    """cfg.TEST.RPN_POST_NMS_TOP_N as the mirror modules read it: the reference takes any value, this library up to POST_NMS_CAPACITY_MAX."""
    post = int(post_nms_topn)
    if post > POST_NMS_CAPACITY_MAX:
        raise ValueError("RPN_POST_NMS_TOP_N = %d exceeds the limit of %d proposals per image (CTPN_POST_NMS_CAPACITY_MAX)" % (post, POST_NMS_CAPACITY_MAX))
    return post


def reserve_for(ctx, post_nms_topn):
    """What the mirror modules do before a proposal call: raise the ctx's capacity where cfg.TEST.RPN_POST_NMS_TOP_N exceeds it."""
    post = check_post_nms_topn(post_nms_topn)
    if post > ctx.proposal_capacity:
        ctx.reserve_proposals(post)


def proposal_plan(n, hf, wf, **kw):
    """The plan of one ctpn_proposals* call as a ProposalPlan of names and numbers (see ctpn_debug_proposal_plan)."""
    p = [int(v) for v in proposal_plan_sweep(n, hf, 1, wf, 1, **kw)[0, 0]]
    return ProposalPlan(p[0], bool(p[1]), PROPOSAL_SORT_FORMS[p[2]], p[3], p[4], p[5], PROPOSAL_NMS_FORMS[p[6]], p[7], PROPOSAL_PREFIX[p[8]])


def debug_sort_keys(keys, segmented, device_id=0):
    """ctpn_debug_sort_keys: keys (n_img, per_img) uint64 -> (n_img, npad) uint64, the buffer that holds launch_sort_keys' result (behind per_img:
    SORT_POISON in the one-workgroup form, KEY_INVALID in the segmented one)."""
    k = np.ascontiguousarray(keys, np.uint64)
    n_img, per_img = k.shape
    npad = 1
    while npad < per_img:
        npad <<= 1
    out = np.zeros((n_img, npad), np.uint64)
    _check(load_library().ctpn_debug_sort_keys(int(device_id), _ptr(k, C.c_ulonglong), n_img, per_img, 1 if segmented else 0, _ptr(out, C.c_ulonglong)))
    return out


class Context:
    """One ctpn_ctx: a GPU, a stream and the HBM arena for up to max_batch images of max_h x max_w."""

    def __init__(self, device_id=0, max_batch=1, max_h=600, max_w=900, precision="bf16", postproc_only=False, options=None):
        """precision: "fp32" | "bf16" | "fp16" | "split" (CTPN_PREC_*). options: {name: int} for ctpn_set_option (see OPTION_ENV).
        postproc_only: ctpn_create_postproc -- proposal-layer buffers for max_h//16 x max_w//16 feature maps, no network."""
        self._lib = load_library()
        self._h = C.c_void_p()
        self.precision = precision
        self.postproc_only = bool(postproc_only)
        prec = precision_code(precision)
        if postproc_only:
            _check(self._lib.ctpn_create_postproc(C.byref(self._h), int(device_id), int(max_batch), int(max_h) // 16, int(max_w) // 16))
        else:
            _check(self._lib.ctpn_create(C.byref(self._h), int(device_id), int(max_batch), int(max_h), int(max_w), prec))
        self.device_id = device_id
        self.max_batch, self.max_h, self.max_w = max_batch, max_h, max_w
        opts = {k: int(os.environ[e]) for k, e in OPTION_ENV.items() if os.environ.get(e, "") != ""}
        opts.update(options or {})
        for k, v in opts.items():
            self.set_option(k, v)

    def set_option(self, key, value):
        _check(self._lib.ctpn_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int(0)
        _check(self._lib.ctpn_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def set_param(self, name, value):
        """One parameter of the detection tail (ctpn_set_param): cfg.TEST.RPN_* / TextLineCfg of the reference, by its name."""
        _check(self._lib.ctpn_set_param(self._h, name.encode(), float(value)))

    def get_param(self, name):
        v = C.c_double(0.0)
        _check(self._lib.ctpn_get_param(self._h, name.encode(), C.byref(v)))
        return v.value

    def reserve_proposals(self, n):
        """ctpn_reserve_proposals: room for RPN_POST_NMS_TOP_N up to n (1000 .. POST_NMS_CAPACITY_MAX) proposals per image."""
        n = int(n)
        if n > POST_NMS_CAPACITY_MAX:
            raise ValueError("proposal capacity %d exceeds the limit of %d (CTPN_POST_NMS_CAPACITY_MAX)" % (n, POST_NMS_CAPACITY_MAX))
        _check(self._lib.ctpn_reserve_proposals(self._h, n))

    @property
    def proposal_capacity(self):
        """ctpn_proposal_capacity: rows per image of the rois / keep / anchor arrays (1000 on a fresh ctx)."""
        v = C.c_int(0)
        _check(self._lib.ctpn_proposal_capacity(self._h, C.byref(v)))
        return v.value

    def forward_sets(self):
        """ctpn_debug_forward_sets: (sets allocated, set of the most recent forward, device bytes of set 1, (set of slot 0's batch in flight or
        None, set of slot 1's))."""
        out = (C.c_longlong * 4)()
        _check(self._lib.ctpn_debug_forward_sets(self._h, out))
        in_flight = tuple(None if v == 255 else v for v in (int(out[3]) & 255, (int(out[3]) >> 8) & 255))
        return int(out[0]), int(out[1]), int(out[2]), in_flight

    def host_threads(self):
        n = C.c_int(0)
        _check(self._lib.ctpn_host_threads(self._h, C.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ctpn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- weights
    def load_weights(self, arena):
        a = _f32(arena).reshape(-1)
        from .weights import WEIGHT_FLOATS
        if a.size != WEIGHT_FLOATS:
            raise ValueError("weight arena must hold %d floats, got %d" % (WEIGHT_FLOATS, a.size))
        _check(self._lib.ctpn_load_weights_host(self._h, _ptr(a, C.c_float)))
        self.arena_weights = a.copy()               # what network_gradients differentiates at
        self.tail_weights = self.arena_weights[-818748:]      # the last ten tensors (tail_grad.TAIL_FLOATS): what tail_gradients differentiates at

    def load_weights_device(self, dev_ptr):
        """ctpn_load_weights_device: the arena from this device's memory. The copy runs on the ctx's stream: synchronise whatever filled the
        buffer first (torch.cuda.synchronize()). Like every weight load: CTPN_ERR_STATE while a submitted batch is uncollected."""
        _check(self._lib.ctpn_load_weights_device(self._h, C.c_void_p(int(dev_ptr))))

    def broadcast_weights_rank(self, unique_id, rank, world, root=0):
        """One process per GPU: collective over RCCL (every rank calls it with the root's comm_unique_id()); the root has its
        weights loaded, every other rank receives the arena into its HBM and packs it (ctpn_broadcast_weights_rank)."""
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % COMM_ID_BYTES)
        _check(self._lib.ctpn_broadcast_weights_rank(self._h, C.c_char_p(bytes(unique_id)), int(rank), int(world), int(root)))

    # ---- forward
    def forward(self, images, device_ptr=None, shape=None):
        """images: (n,h,w,3) uint8 BGR host array, or device_ptr + shape for HBM-resident input."""
        if device_ptr is not None:
            n, h, w = shape
            _check(self._lib.ctpn_forward(self._h, C.c_void_p(int(device_ptr)), 1, int(n), int(h), int(w)))
            return
        im = np.ascontiguousarray(images, dtype=np.uint8)
        if im.ndim == 3:
            im = im[None]
        n, h, w, c = im.shape
        assert c == 3
        self._keepalive = im
        _check(self._lib.ctpn_forward(self._h, im.ctypes.data_as(C.c_void_p), 0, n, h, w))

    @staticmethod
    def _canvas(canvas, heights, device_ptr, shape):
        """-> (pointer, on_device, n, hc, w, heights int32, keepalive) of a ragged batch (ctpn_hip.h, ctpn_forward_ragged)."""
        if device_ptr is not None:
            n, hc, w = shape
            ptr, on_dev, keep = C.c_void_p(int(device_ptr)), 1, None
        else:
            keep = np.ascontiguousarray(canvas, dtype=np.uint8)
            if keep.ndim != 4 or keep.shape[3] != 3:
                raise ValueError("canvas must be (n, hc, w, 3) uint8")
            n, hc, w, _ = keep.shape
            ptr, on_dev = keep.ctypes.data_as(C.c_void_p), 0
        hts = np.ascontiguousarray(heights, dtype=np.int32).reshape(-1)
        if hts.shape[0] != n:
            raise ValueError("one height per image")
        return ptr, on_dev, int(n), int(hc), int(w), hts, keep

    def forward_ragged(self, canvas, heights, device_ptr=None, shape=None):
        """Images of one width and different heights in one forward (ctpn_forward_ragged): canvas (n,hc,w,3) uint8 BGR, image i in rows
        [0, heights[i]) of slot i (lib/utils/blob.py im_list_to_canvas builds one). Tensors come back canvas-shaped."""
        ptr, on_dev, n, hc, w, hts, keep = self._canvas(canvas, heights, device_ptr, shape)
        self._keepalive = (keep, hts)
        _check(self._lib.ctpn_forward_ragged(self._h, ptr, on_dev, n, hc, w, _ptr(hts, C.c_int)))

    def forward_blob(self, blob, device_ptr=None, shape=None):
        """blob: (n,h,w,3) float32 BGR with PIXEL_MEANS already subtracted (the reference's net.data feed)."""
        if device_ptr is not None:
            n, h, w = shape
            _check(self._lib.ctpn_forward_blob(self._h, C.c_void_p(int(device_ptr)), 1, int(n), int(h), int(w)))
            return
        b = np.ascontiguousarray(blob, dtype=np.float32)
        if b.ndim == 3:
            b = b[None]
        n, h, w, c = b.shape
        assert c == 3
        self._keepalive = b
        _check(self._lib.ctpn_forward_blob(self._h, b.ctypes.data_as(C.c_void_p), 0, n, h, w))

    def sync(self):
        _check(self._lib.ctpn_sync(self._h))

    def stream(self):
        s = C.c_void_p()
        _check(self._lib.ctpn_stream(self._h, C.byref(s)))
        return s.value

    def feat_shape(self):
        n, hf, wf = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.ctpn_feat_shape(self._h, C.byref(n), C.byref(hf), C.byref(wf)))
        return n.value, hf.value, wf.value

    def get_tensor(self, name, capacity=None):
        shape = (C.c_int * 4)()
        if capacity is None:
            probe = np.zeros((1,), np.float32)
            rc = self._lib.ctpn_get_tensor(self._h, name.encode(), _ptr(probe, C.c_float), 0, shape)
            if rc not in (CTPN_OK, -4):
                _check(rc)
            capacity = int(np.prod([shape[i] for i in range(4)]))
        out = np.zeros((max(capacity, 1),), np.float32)
        _check(self._lib.ctpn_get_tensor(self._h, name.encode(), _ptr(out, C.c_float), out.size, shape))
        shp = tuple(shape[i] for i in range(4))
        return out[: int(np.prod(shp))].reshape(shp)

    def get_tensor_device(self, name):
        """ctpn_get_tensor_device: get_tensor's tensor, same shape and bytes, as a float32 torch tensor on cuda:device_id -- unpacked by a
        kernel, nothing crosses to the host. The call returns when the tensor is complete."""
        import torch
        shape = (C.c_int * 4)()
        probe = torch.empty((4,), dtype=torch.float32, device=torch.device("cuda", int(self.device_id)))
        rc = self._lib.ctpn_get_tensor_device(self._h, name.encode(), C.c_void_p(probe.data_ptr()), 0, shape)
        if rc not in (CTPN_OK, -4):
            _check(rc)
        shp = tuple(shape[i] for i in range(4))
        out = torch.empty(shp, dtype=torch.float32, device=probe.device)
        if out.numel():
            _check(self._lib.ctpn_get_tensor_device(self._h, name.encode(), C.c_void_p(out.data_ptr()), out.numel(), shape))
        return out

    # ---- proposals
    def _anchors(self, n, post_nms_topn, counts):
        a = np.zeros((n, post_nms_topn), np.int32)
        _check(self._lib.ctpn_proposal_anchors(self._h, _ptr(a, C.c_int), int(post_nms_topn)))
        return [a[i, : counts[i]].copy() for i in range(n)]

    def proposals(self, im_info, pre_nms_topn=12000, post_nms_topn=1000, nms_thresh=0.7, min_size=8.0, want_anchors=False):
        """-> list of rois (R,5) per image; with want_anchors also the anchor index (y*wf + x)*10 + a of every roi."""
        info = _f32(im_info).reshape(-1, 3)
        n = info.shape[0]
        rois = np.zeros((n, post_nms_topn, 5), np.float32)
        counts = np.zeros((n,), np.int32)
        _check(self._lib.ctpn_proposals(self._h, _ptr(info, C.c_float), int(pre_nms_topn), int(post_nms_topn),
                                        float(nms_thresh), float(min_size), _ptr(rois, C.c_float), _ptr(counts, C.c_int)))
        out = [rois[i, : counts[i]].copy() for i in range(n)]
        return (out, self._anchors(n, post_nms_topn, counts)) if want_anchors else out

    def proposal_fetch(self, what, n, hf, wf, pre_nms_topn, post_nms_topn):
        """ctpn_debug_proposal_fetch: intermediate `what` (a PROPOSAL_FETCH name) of the LAST proposals call, whose shapes the caller restates."""
        code, dt, shape = PROPOSAL_FETCH[what]
        per_img = hf * wf * 10
        npad = 1
        while npad < per_img:
            npad <<= 1
        out = np.zeros((n,) + shape(per_img, npad, int(pre_nms_topn), int(post_nms_topn)), dt)
        _check(self._lib.ctpn_debug_proposal_fetch(self._h, code, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def proposals_from_host(self, cls_prob, bbox_pred, im_info, pre_nms_topn=12000, post_nms_topn=1000,
                            nms_thresh=0.7, min_size=8.0, want_anchors=False):
        cp = _f32(cls_prob)
        bp = _f32(bbox_pred)
        n, hf, wf, _ = cp.shape
        info = _f32(im_info).reshape(-1, 3)
        rois = np.zeros((n, post_nms_topn, 5), np.float32)
        counts = np.zeros((n,), np.int32)
        _check(self._lib.ctpn_proposals_from_host(self._h, _ptr(cp, C.c_float), _ptr(bp, C.c_float), n, hf, wf,
                                                  _ptr(info, C.c_float), int(pre_nms_topn), int(post_nms_topn),
                                                  float(nms_thresh), float(min_size), _ptr(rois, C.c_float),
                                                  _ptr(counts, C.c_int)))
        out = [rois[i, : counts[i]].copy() for i in range(n)]
        return (out, self._anchors(n, post_nms_topn, counts)) if want_anchors else out

    def proposals_from_heads(self, heads, im_info, valid_rows=None, pre_nms_topn=12000, post_nms_topn=1000, nms_thresh=0.7, min_size=8.0):
        """ctpn_debug_proposals_from_heads: heads (n, hf, wf, 64) float32, the heads GEMM's rows -> (rois per image, anchors per image,
        cls_prob (n, hf, wf, 20), bbox_pred (n, hf, wf, 40)) of decode_kernel's production branch. valid_rows: n feature-row counts (ragged)."""
        hd = _f32(heads)
        n, hf, wf, ld = hd.shape
        if ld != 64:
            raise ValueError("heads rows hold 64 floats")
        info = _f32(im_info).reshape(-1, 3)
        vr = None if valid_rows is None else np.ascontiguousarray(valid_rows, dtype=np.int32).reshape(-1)
        if info.shape[0] != n or (vr is not None and vr.shape[0] != n):
            raise ValueError("one im_info row (and one valid_rows entry) per image")
        rois = np.zeros((n, post_nms_topn, 5), np.float32)
        counts = np.zeros((n,), np.int32)
        cls = np.zeros((n, hf, wf, 20), np.float32)
        bbox = np.zeros((n, hf, wf, 40), np.float32)
        _check(self._lib.ctpn_debug_proposals_from_heads(self._h, _ptr(hd, C.c_float), n, hf, wf, _ptr(info, C.c_float),
                                                         None if vr is None else _ptr(vr, C.c_int), int(pre_nms_topn), int(post_nms_topn),
                                                         float(nms_thresh), float(min_size), _ptr(rois, C.c_float), _ptr(counts, C.c_int),
                                                         _ptr(cls, C.c_float), _ptr(bbox, C.c_float)))
        return [rois[i, : counts[i]].copy() for i in range(n)], self._anchors(n, post_nms_topn, counts), cls, bbox

    # ---- whole path
    def detect(self, images=None, scales=None, mode="H", line_capacity=512, device_ptr=None, shape=None,
               want_rois=False):
        if device_ptr is not None:
            n, h, w = shape
            ptr, on_dev = C.c_void_p(int(device_ptr)), 1
        else:
            im = np.ascontiguousarray(images, dtype=np.uint8)
            if im.ndim == 3:
                im = im[None]
            n, h, w, _ = im.shape
            self._keepalive = im
            ptr, on_dev = im.ctypes.data_as(C.c_void_p), 0
        sc = _f32(scales if scales is not None else np.ones((n,), np.float32)).reshape(-1)
        recs = np.zeros((n, line_capacity, 9), np.float64)
        lcnt = np.zeros((n,), np.int32)
        rois = np.zeros((n, self.proposal_capacity, 5), np.float32) if want_rois else None
        rcnt = np.zeros((n,), np.int32) if want_rois else None
        m = MODE_O if str(mode).upper().startswith("O") else MODE_H
        _check(self._lib.ctpn_detect(self._h, ptr, on_dev, int(n), int(h), int(w), _ptr(sc, C.c_float), m,
                                     _ptr(recs, C.c_double), int(line_capacity), _ptr(lcnt, C.c_int),
                                     _ptr(rois, C.c_float) if want_rois else None,
                                     _ptr(rcnt, C.c_int) if want_rois else None))
        lines = [recs[i, : lcnt[i]].copy() for i in range(n)]
        if want_rois:
            return lines, [rois[i, : rcnt[i]].copy() for i in range(n)]
        return lines

    def detect_ragged(self, canvas=None, heights=None, scales=None, mode="H", line_capacity=512, device_ptr=None, shape=None, want_rois=False):
        """detect() for a ragged batch (ctpn_detect_ragged): per image what detect() returns for that image alone."""
        ptr, on_dev, n, hc, w, hts, keep = self._canvas(canvas, heights, device_ptr, shape)
        self._keepalive = (keep, hts)
        sc = _f32(scales if scales is not None else np.ones((n,), np.float32)).reshape(-1)
        recs = np.zeros((n, line_capacity, 9), np.float64)
        lcnt = np.zeros((n,), np.int32)
        rois = np.zeros((n, self.proposal_capacity, 5), np.float32) if want_rois else None
        rcnt = np.zeros((n,), np.int32) if want_rois else None
        m = MODE_O if str(mode).upper().startswith("O") else MODE_H
        _check(self._lib.ctpn_detect_ragged(self._h, ptr, on_dev, n, hc, w, _ptr(hts, C.c_int), _ptr(sc, C.c_float), m,
                                            _ptr(recs, C.c_double), int(line_capacity), _ptr(lcnt, C.c_int),
                                            _ptr(rois, C.c_float) if want_rois else None, _ptr(rcnt, C.c_int) if want_rois else None))
        lines = [recs[i, : lcnt[i]].copy() for i in range(n)]
        if want_rois:
            return lines, [rois[i, : rcnt[i]].copy() for i in range(n)]
        return lines

    def debug_text_lines(self, rois, size, scales=None, mode="H", line_capacity=512, roi_counts=None):
        """The text-line tail of detect on caller-supplied rois (ctpn_debug_text_lines): rois is one (R_i, 5) array [score,x1,y1,x2,y2]
        per image in descending score order (roi_counts: use only that many rows of each), size = (im_h, im_w) of every image.
        -> (lines, keeps): per image the (M, 9) records of `mode` and the roi indices the connector's NMS kept. On CTPN_ERR_CAPACITY the
        raised CtpnError carries the true counts as .line_counts."""
        n = len(rois)
        packed = np.zeros((n, self.proposal_capacity, 5), np.float32)
        rcnt = np.zeros((n,), np.int32)
        for i, r in enumerate(rois):
            r = _f32(r).reshape(-1, 5)
            packed[i, : r.shape[0]] = r
            rcnt[i] = r.shape[0] if roi_counts is None else int(roi_counts[i])
        sc = _f32(scales if scales is not None else np.ones((n,), np.float32)).reshape(-1)
        if sc.shape[0] != n:
            raise ValueError("one scale per image")
        recs = np.zeros((n, max(line_capacity, 1), 9), np.float64)
        lcnt = np.zeros((n,), np.int32)
        keep = np.zeros((n, self.proposal_capacity), np.int32)
        kcnt = np.zeros((n,), np.int32)
        m = MODE_O if str(mode).upper().startswith("O") else MODE_H
        try:
            _check(self._lib.ctpn_debug_text_lines(self._h, _ptr(packed, C.c_float), _ptr(rcnt, C.c_int), int(n), int(size[0]), int(size[1]),
                                                   _ptr(sc, C.c_float), m, _ptr(recs, C.c_double), int(line_capacity), _ptr(lcnt, C.c_int),
                                                   _ptr(keep, C.c_int), _ptr(kcnt, C.c_int)))
        except CtpnError as e:
            e.line_counts = lcnt.copy()
            raise
        return [recs[i, : lcnt[i]].copy() for i in range(n)], [keep[i, : kcnt[i]].copy() for i in range(n)]

    def jpeg_entropy_device_stats(self):
        """Of the last device-entropy call (ctpn_jpeg_entropy_device_stats): dict(device=files decoded on the device, host=files handed to
        the host half because of a flag, subsequences=..., rounds=sync rounds run)."""
        out = (C.c_longlong * 4)()
        _check(self._lib.ctpn_jpeg_entropy_device_stats(self._h, out))
        return {"device": int(out[0]), "host": int(out[1]), "subsequences": int(out[2]), "rounds": int(out[3])}

    @staticmethod
    def _entropy_form(entropy):
        if entropy not in ("host", "device"):
            raise ValueError("entropy must be 'host' or 'device'")
        return entropy == "device"

    def decode_jpeg_batch(self, files, h=None, w=None, fx=1.0, fy=1.0, entropy="host"):
        """resize_im(cv2.imread(f)) of n JPEG files of one size on the device (ctpn_decode_jpeg_batch): Huffman decoding on the ctx's host
        pool, IDCT / upsampling / colour conversion / cv2.resize(fx, fy) as HIP kernels. Returns (device pointer, (n, out_h, out_w)) for
        forward / detect / detect_submit (device_ptr=, shape=); the buffer stays valid until the second-next call.
        CtpnError(code CTPN_ERR_UNSUPPORTED) for CMYK / 4:1:1 / arithmetic-coded / incomplete files: decode those on the host.
        entropy="device": the Huffman decode runs on the device too (ctpn_decode_jpeg_batch_device; sequential files only, a progressive
        one is CTPN_ERR_UNSUPPORTED there); the images are byte-equal."""
        fn = self._lib.ctpn_decode_jpeg_batch_device if self._entropy_form(entropy) else self._lib.ctpn_decode_jpeg_batch
        files = list(files)
        if h is None or w is None:
            h, w = jpeg_probe(files[0])[:2]
        keeps = [_bytes_ptr(f) for f in files]
        n = len(keeps)
        ptrs = (C.POINTER(C.c_uint8) * n)(*[k[1] for k in keeps])
        sizes = (C.c_size_t * n)(*[k[2] for k in keeps])
        out, oh, ow = C.c_void_p(0), C.c_int(0), C.c_int(0)
        _check(fn(self._h, ptrs, sizes, n, int(h), int(w), float(fx), float(fy), C.byref(out), C.byref(oh), C.byref(ow)))
        return out.value, (n, oh.value, ow.value)

    def decode_jpeg_files(self, paths, h, w, fx=1.0, fy=1.0, entropy="host"):
        """decode_jpeg_batch from paths (ctpn_decode_jpeg_files / ctpn_decode_jpeg_files_device): the library's worker threads read the
        files themselves."""
        fn = self._lib.ctpn_decode_jpeg_files_device if self._entropy_form(entropy) else self._lib.ctpn_decode_jpeg_files
        paths = list(paths)
        keep, arr = _path_array(paths)
        out, oh, ow = C.c_void_p(0), C.c_int(0), C.c_int(0)
        _check(fn(self._h, arr, len(paths), int(h), int(w), float(fx), float(fy), C.byref(out), C.byref(oh), C.byref(ow)))
        return out.value, (len(paths), oh.value, ow.value)

    def decode_jpeg_ragged(self, files_or_paths, sizes, factors, hc, wc, entropy="host"):
        """JPEG files of mixed sizes, layouts and orientations into one ragged canvas on the device (ctpn_decode_jpeg_batch_ragged /
        ctpn_decode_jpeg_files_ragged). files_or_paths: every item the bytes of a file, or every item a path (str / os.PathLike); sizes: one
        (h, w) per file as jpeg_probe reports it; factors: one resize_im factor per file (<= 0 or 1: no resize); every width must map to wc
        and every height to 16 .. hc. -> ((device pointer, (n, hc, wc)), heights int32): the canvas handle goes to detect_submit(device_ptr=,
        shape=, heights=) / forward_ragged / detect_ragged and to jpeg_batch_fetch; it stays valid until the second-next decode call."""
        on_dev = 1 if self._entropy_form(entropy) else 0
        items = list(files_or_paths)
        n = len(items)
        hw = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(n, 2))
        fh, fw = np.ascontiguousarray(hw[:, 0]), np.ascontiguousarray(hw[:, 1])
        fac = np.ascontiguousarray(np.asarray(factors, np.float64).reshape(n))
        hts = np.zeros((n,), np.int32)
        out = C.c_void_p(0)
        as_paths = [isinstance(it, (str, os.PathLike)) for it in items]
        if n and all(as_paths):
            keep, arr = _path_array(items)
            _check(self._lib.ctpn_decode_jpeg_files_ragged(self._h, arr, n, _ptr(fh, C.c_int), _ptr(fw, C.c_int), _ptr(fac, C.c_double), int(hc), int(wc), on_dev,
                                                           C.byref(out), _ptr(hts, C.c_int)))
        else:
            if any(as_paths):
                raise ValueError("decode_jpeg_ragged wants all files as bytes or all as paths")
            keeps = [_bytes_ptr(f) for f in items]
            ptrs = (C.POINTER(C.c_uint8) * n)(*[k[1] for k in keeps])
            lens = (C.c_size_t * n)(*[k[2] for k in keeps])
            _check(self._lib.ctpn_decode_jpeg_batch_ragged(self._h, ptrs, lens, n, _ptr(fh, C.c_int), _ptr(fw, C.c_int), _ptr(fac, C.c_double), int(hc), int(wc),
                                                           on_dev, C.byref(out), _ptr(hts, C.c_int)))
        return (out.value, (n, int(hc), int(wc))), hts

    def pack_canvas(self, images, factors, hc, wc):
        """Images of mixed sizes -- (h, w, 3) uint8 arrays, or device (pointer, (h, w)[, pitch]) items -- into one ragged canvas on the device
        (ctpn_pack_canvas; see the module's pack_canvas). -> ((device pointer, (n, hc, wc)), heights int32), as decode_jpeg_ragged returns them;
        the canvas stays valid until the second-next decode or pack call."""
        return pack_canvas(self, images, factors, hc, wc)

    def decode_png_ragged(self, paths, shapes, factors, hc, wc):
        """PNG files of mixed sizes into one ragged canvas on the device (ctpn_decode_png_files_ragged; see the module's
        decode_png_files_ragged). -> ((device pointer, (n, hc, wc)), heights int32), as decode_jpeg_ragged returns them."""
        return decode_png_files_ragged(self, paths, shapes, factors, hc, wc)

    def jpeg_batch_fetch(self, device_ptr, shape):
        """The decoded batch as an (n, h, w, 3) uint8 array on the host (ctpn_jpeg_batch_fetch)."""
        n, h, w = shape
        out = np.empty((n, h, w, 3), np.uint8)
        _check(self._lib.ctpn_jpeg_batch_fetch(self._h, C.c_void_p(int(device_ptr)), _ptr(out, C.c_uint8), out.size))
        return out

    def jpeg_encode_device_stats(self):
        """Of the last device-entropy encode (ctpn_jpeg_entropy_encode_device_stats): dict(device=files coded on the device, host=files handed
        to the host half, blocks=blocks coded on the device, d2h_bytes=bytes copied device to host)."""
        out = (C.c_longlong * 4)()
        _check(self._lib.ctpn_jpeg_entropy_encode_device_stats(self._h, out))
        return {"device": int(out[0]), "host": int(out[1]), "blocks": int(out[2]), "d2h_bytes": int(out[3])}

    def encode_jpeg_batch(self, images=None, quality=95, device_ptr=None, shape=None, entropy="host"):
        """cv2.imwrite's JPEG bytes of n BGR uint8 images of one size (ctpn_encode_jpeg_batch): colour conversion, chroma downsampling, DCT
        and quantiser on the device, Huffman coding on the ctx's host pool. images: (n, h, w, 3) on the host, or device_ptr + shape.
        -> list of n bytes objects, byte-equal to Pillow's save(quality=quality, subsampling=2).
        entropy="device": the Huffman coding runs on the device too (ctpn_encode_jpeg_batch_device); the files are byte-equal."""
        fn = self._lib.ctpn_encode_jpeg_batch_device if self._entropy_form(entropy) else self._lib.ctpn_encode_jpeg_batch
        if device_ptr is None:
            images = np.ascontiguousarray(images, dtype=np.uint8)
            if images.ndim != 4 or images.shape[3] != 3:
                raise ValueError("encode_jpeg_batch wants (n,h,w,3) uint8")
            shape, src, on_dev = images.shape, images.ctypes.data_as(C.c_void_p), 0
        else:
            src, on_dev = C.c_void_p(int(device_ptr)), 1
        n, h, w = int(shape[0]), int(shape[1]), int(shape[2])
        bound = jpeg_encode_capacity(h, w)
        sizes = (C.c_size_t * n)()
        for cap in (min(bound, h * w + 4096), bound):      # a byte per pixel holds any photograph; the proven bound is three times the raw image
            bufs = np.empty((n, cap), np.uint8)
            ptrs = (C.c_void_p * n)(*[bufs[i].ctypes.data for i in range(n)])
            caps = (C.c_size_t * n)(*([cap] * n))
            rc = fn(self._h, src, on_dev, n, h, w, int(quality), ptrs, caps, sizes)
            if rc != CTPN_ERR_CAPACITY or cap == bound:
                break
        _check(rc)
        return [bufs[i, : sizes[i]].tobytes() for i in range(n)]

    def write_annotated_files(self, device_ptr, shape, recs, scale, paths, quality=95, entropy="host"):
        """draw_boxes + cv2.resize(1 / scale) + cv2.imwrite (reference ctpn/demo.py:28-52) for a batch of device images
        (ctpn_write_annotated_files): recs = one (M_i, 9) array per image, paths = one JPEG file name per image. The batch is not modified.
        entropy="device": ctpn_write_annotated_files_device, the same files with the Huffman coding on the device."""
        fn = self._lib.ctpn_write_annotated_files_device if self._entropy_form(entropy) else self._lib.ctpn_write_annotated_files
        n, h, w = int(shape[0]), int(shape[1]), int(shape[2])
        recs = [np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 9) for r in recs]
        assert len(recs) == n and len(paths) == n
        cap = max([r.shape[0] for r in recs] + [1])
        packed = np.zeros((n, cap, 9), np.float64)
        counts = np.zeros((n,), np.int32)
        for i, r in enumerate(recs):
            packed[i, : r.shape[0]] = r
            counts[i] = r.shape[0]
        keep, arr = _path_array(list(paths))
        _check(fn(self._h, C.c_void_p(int(device_ptr)), n, h, w, _ptr(packed, C.c_double), cap, _ptr(counts, C.c_int),
                                                    float(scale), arr, int(quality)))

    def write_annotated_files_ragged(self, images=None, device_ptr=None, shape=None, heights=None, recs=(), scales=None, paths=(), quality=95, entropy="host"):
        """write_annotated_files for a RAGGED batch (ctpn_write_annotated_files_ragged): images = the canvas (n, hc, w, 3) on the host, or
        device_ptr + shape = (n, hc, w) -- a live canvas of decode_jpeg_ragged is written from where it lies; heights: image i is rows
        [0, heights[i]) of slot i; recs = one (M_i, 9) array per image; scales: one per image -- image i is resized by 1 / scales[i] into a
        file of its own size. File i is byte-equal to write_annotated_files of that image alone. The canvas is not modified.
        entropy="device": ctpn_write_annotated_files_ragged_device."""
        fn = self._lib.ctpn_write_annotated_files_ragged_device if self._entropy_form(entropy) else self._lib.ctpn_write_annotated_files_ragged
        self._write_annotated_ragged(fn, "write_annotated_files_ragged", images, device_ptr, shape, heights, recs, scales, paths, (int(quality),))

    def _write_annotated_ragged(self, fn, who, images, device_ptr, shape, heights, recs, scales, paths, tail):
        """the ragged annotated writers' common call; tail: what the format's entry point takes behind the paths"""
        if heights is None or scales is None:
            raise ValueError(who + " wants heights and scales")
        ptr, on_dev, n, hc, w, hts, keep = self._canvas(images, heights, device_ptr, shape)
        sc = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
        paths = list(paths)
        if sc.shape[0] != n or len(paths) != n:
            raise ValueError(who + " wants one scale and one path per image")
        packed, counts = _pack_lines(recs, None, n)
        keep_paths, arr = _path_array(paths)
        _check(fn(self._h, ptr, on_dev, n, hc, w, _ptr(hts, C.c_int), _ptr(packed, C.c_double), int(packed.shape[1]), _ptr(counts, C.c_int), _ptr(sc, C.c_double),
                  arr, *tail))

    def write_annotated_png_files_ragged(self, images=None, device_ptr=None, shape=None, heights=None, recs=(), scales=None, paths=()):
        """write_annotated_png_files for a RAGGED batch (ctpn_write_annotated_png_files_ragged): the arguments of write_annotated_files_ragged
        without quality. images = the canvas (n, hc, w, 3) on the host (PNG files are decoded there), or device_ptr + shape. File i is
        byte-equal to write_annotated_png_files of image i alone (rows [0, heights[i]), its lines, its scale). The canvas is not modified."""
        self._write_annotated_ragged(self._lib.ctpn_write_annotated_png_files_ragged, "write_annotated_png_files_ragged", images, device_ptr, shape, heights, recs,
                                     scales, paths, ())

    def png_encode_device_stats(self):
        """Of the last PNG call of this ctx (ctpn_png_encode_device_stats): dict(device=files coded on the device, host=files handed to the
        host form, pieces=256-byte pieces coded on the device, d2h_bytes=bytes copied device to host)."""
        out = (C.c_longlong * 4)()
        _check(self._lib.ctpn_png_encode_device_stats(self._h, out))
        return {"device": int(out[0]), "host": int(out[1]), "pieces": int(out[2]), "d2h_bytes": int(out[3])}

    @staticmethod
    def _image_source(images, device_ptr, shape, who):
        if device_ptr is None:
            images = np.ascontiguousarray(images, dtype=np.uint8)
            if images.ndim != 4 or images.shape[3] != 3:
                raise ValueError(who + " wants (n,h,w,3) uint8")
            return images, images.shape, images.ctypes.data_as(C.c_void_p), 0
        return None, shape, C.c_void_p(int(device_ptr)), 1

    def encode_png_batch(self, images=None, device_ptr=None, shape=None):
        """cv2.imwrite's PNG files of n BGR uint8 images of one size, coded on the device (ctpn_encode_png_batch): Sub filter, histogram,
        length, prefix-sum and write passes over 256-byte pieces of the filtered stream; the code tables and the framing on the ctx's host
        pool. images: (n, h, w, 3) on the host, or device_ptr + shape. -> list of n bytes objects; lossless, byte-equal to png_encode."""
        keep, shape, src, on_dev = self._image_source(images, device_ptr, shape, "encode_png_batch")
        n, h, w = int(shape[0]), int(shape[1]), int(shape[2])
        bound = png_encode_capacity(h, w)
        sizes = (C.c_size_t * n)()
        for cap in (min(bound, h * w * 3 + 4096), bound):      # the raw size holds anything but noise; the proven bound is twice it
            bufs = np.empty((n, cap), np.uint8)
            ptrs = (C.c_void_p * n)(*[bufs[i].ctypes.data for i in range(n)])
            caps = (C.c_size_t * n)(*([cap] * n))
            rc = self._lib.ctpn_encode_png_batch(self._h, src, on_dev, n, h, w, ptrs, caps, sizes)
            if rc != CTPN_ERR_CAPACITY or cap == bound:
                break
        _check(rc)
        return [bufs[i, : sizes[i]].tobytes() for i in range(n)]

    def write_annotated_png_files(self, images=None, device_ptr=None, shape=None, recs=(), scale=1.0, paths=()):
        """draw_boxes + cv2.resize(1 / scale) + cv2.imwrite (reference ctpn/demo.py:28-52) into PNG files, all on the device
        (ctpn_write_annotated_png_files). images: (n, h, w, 3) on the host (a PNG batch is decoded there), or device_ptr + shape (a live batch
        of decode_jpeg_batch); recs = one (M_i, 9) array per image, paths = one file name per image. The batch is not modified."""
        keep, shape, src, on_dev = self._image_source(images, device_ptr, shape, "write_annotated_png_files")
        n, h, w = int(shape[0]), int(shape[1]), int(shape[2])
        recs = [np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 9) for r in recs]
        assert len(recs) == n and len(paths) == n
        cap = max([r.shape[0] for r in recs] + [1])
        packed = np.zeros((n, cap, 9), np.float64)
        counts = np.zeros((n,), np.int32)
        for i, r in enumerate(recs):
            packed[i, : r.shape[0]] = r
            counts[i] = r.shape[0]
        keep_paths, arr = _path_array(list(paths))
        _check(self._lib.ctpn_write_annotated_png_files(self._h, src, on_dev, n, h, w, _ptr(packed, C.c_double), cap, _ptr(counts, C.c_int),
                                                        float(scale), arr))

    @staticmethod
    def _ragged_heights(heights, n):
        """heights= of crop_lines / write_line_crops -> the extra argument of the *_ragged call: () for a uniform batch"""
        if heights is None:
            return None, ()
        hts = np.ascontiguousarray(heights, dtype=np.int32).reshape(-1)
        if hts.shape[0] != n:
            raise ValueError("one height per image")
        return hts, (_ptr(hts, C.c_int),)

    def crop_lines(self, images=None, recs=(), line_counts=None, crop_h=32, max_w=512, pad_value=0, device_ptr=None, shape=None,
                   out_device_ptr=None, out_capacity=0, heights=None):
        """One rectified crop of height crop_h per text line, cut out on the device (ctpn_crop_lines). images: (n, h, w, 3) uint8 on the host,
        or device_ptr + shape = (n, h, w) -- a live batch of decode_jpeg_batch is cropped where it lies, without a fetch. recs: one (M_i, 9)
        array per image as detect / detect_collect return them, or an (n, capacity, 9) array with line_counts. -> (crops, widths): crops
        (total, crop_h, max_w, 3) BGR uint8, lines in image order, columns >= widths[k] of crop k filled with pad_value (a longer line is
        squeezed to max_w). With out_device_ptr (4-byte aligned, out_capacity bytes) the crops stay in device memory and crops is None.
        heights: the batch is a ragged canvas (n, hc, w) -- image i is rows [0, heights[i]) of slot i (ctpn_crop_lines_ragged): the crops
        are those of every image alone, and a line that hangs below its image reads the image's last row, never a canvas row."""
        if device_ptr is None:
            images = np.ascontiguousarray(images, dtype=np.uint8)
            if images.ndim == 3:
                images = images[None]
            if images.ndim != 4 or images.shape[3] != 3:
                raise ValueError("crop_lines wants (n,h,w,3) uint8")
            shape, src, on_dev = images.shape, images.ctypes.data_as(C.c_void_p), 0
        else:
            src, on_dev = C.c_void_p(int(device_ptr)), 1
        n, h, w = int(shape[0]), int(shape[1]), int(shape[2])
        packed, counts = _pack_lines(recs, line_counts, n)
        widths = np.zeros((max(int(counts.sum()), 1),), np.int32)
        total = C.c_int(0)
        hts, hts_arg = self._ragged_heights(heights, n)
        fn = self._lib.ctpn_crop_lines if hts is None else self._lib.ctpn_crop_lines_ragged

        def call(out, out_on_dev, capacity):
            _check(fn(self._h, src, on_dev, n, h, w, *hts_arg, _ptr(packed, C.c_double), int(packed.shape[1]), _ptr(counts, C.c_int), int(crop_h),
                      int(max_w), int(pad_value), out, out_on_dev, capacity, _ptr(widths, C.c_int), C.byref(total)))
        if out_device_ptr is not None:
            call(C.c_void_p(int(out_device_ptr)), 1, int(out_capacity))
            return None, widths[: total.value].copy()
        call(None, 0, 0)                                   # sizes the call: the widths and the total, on the host
        crops = np.empty((total.value, int(crop_h), int(max_w), 3), np.uint8)
        if total.value:
            call(crops.ctypes.data_as(C.c_void_p), 0, crops.size)
        return crops, widths[: total.value].copy()

    def write_line_crops(self, images=None, recs=(), line_counts=None, crop_h=32, max_w=512, pad_value=0, device_ptr=None, shape=None, paths=None,
                         quality=95, entropy="host", heights=None, format="jpg"):
        """crop_lines with the crops written as JPEG files where they are cut (ctpn_write_line_crops): crop k, crop_h x widths[k], goes to
        paths[k] at `quality` -- image 0's lines first, then image 1's, ... --, byte-equal to Pillow's save(quality=quality, subsampling=2) of
        crop_lines' crops[k, :, :widths[k]]. No crop visits the host. paths=None sizes the call. -> widths (int32, one per line).
        entropy="device": ctpn_write_line_crops_device, the same files with the Huffman coding on the device.
        heights: the batch is a ragged canvas, as in crop_lines (ctpn_write_line_crops_ragged / ctpn_write_line_crops_ragged_device).
        format="png": lossless PNG files (ctpn_write_line_crops_png / ctpn_write_line_crops_png_ragged), file k byte-equal to png_encode of
        crops[k, :, :widths[k]]; no quality, and no entropy="device" (ValueError)."""
        if format not in ("jpg", "png"):
            raise ValueError("format must be 'jpg' or 'png'")
        dev = self._entropy_form(entropy)
        if format == "png":
            if dev:
                raise ValueError("format='png' has no entropy='device' form")
            fn = self._lib.ctpn_write_line_crops_png if heights is None else self._lib.ctpn_write_line_crops_png_ragged
        elif heights is None:
            fn = self._lib.ctpn_write_line_crops_device if dev else self._lib.ctpn_write_line_crops
        else:
            fn = self._lib.ctpn_write_line_crops_ragged_device if dev else self._lib.ctpn_write_line_crops_ragged
        if device_ptr is None:
            images = np.ascontiguousarray(images, dtype=np.uint8)
            if images.ndim == 3:
                images = images[None]
            if images.ndim != 4 or images.shape[3] != 3:
                raise ValueError("write_line_crops wants (n,h,w,3) uint8")
            shape, src, on_dev = images.shape, images.ctypes.data_as(C.c_void_p), 0
        else:
            src, on_dev = C.c_void_p(int(device_ptr)), 1
        n, h, w = int(shape[0]), int(shape[1]), int(shape[2])
        packed, counts = _pack_lines(recs, line_counts, n)
        lines = int(counts.sum())
        widths = np.zeros((max(lines, 1),), np.int32)
        total = C.c_int(0)
        arr = None
        if paths is not None:
            paths = list(paths)
            if len(paths) != lines:
                raise ValueError("write_line_crops wants one path per line")
            keep, arr = _path_array(paths)
        hts, hts_arg = self._ragged_heights(heights, n)
        _check(fn(self._h, src, on_dev, n, h, w, *hts_arg, _ptr(packed, C.c_double), int(packed.shape[1]), _ptr(counts, C.c_int), int(crop_h), int(max_w),
                  int(pad_value), *(() if format == "png" else (int(quality),)), arr, _ptr(widths, C.c_int), C.byref(total)))
        return widths[: total.value].copy()

    def encode_png_mixed(self, images=None, device_ptr=None, heights=None, widths=None, pitches=None, offsets=None):
        """PNG files of n BGR uint8 images of ANY mix of sizes in one call (ctpn_encode_png_mixed). images: a list of (h_i, w_i, 3) arrays
        (packed into one source buffer, image after image at pitch 3 w), or device_ptr with the tables heights / widths / pitches (bytes,
        >= 3 w) / offsets (bytes into the buffer). -> list of n bytes objects, each byte-equal to png_encode of that image; lossless."""
        if device_ptr is None:
            images = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
            if any(im.ndim != 3 or im.shape[2] != 3 for im in images):
                raise ValueError("encode_png_mixed wants a list of (h,w,3) uint8 images")
            heights = [im.shape[0] for im in images]
            widths = [im.shape[1] for im in images]
            pitches = [3 * w for w in widths]
            offsets = [int(v) for v in np.cumsum([0] + [im.size for im in images])[:-1]]
            source = np.concatenate([im.reshape(-1) for im in images]) if images else np.zeros((1,), np.uint8)
            src, on_dev, nbytes = source.ctypes.data_as(C.c_void_p), 0, source.size
        else:
            src, on_dev, nbytes = C.c_void_p(int(device_ptr)), 1, 0
        ht = np.ascontiguousarray(heights, dtype=np.int32).reshape(-1)
        wd = np.ascontiguousarray(widths, dtype=np.int32).reshape(-1)
        n = int(ht.shape[0])
        if wd.shape[0] != n or len(pitches) != n or len(offsets) != n:
            raise ValueError("encode_png_mixed wants one height, width, pitch and offset per image")
        pt = (C.c_size_t * max(n, 1))(*[int(v) for v in pitches])
        of = (C.c_size_t * max(n, 1))(*[int(v) for v in offsets])
        bounds = [png_encode_capacity(int(h), int(w)) for h, w in zip(ht, wd)]
        sizes = (C.c_size_t * max(n, 1))()
        rc = CTPN_OK
        # first a little above the raw size: noise codes at just over 8 bits per byte, and ONE file above its buffer repeats the whole call;
        # then the proven bound, twice the raw size
        for proven in (False, True):
            want = [b if proven else min(b, int(h) * int(w) * 3 * 65 // 64 + 4096) for b, h, w in zip(bounds, ht, wd)]
            bufs = [np.empty((cap,), np.uint8) for cap in want]
            ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
            caps = (C.c_size_t * max(n, 1))(*want)
            rc = self._lib.ctpn_encode_png_mixed(self._h, src, on_dev, nbytes, n, _ptr(ht, C.c_int), _ptr(wd, C.c_int), pt, of, ptrs, caps, sizes)
            if rc != CTPN_ERR_CAPACITY:
                break
        _check(rc)
        return [bufs[i][: sizes[i]].tobytes() for i in range(n)]

    def encode_jpeg_mixed(self, images=None, quality=95, entropy="host", device_ptr=None, heights=None, widths=None, pitches=None, offsets=None):
        """JPEG files of n BGR uint8 images of ANY mix of sizes in one call (ctpn_encode_jpeg_mixed). images: a list of (h_i, w_i, 3) arrays
        (packed into one source buffer, rows 4-byte aligned), or device_ptr with the tables heights / widths / pitches (bytes, >= 3 w) /
        offsets (bytes into the buffer). -> list of n bytes objects, each byte-equal to encode_jpeg_batch of that image alone and to
        Pillow's save(quality=quality, subsampling=2). entropy="device": ctpn_encode_jpeg_mixed_device."""
        fn = self._lib.ctpn_encode_jpeg_mixed_device if self._entropy_form(entropy) else self._lib.ctpn_encode_jpeg_mixed
        if device_ptr is None:
            images = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
            if any(im.ndim != 3 or im.shape[2] != 3 for im in images):
                raise ValueError("encode_jpeg_mixed wants a list of (h,w,3) uint8 images")
            heights = [im.shape[0] for im in images]
            widths = [im.shape[1] for im in images]
            pitches = [(3 * w + 3) & ~3 for w in widths]
            offsets, at = [], 0
            for h, p in zip(heights, pitches):
                offsets.append(at)
                at += h * p
            source = np.zeros((max(at, 1),), np.uint8)
            for im, p, o in zip(images, pitches, offsets):
                h, w = im.shape[:2]
                source[o: o + h * p].reshape(h, p)[:, : 3 * w] = im.reshape(h, 3 * w)
            src, on_dev, nbytes = source.ctypes.data_as(C.c_void_p), 0, source.size
        else:
            src, on_dev, nbytes = C.c_void_p(int(device_ptr)), 1, 0
        ht = np.ascontiguousarray(heights, dtype=np.int32).reshape(-1)
        wd = np.ascontiguousarray(widths, dtype=np.int32).reshape(-1)
        n = int(ht.shape[0])
        if wd.shape[0] != n or len(pitches) != n or len(offsets) != n:
            raise ValueError("encode_jpeg_mixed wants one height, width, pitch and offset per image")
        pt = (C.c_size_t * max(n, 1))(*[int(v) for v in pitches])
        of = (C.c_size_t * max(n, 1))(*[int(v) for v in offsets])
        bounds = [jpeg_encode_capacity(int(h), int(w)) for h, w in zip(ht, wd)]
        sizes = (C.c_size_t * max(n, 1))()
        rc = CTPN_OK
        for proven in (False, True):      # a byte per pixel holds any photograph; the proven bound is three times the raw image
            want = [b if proven else min(b, int(h) * int(w) + 4096) for b, h, w in zip(bounds, ht, wd)]
            bufs = [np.empty((cap,), np.uint8) for cap in want]
            ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
            caps = (C.c_size_t * max(n, 1))(*want)
            rc = fn(self._h, src, on_dev, nbytes, n, _ptr(ht, C.c_int), _ptr(wd, C.c_int), pt, of, int(quality), ptrs, caps, sizes)
            if rc != CTPN_ERR_CAPACITY:
                break
        _check(rc)
        return [bufs[i][: sizes[i]].tobytes() for i in range(n)]

    def detect_submit(self, images=None, slot=0, scales=None, device_ptr=None, shape=None, heights=None):
        """Asynchronous detect, part 1 (ctpn_detect_submit). Returns immediately. heights: the batch is ragged -- images is a canvas
        (ctpn_detect_submit_ragged; see forward_ragged)."""
        if heights is not None:
            ptr, on_dev, n, hc, w, hts, keep = self._canvas(images, heights, device_ptr, shape)
            self._keep_slot = getattr(self, "_keep_slot", {})
            self._keep_slot[slot] = (keep, hts)
            sc = _f32(scales if scales is not None else np.ones((n,), np.float32)).reshape(-1)
            _check(self._lib.ctpn_detect_submit_ragged(self._h, ptr, on_dev, n, hc, w, _ptr(hts, C.c_int), _ptr(sc, C.c_float), int(slot)))
            self._slot_n = getattr(self, "_slot_n", {})
            self._slot_n[slot] = n
            return
        if device_ptr is not None:
            n, h, w = shape
            ptr, on_dev = C.c_void_p(int(device_ptr)), 1
        else:
            im = np.ascontiguousarray(images, dtype=np.uint8)
            if im.ndim == 3:
                im = im[None]
            n, h, w, _ = im.shape
            self._keep_slot = getattr(self, "_keep_slot", {})
            self._keep_slot[slot] = im
            ptr, on_dev = im.ctypes.data_as(C.c_void_p), 0
        sc = _f32(scales if scales is not None else np.ones((n,), np.float32)).reshape(-1)
        _check(self._lib.ctpn_detect_submit(self._h, ptr, on_dev, int(n), int(h), int(w), _ptr(sc, C.c_float), int(slot)))
        self._slot_n = getattr(self, "_slot_n", {})
        self._slot_n[slot] = n

    def detect_collect(self, slot=0, mode="H", line_capacity=512, want_rois=False):
        """Asynchronous detect, part 2 (ctpn_detect_collect): waits for the slot and returns its text lines."""
        n = self._slot_n[slot]
        recs = np.zeros((n, line_capacity, 9), np.float64)
        lcnt = np.zeros((n,), np.int32)
        rois = np.zeros((n, self.proposal_capacity, 5), np.float32) if want_rois else None
        rcnt = np.zeros((n,), np.int32) if want_rois else None
        m = MODE_O if str(mode).upper().startswith("O") else MODE_H
        _check(self._lib.ctpn_detect_collect(self._h, int(slot), m, _ptr(recs, C.c_double), int(line_capacity), _ptr(lcnt, C.c_int),
                                             _ptr(rois, C.c_float) if want_rois else None, _ptr(rcnt, C.c_int) if want_rois else None))
        lines = [recs[i, : lcnt[i]].copy() for i in range(n)]
        if want_rois:
            return lines, [rois[i, : rcnt[i]].copy() for i in range(n)]
        return lines

    ragged_valid_rows = staticmethod(ragged_valid_rows)

    # ---- measurement
    def profile_enable(self, on=True):
        """on: False / True (an event pair around every stage) / 2 (ONE pair around the 13 conv3x3 launches of a forward)."""
        _check(self._lib.ctpn_profile_enable(self._h, 2 if on == 2 else (1 if on else 0)))

    def profile_reset(self):
        _check(self._lib.ctpn_profile_reset(self._h))

    def profile_read(self):
        out = {}
        for k, name in enumerate(KIND_NAMES):
            ms, n, work = C.c_double(), C.c_longlong(), C.c_double()
            _check(self._lib.ctpn_profile_read(self._h, k, C.byref(ms), C.byref(n), C.byref(work)))
            out[name] = {"ms": ms.value, "launches": n.value, "work": work.value}
        return out
