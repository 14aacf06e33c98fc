"""MI355X-native CTPN inference hot path (drop-in for eragonruan/text-detection-ctpn's demo path).

Layout mirrors the reference tree for the modules on the hot path:
  ctpn/demo.py, lib/fast_rcnn/{config,test,nms_wrapper,bbox_transform}.py, lib/rpn_msr/*, lib/utils/*,
  lib/networks/*, lib/text_connector/*  -- Python host code over the C ABI of libctpn_hip.so (include/ctpn_hip.h).
There is no CPU fallback: importing works without a GPU (so the build and the host logic can be checked),
but every compute entry point raises CtpnError when the HIP library or a gfx950 device is missing.
"""
from ._binding import CtpnError, lib_path, load_library, Context  # noqa: F401
from .weights import MANIFEST, WEIGHT_FLOATS, make_synthetic_arena, arena_views  # noqa: F401
from .page import detect_page, PageResult  # noqa: F401
from .targets import (target_config_default, bbox_overlaps, bbox_intersections, anchor_targets, rpn_loss, score_pages,  # noqa: F401
                      AnchorTargets, RpnLoss)
from .tail_grad import (tail_forward, tail_backward, tail_views, tail_gradients, momentum_step, TailForward, TailBackward,  # noqa: F401
                        TAIL_FLOATS, TAIL_OFFSET)
from .conv_grad import conv_backward, pool_backward, conv_backward_plan, network_gradients, ConvBackward  # noqa: F401
from .solver import solver_plan, solver_defaults, solver_step, decay_table  # noqa: F401
from .train import network_gradients_device, Trainer  # noqa: F401
from .data_layer import split_labels, split_label_dims, train_page, train_boxes, DataLayer  # noqa: F401

__all__ = ["CtpnError", "lib_path", "load_library", "Context", "MANIFEST", "WEIGHT_FLOATS",
           "make_synthetic_arena", "arena_views", "detect_page", "PageResult",
           "target_config_default", "bbox_overlaps", "bbox_intersections", "anchor_targets", "rpn_loss", "score_pages", "AnchorTargets", "RpnLoss",
           "tail_forward", "tail_backward", "tail_views", "tail_gradients", "momentum_step", "TailForward", "TailBackward", "TAIL_FLOATS", "TAIL_OFFSET",
           "conv_backward", "pool_backward", "conv_backward_plan", "network_gradients", "ConvBackward",
           "solver_plan", "solver_defaults", "solver_step", "decay_table", "network_gradients_device", "Trainer",
           "split_labels", "split_label_dims", "train_page", "train_boxes", "DataLayer"]
