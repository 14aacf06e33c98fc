"""`anchor_target_layer(rpn_cls_score, gt_boxes, gt_ishard, dontcare_areas, im_info, _feat_stride, anchor_scales)`: the reference's signature
and return shapes (lib/rpn_msr/anchor_target_layer_tf.py:10-276) over the C-ABI `ctpn_anchor_targets`, for a batch of one. Settings come from
cfg.TRAIN as in the reference (a key cfg.TRAIN does not hold takes lib/fast_rcnn/config.py's default). The subsampling seed is drawn from
numpy's global generator, so np.random.seed repeats a run; the sampled set is this library's rule (include/ctpn_hip.h), not npr.choice's."""
import numpy as np

from ..fast_rcnn.config import cfg
from ... import targets as _t

_KEYS = ("RPN_NEGATIVE_OVERLAP", "RPN_POSITIVE_OVERLAP", "RPN_CLOBBER_POSITIVES", "RPN_FG_FRACTION", "RPN_BATCHSIZE", "DONTCARE_AREA_INTERSECTION_HI",
         "PRECLUDE_HARD_SAMPLES")
_CONFIG_PY = (0.3, 0.7, 0.0, 0.5, 256.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0)      # lib/fast_rcnn/config.py:112-139


def train_cfg12():
    t = cfg.TRAIN
    c = np.array(_CONFIG_PY, np.float64)
    for i, k in enumerate(_KEYS):
        if k in t:
            c[i] = float(t[k])
    if "RPN_BBOX_INSIDE_WEIGHTS" in t:
        c[7:11] = [float(v) for v in t["RPN_BBOX_INSIDE_WEIGHTS"]]
    if "RPN_POSITIVE_WEIGHT" in t:
        c[11] = float(t["RPN_POSITIVE_WEIGHT"])
    return c


def anchor_target_layer(rpn_cls_score, gt_boxes, gt_ishard, dontcare_areas, im_info, _feat_stride=[16, ], anchor_scales=[16, ]):
    assert rpn_cls_score.shape[0] == 1, 'Only single item batches are supported'
    assert list(_feat_stride) == [16] and list(anchor_scales) == [16], 'the anchors are generate_anchors(scales=[16]) on a 16-px grid'
    height, width = (int(v) for v in rpn_cls_score.shape[1:3])
    hard = None if gt_ishard is None or np.asarray(gt_ishard).shape[0] == 0 else [np.asarray(gt_ishard).reshape(-1).astype(np.int32)]
    dc = None if dontcare_areas is None or np.asarray(dontcare_areas).shape[0] == 0 else [np.asarray(dontcare_areas, np.float32).reshape(-1, 4)]
    seed = int(np.random.randint(0, 2 ** 31 - 1))
    t = _t.anchor_targets(height, width, np.asarray(im_info, np.float32).reshape(-1, 3)[:1], [np.asarray(gt_boxes, np.float32).reshape(-1, 5)], hard, dc,
                          train_cfg12(), seed, int(cfg.GPU_ID))
    return t.labels, t.bbox_targets, t.inside_weights, t.outside_weights
