"""`bbox_overlaps(boxes, query_boxes)` and `bbox_intersections(boxes, query_boxes)`: the signatures of the reference's compiled Cython module
(lib/utils/bbox.pyx:15-93), which lib/rpn_msr/anchor_target_layer_tf.py:5 imports. Both take float64 (N, 4) and (K, 4) arrays and return
(N, K) float64, computed on the GPU by the C-ABI `ctpn_bbox_overlaps` and bit-equal to the reference's arithmetic."""
from ... import targets as _t


def bbox_overlaps(boxes, query_boxes):
    return _t.bbox_overlaps(boxes, query_boxes)


def bbox_intersections(boxes, query_boxes):
    return _t.bbox_intersections(boxes, query_boxes)
