"""Generator of tests/golden/dense_pages.npz: what the reference's OWN proposal_layer and TextDetector return for the dense pages of
tests/dense_pages.py with cfg.TEST.RPN_POST_NMS_TOP_N = 4096 -- the run-time knob of the reference (lib/rpn_msr/proposal_layer_tf.py:55,
lib/fast_rcnn/config.py:180) this library follows through ctpn_reserve_proposals. The reference is imported unmodified, the way
oracle/make_golden.py imports it (its shim: stand-ins for easydict, cv2, tensorflow and the training-only Cython extension). Runs on the
CPU, in the authoring container only (the reference does not travel with the repository); the file it writes is committed.

The file holds OUTPUTS only -- per page rois (R, 5) float32 and recs_H / recs_O (M, 9) float64 -- the inputs are the seeded recipe.

    python tools/make_dense_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import make_golden as G  # noqa: E402
import dense_pages as D  # noqa: E402

PAGES = ("24x48", "40x64")
POST = 4096


def main():
    G.install_shim()
    from lib.fast_rcnn.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(G.REF, "ctpn", "text.yml"))
    from lib.rpn_msr.proposal_layer_tf import proposal_layer
    from lib.fast_rcnn import nms_wrapper
    from lib.text_connector.detectors import TextDetector
    assert nms_wrapper.pure_python_nms, "expected the reference's py_cpu_nms path"
    cfg.TEST.RPN_POST_NMS_TOP_N = POST
    out = {"post_nms_topn": np.int32(POST)}
    for name in PAGES:
        p = D.PAGES[name]
        cls, box, info = D.page(name)
        blob, _ = proposal_layer(cls.copy(), box.copy(), info.reshape(1, 3).copy(), "TEST", _feat_stride=[16, ], anchor_scales=[16, ])
        out["rois_" + name] = np.asarray(blob, np.float32)
        scores, boxes = blob[:, 0], blob[:, 1:5] / info[2]
        for mode in ("H", "O"):
            cfg.TEST.DETECT_MODE = mode
            recs = TextDetector().detect(boxes.copy(), scores[:, np.newaxis].copy(), (16 * p.hf, 16 * p.wf))
            out["recs_%s_%s" % (mode, name)] = np.asarray(recs, np.float64)
        print(name, "rois", blob.shape, "H", out["recs_H_" + name].shape, "O", out["recs_O_" + name].shape)
    path = os.path.join(ROOT, "tests", "golden", "dense_pages.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
