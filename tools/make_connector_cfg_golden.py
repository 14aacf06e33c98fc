"""Writes tests/golden/connector_cfg_cases.npz: the reference's own TextDetector (lib/text_connector/detectors.py, imported unmodified
behind oracle/make_golden.py's import shim, py_cpu_nms path) on the generated scenes of tests/tail_scenes.py with its TextLineCfg edited
to three of that module's configurations -- what tests/test_tail_params.py pins the host connector and the patched oracle to. The
scenes' tied scores are made distinct first (row i loses i * 1e-6: the order stays, the ties go): the reference sorts with numpy's
unstable argsort, so on tied scores its own result depends on the sort's internals, which is nothing a fixture can pin. The inputs as
fed are part of the file. Needs the reference tree, so it runs where the fixtures are authored; the file it writes is committed.

    python tools/make_connector_cfg_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import make_golden as G  # noqa: E402
import tail_scenes as T  # noqa: E402

CONFIG_NAMES = ("nms_0.4", "gap_20", "all")


def main():
    G.install_shim()
    from lib.fast_rcnn.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(G.REF, "ctpn", "text.yml"))
    from lib.fast_rcnn import nms_wrapper
    from lib.text_connector.detectors import TextDetector
    from lib.text_connector.text_connect_cfg import Config as TextLineCfg
    assert nms_wrapper.pure_python_nms, "expected the reference's py_cpu_nms path"
    out = {"config_names": np.array(CONFIG_NAMES), "cfg8_names": np.array(T.CFG8_NAMES), "size": np.array([T.H, T.W], np.int32)}
    scenes = []
    for sc in T.scenes():
        rois = sc.rois.copy()
        rois[:, 0] -= np.arange(rois.shape[0], dtype=np.float32) * np.float32(1e-6)
        assert np.all(rois[:-1, 0] > rois[1:, 0])
        scenes.append(sc._replace(rois=rois))
        out["rois_" + sc.name] = rois
    for name in CONFIG_NAMES:
        out["cfg8_" + name] = T.cfg8(T.CONFIGS[name])
        with T.patched(TextLineCfg, T.CONFIGS[name]):
            for sc in scenes:
                for mode in "HO":
                    cfg.TEST.DETECT_MODE = mode
                    recs = TextDetector().detect(sc.rois[:, 1:5].copy(), sc.rois[:, 0:1].copy(), (sc.h, sc.w))
                    out["recs_%s_%s_%s" % (name, sc.name, mode)] = np.asarray(recs, np.float64).reshape(-1, 9)
    path = os.path.join(ROOT, "tests", "golden", "connector_cfg_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
