#!/usr/bin/env python
"""Writes tests/golden/data_layer.npz: inputs and recorded results of the reference's label splitter and data-layer order, which
tests/test_data_layer.py and tests/test_gpu_data_layer.py hold the restatement (tests/data_layer_ref.py) and the kernels against.

    python tools/make_data_layer_golden.py --reference /path/to/text-detection-ctpn [--out tests/golden/data_layer.npz]

Nothing of the reference is copied into this repository: its lib/prepare_training_data/split_label.py is read from the reference tree at
run time, its two path constants are replaced in a temporary copy outside the repository, and the copy is run there with a stand-in `cv2`
module (imread: zeros of the recorded size; resize: zeros of the round-half-even size; imwrite: nothing) -- the script uses cv2 for the
sizes alone. What is recorded: the label text of about 40 quadrilaterals over five page sizes and the strips label_tmp/ holds for them.
The pages: 600 x 1024 (factor 1, and a width that is a power of two, so a label's x is the strip rule's xmin / xmax exactly: every row of
the quirk table in include/ctpn_hip_data_layer.h is there), 900 x 1400, 500 x 1500 (the 1200 cap decides the factor), 375 x 500 (enlarged) and
1200 x 12 (factor 1 by the cap; a strip that ends beyond a page 12 wide). xmin == xmax is left out: the reference stops there.

The order: the reference's RoIDataLayer imported from the reference tree with stand-ins for three modules it imports and the order never touches (cv2, easydict
and the compiled lib.utils.bbox, which need not be installed where this runs); the first 40 indices of _get_next_minibatch_inds after
np.random.seed(3) for roidb lengths 1, 2, 3 and 8 with IMS_PER_BATCH 1."""
import argparse
import contextlib
import io
import os
import re
import runpy
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (stem, file h, file w)
PAGES = [("page_a", 600, 1024), ("page_b", 900, 1400), ("page_c", 500, 1500), ("page_d", 375, 500), ("page_e", 1200, 12)]


def rect(x1, x2, y1=100, y2=140, tail=""):
    return "%s,%s,%s,%s,%s,%s,%s,%s%s" % (x1, y1, x2, y1, x2, y2, x1, y2, tail)


def label_text():
    """stem -> the label file's text"""
    a = [rect(5, 100), rect(3, 17), rect(16, 33), rect(31, 48), rect(3, 10), rect(3, 15), rect(3, 16), rect(16, 32), rect(15, 16),
         rect(0, 1023, 0, 599), rect(100, 1500, 580, 700, ",Latin,Hello, World"), rect(-40, 37, -20, 30), rect(47, 64), rect(47, 65), rect(15, 33),
         # tied x in the middle of the order, the two points given in both orders; ties at both ends; all four tied in pairs with crossed y
         "10,100,50,80,50,140,90,110", "10,100,50,140,50,80,90,110", "90,110,50,140,10,100,50,80", "50,80,50,140,50,100,90,110",
         "200,300,200,340,200,320,260,310", "300,50,300,90,340,90,340,50,###",
         # outside the page: left of it (xmax < xmin after the clamps), right of it (xmin is not clamped), above and below
         "-90,10,-60,12,-58,40,-95,44", "1100,10,1180,12,1190,40,1090,44", "400,-80,470,-90,480,-20,395,-10", "400,620,470,610,480,690,395,700",
         # whole numbers at which v / 600 * 600 in double falls just below v: dividing first gives 54 and 96, multiplying first 55 and 97
         rect(200, 280, 55, 97)]
    rs = np.random.RandomState(20)
    out = {"page_a": a, "page_e": [rect(3, 9, 20, 90), rect(6, 11.5, 1000, 1300)]}
    for stem, h, w in PAGES[1:4]:
        lines = []
        for k in range(6):
            x0, y0 = rs.uniform(-0.05 * w, 0.9 * w), rs.uniform(-0.05 * h, 0.9 * h)
            bw, bh = rs.uniform(20, 0.4 * w), rs.uniform(8, 60)
            pts = np.array([[x0, y0], [x0 + bw, y0 + rs.uniform(-6, 6)], [x0 + bw + rs.uniform(-6, 6), y0 + bh], [x0 + rs.uniform(-6, 6), y0 + bh + rs.uniform(-6, 6)]])
            pts = np.roll(pts, k % 4, axis=0)
            fmt = "%.2f" if k % 2 else "%d"
            lines.append(",".join(fmt % v for v in pts.reshape(-1)) + (",Text" if k % 3 == 0 else ""))
        if stem == "page_c":      # likewise 275 / 1500 * 1200 and 395 / 1500 * 1200: 219 and 315, not 220 and 316
            lines.append(rect(275, 395, 100, 130))
        out[stem] = lines
    return {k: "".join(ln + "\n" for ln in v) for k, v in out.items()}


def fake_cv2(sizes, resized):
    """the stand-in: sizes[stem] = (h, w) of imread's zeros; resized[stem] = the size resize gave, in call order"""
    m = types.ModuleType("cv2")
    m.INTER_LINEAR = 1
    state = {}

    def imread(path):
        stem = os.path.splitext(os.path.basename(path))[0]
        state["stem"] = stem
        h, w = sizes[stem]
        return np.zeros((h, w, 3), np.uint8)

    def resize(img, dsize, dst=None, fx=0.0, fy=0.0, interpolation=1):
        h, w = img.shape[:2]
        oh, ow = int(np.rint(np.float64(h) * np.float64(fy))), int(np.rint(np.float64(w) * np.float64(fx)))
        resized[state["stem"]] = (oh, ow, float(fx))
        return np.zeros((oh, ow, 3), np.uint8)

    m.imread, m.resize, m.imwrite = imread, resize, lambda path, img: True
    return m


def run_split_label(reference, texts):
    src = open(os.path.join(reference, "lib", "prepare_training_data", "split_label.py")).read()
    tmp = tempfile.mkdtemp(prefix="data_layer_golden_")
    try:
        img_dir, gt_dir = os.path.join(tmp, "image"), os.path.join(tmp, "label")
        os.makedirs(img_dir)
        os.makedirs(gt_dir)
        # the copy differs from the reference's file in its two path constants alone
        src, n1 = re.subn(r"(?m)^path = .*$", lambda m: "path = %r" % img_dir, src, count=1)
        src, n2 = re.subn(r"(?m)^gt_path = .*$", lambda m: "gt_path = %r" % gt_dir, src, count=1)
        assert n1 == 1 and n2 == 1
        script = os.path.join(tmp, "split_label_copy.py")
        with open(script, "w") as f:
            f.write(src)
        for stem, h, w in PAGES:
            open(os.path.join(img_dir, stem + ".jpg"), "wb").close()
            with open(os.path.join(gt_dir, "gt_" + stem + ".txt"), "w") as f:
                f.write(texts[stem])
        resized = {}
        saved_cv2, cwd = sys.modules.get("cv2"), os.getcwd()
        sys.modules["cv2"] = fake_cv2({stem: (h, w) for stem, h, w in PAGES}, resized)
        os.chdir(tmp)
        try:
            with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):      # the script prints every file's path
                warnings.simplefilter("ignore", DeprecationWarning)
                runpy.run_path(script, run_name="__main__")
        finally:
            os.chdir(cwd)
            if saved_cv2 is None:
                del sys.modules["cv2"]
            else:
                sys.modules["cv2"] = saved_cv2
        strips = {}
        for stem, _, _ in PAGES:
            rows = []
            p = os.path.join(tmp, "label_tmp", stem + ".txt")
            if os.path.exists(p):
                for line in open(p):
                    parts = line.rstrip("\n").split("\t")
                    assert parts[0] == "text" and len(parts) == 5
                    rows.append([int(v) for v in parts[1:]])
            strips[stem] = np.array(rows, np.int32).reshape(-1, 4)
        return strips, resized
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


class _EasyDict(dict):
    """easydict.EasyDict's behaviour as far as the reference's config.py uses it"""

    def __init__(self, d=None, **kw):
        super(_EasyDict, self).__init__()
        for k, v in dict(d or {}, **kw).items():
            setattr(self, k, v)

    def __setattr__(self, k, v):
        if isinstance(v, dict) and not isinstance(v, _EasyDict):
            v = _EasyDict(v)
        self[k] = v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def run_layer_order(reference, lengths, count, seed):
    """-> {length: indices} from the reference's RoIDataLayer, or None and the reason where it cannot be imported here"""
    stand_ins = {"cv2": types.ModuleType("cv2"), "easydict": types.ModuleType("easydict"), "lib.utils.bbox": types.ModuleType("lib.utils.bbox")}
    stand_ins["easydict"].EasyDict = _EasyDict
    stand_ins["lib.utils.bbox"].bbox_overlaps = None
    saved = {k: sys.modules.get(k) for k in stand_ins}
    mine = [k for k in sys.modules if k == "lib" or k.startswith("lib.")]
    if mine:
        return None, "a package named lib is already imported"
    sys.modules.update(stand_ins)
    sys.path.insert(0, reference)
    try:
        try:
            from lib.fast_rcnn.config import cfg
            from lib.roi_data_layer.layer import RoIDataLayer
        except Exception as e:
            return None, "%s: %s" % (type(e).__name__, e)
        cfg.TRAIN.HAS_RPN, cfg.TRAIN.IMS_PER_BATCH = True, 1
        out = {}
        for n in lengths:
            np.random.seed(seed)
            layer = RoIDataLayer([{} for _ in range(n)], 2)
            out[n] = np.array([int(layer._get_next_minibatch_inds()[0]) for _ in range(count)], np.int32)
        return out, None
    finally:
        sys.path.remove(reference)
        for k in [k for k in sys.modules if k == "lib" or k.startswith("lib.")]:
            del sys.modules[k]
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="the reference tree (eragonruan/text-detection-ctpn)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "data_layer.npz"))
    args = ap.parse_args()
    reference = os.path.abspath(args.reference)
    texts = label_text()
    strips, resized = run_split_label(reference, texts)
    data = {"stems": np.array([p[0] for p in PAGES]), "numpy_version": np.array(np.__version__)}
    data["page_dims"] = np.array([[h, w, resized[stem][0], resized[stem][1]] for stem, h, w in PAGES], np.int32)
    data["factors"] = np.array([resized[stem][2] for stem, _, _ in PAGES], np.float64)
    for stem, _, _ in PAGES:
        data["text_" + stem] = np.array(texts[stem])
        data["strips_" + stem] = strips[stem]
    order, why = run_layer_order(reference, (1, 2, 3, 8), 40, 3)
    data["order_from_reference"] = np.array(order is not None)
    if order is None:
        print("RoIDataLayer could not be imported (%s): the order is NOT recorded" % why)
    else:
        for n, inds in order.items():
            data["order_%d" % n] = inds
    np.savez_compressed(args.out, **data)
    print("%s: %d pages, %d quads, %d strips, order %s, %d bytes" % (
        args.out, len(PAGES), sum(t.count("\n") for t in texts.values()), sum(s.shape[0] for s in strips.values()),
        "recorded" if order is not None else "not recorded", os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
