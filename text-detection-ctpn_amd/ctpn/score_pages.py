"""`python ctpn/score_pages.py IMAGES LABELS` -- how good is this model on my labelled pages: the numbers ctpn/train_net.py logs for a step
(rpn_cross_entropy, rpn_loss_box, model_loss), for every image of a directory, one JSON line each.

IMAGES holds *.jpg / *.png files, LABELS one <stem>.txt (or gt_<stem>.txt) per image in the format lib/prepare_training_data/split_label.py:108-117
writes: `text`, x1, y1, x2, y2, tab-separated, one 16-px strip per line, in the image file's pixel coordinates. Every image is resized as the
demo resizes it (resize_im), the boxes are scaled by the same factor, and ctpn_amd.score_pages runs the forward, the anchor targets and the
loss on the GPU. Subsampling is off by default (RPN_BATCHSIZE 0: every labelled anchor counts, the result does not depend on a seed);
--sample turns text.yml's RPN_BATCHSIZE back on. Weights as in ctpn/demo.py (--synthetic SEED for the seeded random-init weights).
"""
from __future__ import print_function

import argparse
import glob
import json
import os
import sys

import numpy as np

_PKG_PARENT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG_PARENT not in sys.path:
    sys.path.insert(0, _PKG_PARENT)

import ctpn_amd  # noqa: E402


def read_labels(path):
    """A label file -> (G, 4) float32 boxes x1, y1, x2, y2. Blank lines are skipped; a line that is not `text` and four numbers is an error
    that names the file and the line."""
    boxes = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            parts = line.rstrip("\r\n").split("\t")
            try:
                if len(parts) != 5:
                    raise ValueError
                boxes.append([float(v) for v in parts[1:]])
            except ValueError:
                raise ValueError("%s:%d: expected `text<TAB>x1<TAB>y1<TAB>x2<TAB>y2`, got %r" % (path, no, line.rstrip("\r\n")))
    return np.array(boxes, np.float32).reshape(-1, 4)


def label_path(labels_dir, image_path):
    stem = os.path.splitext(os.path.basename(image_path))[0]
    for name in (stem + ".txt", "gt_" + stem + ".txt"):
        p = os.path.join(labels_dir, name)
        if os.path.exists(p):
            return p
    return None


def scale_boxes(boxes, factor):
    """the image's resize_im factor applied to its label boxes"""
    return (np.asarray(boxes, np.float32).reshape(-1, 4) * np.float32(factor)).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("images")
    ap.add_argument("labels")
    ap.add_argument("--root", default=os.getcwd(), help="directory holding ctpn/text.yml and checkpoints/")
    ap.add_argument("--synthetic", type=int, default=None, metavar="SEED")
    ap.add_argument("--precision", default=None, help="fp32 | bf16 | fp16 | split (default: cfg.TEST.PRECISION)")
    ap.add_argument("--seed", type=int, default=0, help="subsampling seed (with --sample)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--no-sample", dest="sample", action="store_false", help="RPN_BATCHSIZE 0 (the default)")
    g.add_argument("--sample", dest="sample", action="store_true", help="subsample to the library's RPN_BATCHSIZE")
    ap.set_defaults(sample=False)
    args = ap.parse_args(argv)
    from ctpn_amd.ctpn import demo as D
    from ctpn_amd.lib.fast_rcnn.config import cfg, cfg_from_file
    from ctpn_amd.lib.networks.factory import get_network
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg
    from ctpn_amd.lib.utils import image as imutil
    images, labels = os.path.abspath(args.images), os.path.abspath(args.labels)
    os.chdir(args.root)
    yml = "ctpn/text.yml" if os.path.exists("ctpn/text.yml") else os.path.join(os.path.dirname(os.path.abspath(__file__)), "text.yml")
    cfg_from_file(yml)
    if args.precision:
        cfg.TEST.PRECISION = args.precision
    net = get_network("VGGnet_test")
    D.load_weights(net, args.synthetic)
    tcfg = ctpn_amd.target_config_default()
    if not args.sample:
        tcfg[4] = 0.0
    names = sorted(glob.glob(os.path.join(images, "*.png")) + glob.glob(os.path.join(images, "*.jpg")))
    for name in names:
        lp = label_path(labels, name)
        if lp is None:
            print(json.dumps({"image": os.path.basename(name), "error": "no label file"}))
            continue
        img, f = D.resize_im(imutil.imread(name), scale=TextLineCfg.SCALE, max_scale=TextLineCfg.MAX_SCALE)
        net.ensure_capacity(1, img.shape[0], img.shape[1])
        r = ctpn_amd.score_pages(net.ctx, img[None], [scale_boxes(read_labels(lp), f)], cfg=tcfg, seed=args.seed)[0]
        r["image"], r["scale"] = os.path.basename(name), f
        print(json.dumps(r))


if __name__ == "__main__":
    main()
