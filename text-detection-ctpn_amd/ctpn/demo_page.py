"""Pages larger than the network input: a file or a folder of scans in, `res_<stem>.txt` (+ annotated images) out, every page detected at
its own resolution as overlapping tiles (ctpn_amd.detect_page; include/ctpn_hip.h, "pages in tiles") instead of being shrunk to 600 px by
resize_im -- an A4 scan at 300 dpi keeps its 6 - 8 pt print above CTPN's smallest anchor.

  * the ctx is sized once, for `--batch` tiles of `--tile H W` (rounded down to multiples of 16); a page of any size up to 16384 x 16384
    goes through it in chunks, software-pipelined over the ctx's two slots;
  * --factor f resizes the page first (ctpn_resize, on the GPU); res_<stem>.txt is written in the coordinates of the FILE
    (ctpn_write_result_file divides by f, as demo.py does by its scale);
  * --annotate writes the page with the lines' outlines next to it (ctpn_draw_boxes, then the usual writer);
  * --overlap: pixels two neighbouring tiles share, a multiple of 32; choose it >= the tallest text expected (times f).

    python -m ctpn_amd.ctpn.demo_page --input scans/ --out data/results [--factor 0.5] [--mode O] [--annotate] [--synthetic 0]
"""
from __future__ import print_function

import argparse
import os
import sys
import time

import numpy as np

_PKG_PARENT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG_PARENT not in sys.path:
    sys.path.insert(0, _PKG_PARENT)

import ctpn_amd  # noqa: E402
from ctpn_amd import _binding as B  # noqa: E402
from ctpn_amd.ctpn import demo as D  # noqa: E402
from ctpn_amd.ctpn.demo_batch import list_images  # noqa: E402
from ctpn_amd.lib.networks.VGGnet_test import VGGnet_test  # noqa: E402
from ctpn_amd.lib.fast_rcnn.config import cfg_from_file  # noqa: E402
from ctpn_amd.lib.utils import image as imutil  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input", required=True, help="an image file or a folder of *.png | *.jpg | *.jpeg | *.bmp")
    ap.add_argument("--out", default="data/results")
    ap.add_argument("--factor", type=float, default=1.0, help="resize the page by this factor first (ctpn_resize)")
    ap.add_argument("--tile", type=int, nargs=2, default=(608, 912), metavar=("H", "W"))
    ap.add_argument("--batch", type=int, default=32, help="tiles per forward (the ctx's max_batch)")
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--mode", default="H", choices=["H", "O"])
    ap.add_argument("--nms-form", type=int, default=None, choices=[0, 1], help="the page tail's NMS: 0 ctpn_nms, 1 ctpn_page_nms (default: the library's)")
    ap.add_argument("--precision", default=None, help="fp32 | bf16 | fp16 | split (default: cfg.TEST.PRECISION)")
    ap.add_argument("--annotate", action="store_true", help="also write the page with the lines drawn in")
    ap.add_argument("--synthetic", type=int, default=None, metavar="SEED")
    ap.add_argument("--root", default=os.getcwd(), help="directory holding ctpn/text.yml and checkpoints/")
    return ap


def page_names(path):
    return [path] if os.path.isfile(path) else list_images(path)


def run_page(ctx, name, out_dir, factor=1.0, overlap=128, mode="H", nms_form=None, annotate=False):
    """one file -> res_<stem>.txt (and the annotated page); returns (PageResult, seconds)"""
    t0 = time.time()
    page = imutil.imread(name)
    if factor != 1.0:
        page = B.resize_linear(page, factor, factor, device_id=ctx.device_id)
    res = ctpn_amd.detect_page(ctx, page, overlap=overlap, mode=mode, nms_form=nms_form)
    base = os.path.basename(name)
    B.write_result_file(os.path.join(out_dir, "res_{}.txt".format(base.split(".")[0])), res.lines, factor)
    if annotate:
        img = np.ascontiguousarray(page, dtype=np.uint8)
        B.draw_boxes(img, res.lines)
        if factor != 1.0:
            img = imutil.resize_bilinear(img, fx=1.0 / factor, fy=1.0 / factor)
        imutil.imwrite(os.path.join(out_dir, base), img)
    return res, time.time() - t0


def main(argv=None):
    args = build_parser().parse_args(argv)
    names = page_names(os.path.abspath(args.input))
    out_dir = os.path.abspath(args.out)
    os.chdir(args.root)
    yml = "ctpn/text.yml" if os.path.exists("ctpn/text.yml") else os.path.join(os.path.dirname(os.path.abspath(__file__)), "text.yml")
    cfg_from_file(yml)
    if not os.path.isdir(out_dir):
        os.makedirs(out_dir)
    net = VGGnet_test(max_batch=args.batch, max_h=args.tile[0], max_w=args.tile[1], precision=args.precision)
    D.load_weights(net, args.synthetic)
    ctx = net.ctx
    for name in names:
        res, secs = run_page(ctx, name, out_dir, factor=args.factor, overlap=args.overlap, mode=args.mode, nms_form=args.nms_form, annotate=args.annotate)
        print("{:s}: {:d} x {:d} tiles, {:d} proposals, {:d} lines, {:.3f}s".format(name, res.grid[0], res.grid[1], len(res.boxes), len(res.lines), secs))
    net.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
