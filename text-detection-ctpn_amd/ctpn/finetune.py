"""`python ctpn/finetune.py IMAGES LABELS --steps N [--from LAYER] [--lr LR] [--momentum M] [--out ARENA.npy] [--synthetic SEED]` -- adapt the
network to labelled pages, one page per step, one JSON line per step: every tensor of the arena from LAYER on (default conv1_1: all 17 893 244
floats; `--from rpn_conv/3x3` trains that conv and the tail).

It is ctpn/finetune_tail.py's loop over ctpn_amd.network_gradients: the `Momentum` branch of lib/fast_rcnn/train.py:94-109,
tf.clip_by_global_norm(grads, 10.0), then tf.train.MomentumOptimizer with TRAIN.LEARNING_RATE and TRAIN.MOMENTUM of lib/fast_rcnn/config.py, on
the flat vector of the trained tensors. The gradient comes from the GPU (forward with stored activations, anchor targets, RPN loss, the
backward pass through the tail and the conv stack), the update is a few numpy lines on the host, and the weights go back with
ctpn_load_weights_host between steps. The ctx runs with keep_acts = 1. Not built, and not done here: Adam and RMSProp, weight decay (the loss
is model_loss, not total_loss), the learning-rate schedule and the data layers (no shuffling, no augmentation: page k % pages at step k).
IMAGES and LABELS as in ctpn/score_pages.py.
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
from ctpn_amd.conv_grad import CONVS  # noqa: E402
from ctpn_amd.tail_grad import momentum_step  # noqa: E402

CLIP_NORM = 10.0      # lib/fast_rcnn/train.py:108


def trained_offset(from_layer):
    """the arena offset of from_layer's weights: arena[offset:] is what the loop trains (the manifest is in network order)"""
    for name, _, off in ctpn_amd.MANIFEST:
        if name == from_layer + "/weights":
            return off
    raise ValueError("--from is one of " + ", ".join(CONVS))


def run_steps(ctx_for, arena, pages, steps, lr, momentum, cfg=None, seed=0, emit=None, from_layer="conv1_1"):
    """`steps` updates of arena[trained_offset(from_layer):] (a copy; the caller's arena is not written). pages: [(image (h, w, 3) uint8, boxes
    (G, 4))]; ctx_for(h, w) -> a Context with keep_acts = 1 that takes one h x w image, whose weights this function reloads from the arena
    before every step. emit(record) is called once per step with {"step", "page", "model_loss", "rpn_cross_entropy", "rpn_loss_box",
    "grad_norm"}: the loss BEFORE that step's update. -> (the new arena, the records)"""
    arena = np.array(arena, np.float32).reshape(-1)
    first = trained_offset(from_layer)
    names = [name for name, _, off in ctpn_amd.MANIFEST if off >= first]
    velocity = np.zeros((arena.size - first,), np.float32)
    records = []
    for k in range(int(steps)):
        img, boxes = pages[k % len(pages)]
        ctx = ctx_for(int(img.shape[0]), int(img.shape[1]))
        ctx.load_weights(arena)
        losses, grads = ctpn_amd.network_gradients(ctx, img[None], [boxes], cfg=cfg, seed=seed + k, from_layer=from_layer)
        g = np.concatenate([grads[name].reshape(-1) for name in names])
        arena[first:], velocity, norm = momentum_step(arena[first:], velocity, g, lr, momentum, CLIP_NORM)
        rec = {"step": k, "page": k % len(pages), "model_loss": losses[0]["model_loss"], "rpn_cross_entropy": losses[0]["rpn_cross_entropy"],
               "rpn_loss_box": losses[0]["rpn_loss_box"], "grad_norm": norm}
        records.append(rec)
        if emit:
            emit(rec)
    return arena, records


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("images")
    ap.add_argument("labels")
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--from", dest="from_layer", default="conv1_1", metavar="LAYER", help="the first conv trained: conv1_1 (default) .. rpn_conv/3x3")
    ap.add_argument("--lr", type=float, default=None, help="default: cfg.TRAIN.LEARNING_RATE")
    ap.add_argument("--momentum", type=float, default=None, help="default: cfg.TRAIN.MOMENTUM")
    ap.add_argument("--out", default=None, metavar="ARENA.npy", help="write the fine-tuned weight arena (float32, ctpn_amd.WEIGHT_FLOATS) here")
    ap.add_argument("--root", default=os.getcwd(), help="directory holding ctpn/text.yml and checkpoints/")
    ap.add_argument("--synthetic", type=int, default=None, metavar="SEED")
    ap.add_argument("--precision", default="fp32", help="fp32 (default: the gradient is exact for it) | bf16 | fp16 | split: straight-through at the rounded activations")
    ap.add_argument("--seed", type=int, default=0, help="subsampling seed (with --sample)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--no-sample", dest="sample", action="store_false", help="RPN_BATCHSIZE 0 (the default)")
    g.add_argument("--sample", dest="sample", action="store_true", help="subsample to the library's RPN_BATCHSIZE")
    ap.set_defaults(sample=False)
    args = ap.parse_args(argv)
    trained_offset(args.from_layer)
    from ctpn_amd.ctpn import demo as D
    from ctpn_amd.ctpn.score_pages import label_path, read_labels, scale_boxes
    from ctpn_amd.lib.fast_rcnn.config import cfg, cfg_from_file
    from ctpn_amd.lib.networks.factory import get_network
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg
    from ctpn_amd.lib.utils import image as imutil
    images, labels = os.path.abspath(args.images), os.path.abspath(args.labels)
    out = None if args.out is None else os.path.abspath(args.out)
    os.chdir(args.root)
    yml = "ctpn/text.yml" if os.path.exists("ctpn/text.yml") else os.path.join(os.path.dirname(os.path.abspath(__file__)), "text.yml")
    cfg_from_file(yml)
    cfg.TEST.PRECISION = args.precision
    net = get_network("VGGnet_test")
    D.load_weights(net, args.synthetic)
    arena = net._arena      # the host arena every loader of the network class ends in (load_arena)
    tcfg = ctpn_amd.target_config_default()
    if not args.sample:
        tcfg[4] = 0.0
    pages = []
    for name in sorted(glob.glob(os.path.join(images, "*.png")) + glob.glob(os.path.join(images, "*.jpg"))):
        lp = label_path(labels, name)
        if lp is None:
            print(json.dumps({"image": os.path.basename(name), "error": "no label file"}))
            continue
        img, f = D.resize_im(imutil.imread(name), scale=TextLineCfg.SCALE, max_scale=TextLineCfg.MAX_SCALE)
        pages.append((img, scale_boxes(read_labels(lp), f)))
    if not pages:
        raise SystemExit("finetune: no labelled image under %s" % images)

    def ctx_for(h, w):
        net.ensure_capacity(1, h, w)
        if net.ctx.get_option("keep_acts") != 1:
            net.ctx.set_option("keep_acts", 1)      # this program's own ctx: network_gradients needs every activation stored
        return net.ctx

    lr = cfg.TRAIN.LEARNING_RATE if args.lr is None else args.lr
    momentum = cfg.TRAIN.MOMENTUM if args.momentum is None else args.momentum
    arena, _ = run_steps(ctx_for, arena, pages, args.steps, lr, momentum, tcfg, args.seed, emit=lambda r: print(json.dumps(r)),
                         from_layer=args.from_layer)
    if out:
        np.save(out, arena)


if __name__ == "__main__":
    main()
