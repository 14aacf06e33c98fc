"""`python ctpn/train_net.py IMAGES LABELS --steps N [--solver Momentum|Adam|RMS] [--lr LR] [--weight-decay WD] [--from LAYER] [--cfg YML]
[--snapshot-iters K] [--restore SNAPSHOT.npz] [--out PREFIX] [--synthetic SEED] [--data-layer [--no-flip] [--shuffle-seed S] [--no-prefetch]]` -- the
reference's ctpn/train_net.py on the device: one page per step, one JSON line per step (ctpn_amd.train.RECORD_FIELDS and the page).

It is lib/fast_rcnn/train.py's loop over ctpn_amd.Trainer: the gradient of total_loss (model_loss plus TRAIN.WEIGHT_DECAY's L2 terms),
tf.clip_by_global_norm(grads, 10.0), then the optimiser TRAIN.SOLVER names with TRAIN.LEARNING_RATE (and TRAIN.MOMENTUM), the learning-rate
schedule of TRAIN.STEPSIZE / TRAIN.GAMMA (which only Momentum follows, as in the reference), a snapshot every TRAIN.SNAPSHOT_ITERS steps.
Activations, gradients, the optimiser's state and the weights stay on the device from step to step. The defaults are cfg.TRAIN's; --cfg reads
a yml on top of ctpn/text.yml (the reference's own ctpn/text.yml selects Adam, 1e-5, 5e-4). --out PREFIX writes PREFIX_iter_K.npz snapshots
and PREFIX.npy, the final arena; --restore continues from a snapshot (its solver and settings win).

Without --data-layer, IMAGES and LABELS are as in ctpn/score_pages.py -- labels already cut into 16-px strips, pages of one size -- and step k
visits page k % pages. With --data-layer the run is the reference's from an ICDAR-style folder on: LABELS holds gt_<stem>.txt / <stem>.txt
files of `x1,y1,x2,y2,x3,y3,x4,y4[,...]` lines (further comma fields are ignored, as lib/prepare_training_data/split_label.py:37 does), the
pages may resize to any mix of sizes, and ctpn_amd.DataLayer serves them in RoIDataLayer's shuffled order with the mirrored copies of
TRAIN.USE_FLIPPED (--no-flip: without them; --shuffle-seed: default cfg.RNG_SEED; --no-prefetch: the next file is not decoded ahead). The
JSON line then also carries page, flipped, h and w. A restored run starts the layer's order from its beginning.
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
from ctpn_amd.solver import SOLVERS, solver_defaults  # noqa: E402


def solver_settings(train_cfg, solver=None, lr=None, weight_decay=None):
    """cfg.TRAIN and the command line's overrides -> (solver name, hyper8, weight decay, stepsize, gamma, snapshot iters)"""
    name = train_cfg.SOLVER if solver is None else solver
    if name not in SOLVERS:
        raise SystemExit("train_net: TRAIN.SOLVER is one of " + ", ".join(SOLVERS))
    hyper = solver_defaults(name)
    hyper[0] = train_cfg.LEARNING_RATE if lr is None else lr
    if name == "Momentum":
        hyper[1] = train_cfg.MOMENTUM
    wd = train_cfg.WEIGHT_DECAY if weight_decay is None else weight_decay
    return name, hyper, float(wd), int(train_cfg.STEPSIZE), float(train_cfg.GAMMA), int(train_cfg.SNAPSHOT_ITERS)


def run(trainer, pages, steps, seed=0, emit=None, snapshot_iters=0, out=None):
    """`steps` Trainer steps, page k % pages at iteration k (counted from the trainer's own iteration, so a restored run goes on where it
    stopped) -> the records; a snapshot OUT_iter_K.npz after every snapshot_iters-th iteration"""
    records = []
    for _ in range(int(steps)):
        k = trainer.iter
        img, boxes = pages[k % len(pages)]
        rec = trainer.step(img[None], [boxes], seed=seed + k)
        rec["page"] = k % len(pages)
        records.append(rec)
        if emit:
            emit(rec)
        if out and snapshot_iters > 0 and trainer.iter % snapshot_iters == 0:
            trainer.snapshot("%s_iter_%d.npz" % (out, trainer.iter))
    return records


def run_layer(trainer, layer, steps, seed=0, emit=None, snapshot_iters=0, out=None):
    """run() over a DataLayer: `steps` Trainer.step_record steps on the layer's records; the records gain page, flipped, h and w"""
    records = []
    for _ in range(int(steps)):
        k = trainer.iter
        page = layer.next()
        rec = trainer.step_record(page, seed=seed + k)
        rec["page"], rec["flipped"], rec["h"], rec["w"] = page.page, page.flipped, page.hw[0], page.hw[1]
        records.append(rec)
        if emit:
            emit(rec)
        if out and snapshot_iters > 0 and trainer.iter % snapshot_iters == 0:
            trainer.snapshot("%s_iter_%d.npz" % (out, trainer.iter))
    return records


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("images")
    ap.add_argument("labels")
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--solver", default=None, choices=sorted(SOLVERS), help="default: cfg.TRAIN.SOLVER")
    ap.add_argument("--lr", type=float, default=None, help="default: cfg.TRAIN.LEARNING_RATE")
    ap.add_argument("--momentum", type=float, default=None, help="Momentum's momentum; default: cfg.TRAIN.MOMENTUM")
    ap.add_argument("--weight-decay", type=float, default=None, help="default: cfg.TRAIN.WEIGHT_DECAY")
    ap.add_argument("--from", dest="from_layer", default="conv1_1", metavar="LAYER", help="the first conv trained: conv1_1 (default) .. rpn_conv/3x3")
    ap.add_argument("--cfg", default=None, metavar="YML", help="a yml read on top of ctpn/text.yml, e.g. the reference's ctpn/text.yml")
    ap.add_argument("--snapshot-iters", type=int, default=None, help="default: cfg.TRAIN.SNAPSHOT_ITERS; 0: none")
    ap.add_argument("--restore", default=None, metavar="SNAPSHOT.npz")
    ap.add_argument("--out", default=None, metavar="PREFIX", help="PREFIX_iter_K.npz snapshots and PREFIX.npy, the final arena")
    ap.add_argument("--root", default=os.getcwd(), help="directory holding ctpn/text.yml and checkpoints/")
    ap.add_argument("--synthetic", type=int, default=None, metavar="SEED")
    ap.add_argument("--seed", type=int, default=0, help="subsampling seed (with --sample)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--no-sample", dest="sample", action="store_false", help="RPN_BATCHSIZE 0 (the default)")
    g.add_argument("--sample", dest="sample", action="store_true", help="subsample to the library's RPN_BATCHSIZE")
    ap.set_defaults(sample=False)
    ap.add_argument("--data-layer", action="store_true", help="LABELS holds quadrilaterals; shuffle, mirror and mix sizes as the reference's data layer does")
    ap.add_argument("--no-flip", dest="flip", action="store_false", help="with --data-layer: no mirrored copies (TRAIN.USE_FLIPPED off)")
    ap.add_argument("--shuffle-seed", type=int, default=None, metavar="S", help="with --data-layer: the order's seed; default: cfg.RNG_SEED")
    ap.add_argument("--no-prefetch", dest="prefetch", action="store_false", help="with --data-layer: decode each file when its step comes")
    args = ap.parse_args(argv)
    if args.from_layer not in CONVS:
        raise SystemExit("train_net: --from is one of " + ", ".join(CONVS))
    from ctpn_amd.ctpn import demo as D
    from ctpn_amd.ctpn.score_pages import label_path, read_labels, scale_boxes
    from ctpn_amd.lib.fast_rcnn.config import cfg, cfg_from_file
    from ctpn_amd.lib.networks.factory import get_network
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg
    from ctpn_amd.lib.utils import image as imutil
    images, labels = os.path.abspath(args.images), os.path.abspath(args.labels)
    out = None if args.out is None else os.path.abspath(args.out)
    extra = None if args.cfg is None else os.path.abspath(args.cfg)
    restore = None if args.restore is None else os.path.abspath(args.restore)
    os.chdir(args.root)
    yml = "ctpn/text.yml" if os.path.exists("ctpn/text.yml") else os.path.join(os.path.dirname(os.path.abspath(__file__)), "text.yml")
    cfg_from_file(yml)
    if extra:
        cfg_from_file(extra)
    cfg.TEST.PRECISION = "fp32"      # the gradient is exact for the fp32 network
    name, hyper, wd, stepsize, gamma, snap = solver_settings(cfg.TRAIN, args.solver, args.lr, args.weight_decay)
    if args.momentum is not None and name == "Momentum":
        hyper[1] = args.momentum
    if args.snapshot_iters is not None:
        snap = args.snapshot_iters
    net = get_network("VGGnet_test")
    D.load_weights(net, args.synthetic)
    tcfg = ctpn_amd.target_config_default()
    if not args.sample:
        tcfg[4] = 0.0
    emit = lambda r: print(json.dumps(r))      # noqa: E731
    make_trainer = lambda: (ctpn_amd.Trainer.restore(net.ctx, restore) if restore else      # noqa: E731
                            ctpn_amd.Trainer(net.ctx, net._arena, name, hyper, wd, args.from_layer, stepsize, gamma, tcfg))
    fnames = sorted(glob.glob(os.path.join(images, "*.png")) + glob.glob(os.path.join(images, "*.jpg")))
    if args.data_layer:
        from ctpn_amd.data_layer import quad_label_path, read_quads
        paths, quads = [], []
        for fname in fnames:
            lp = quad_label_path(labels, fname)
            if lp is None:
                print(json.dumps({"image": os.path.basename(fname), "error": "no label file"}))
                continue
            paths.append(fname)
            quads.append(read_quads(lp))
        if not paths:
            raise SystemExit("train_net: no labelled image under %s" % images)
        with ctpn_amd.DataLayer(net.device_id, paths, quads, flipped=args.flip and bool(cfg.TRAIN.USE_FLIPPED),
                                seed=cfg.RNG_SEED if args.shuffle_seed is None else args.shuffle_seed, scales=cfg.TRAIN.SCALES, max_size=cfg.TRAIN.MAX_SIZE,
                                prefetch=args.prefetch, label_scale=TextLineCfg.SCALE, label_max_size=TextLineCfg.MAX_SCALE) as layer:
            h, w = layer.max_shape()      # the ctx's capacity: the largest page; every forward takes its own page's size
            net.ensure_capacity(1, int(h), int(w))
            if net.ctx.get_option("keep_acts") != 1:
                net.ctx.set_option("keep_acts", 1)
            trainer = make_trainer()
            run_layer(trainer, layer, args.steps, args.seed, emit=emit, snapshot_iters=snap, out=out)
        if out:
            np.save(out + ".npy", trainer.arena())
        return
    pages = []
    for fname in fnames:
        lp = label_path(labels, fname)
        if lp is None:
            print(json.dumps({"image": os.path.basename(fname), "error": "no label file"}))
            continue
        img, f = D.resize_im(imutil.imread(fname), scale=TextLineCfg.SCALE, max_scale=TextLineCfg.MAX_SCALE)
        pages.append((img, scale_boxes(read_labels(lp), f)))
    if not pages:
        raise SystemExit("train_net: no labelled image under %s" % images)
    shapes = set(p[0].shape[:2] for p in pages)
    if len(shapes) != 1:
        raise SystemExit("train_net: the pages resize to %d different sizes; one size per run" % len(shapes))
    h, w = pages[0][0].shape[:2]
    net.ensure_capacity(1, int(h), int(w))
    if net.ctx.get_option("keep_acts") != 1:
        net.ctx.set_option("keep_acts", 1)      # this program's own ctx: the gradient needs every activation stored
    trainer = make_trainer()
    run(trainer, pages, args.steps, args.seed, emit=emit, snapshot_iters=snap, out=out)
    if out:
        np.save(out + ".npy", trainer.arena())


if __name__ == "__main__":
    main()
