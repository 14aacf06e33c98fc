#!/usr/bin/env python3
"""Regenerates tests/golden/anchor_targets.npz from the reference's UNMODIFIED anchor_target_layer (lib/rpn_msr/anchor_target_layer_tf.py of a
reference checkout; its compiled lib.utils.bbox is replaced by the functions below, which follow bbox.pyx's loops in plain numpy float64, a
query box at a time).

    python tools/make_anchor_target_golden.py [--ref /path/to/text-detection-ctpn]

Every scene runs twice: with text.yml's RPN_BATCHSIZE (300) under np.random.seed(s) -- the reference's sampled labels and weights --, and with
RPN_BATCHSIZE = 10**9, which gives the reference's labels before sampling. Stored per scene: the inputs, labels as int8, weights and targets
as float32; for the largest map a SHA-256 of the target bytes in place of the array. Also stored: the reference's TRAIN settings as
ctpn_target_config_default orders them."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _pairs(boxes, query, intersections):
    out = np.zeros((boxes.shape[0], query.shape[0]), np.float64)
    for k in range(query.shape[0]):
        q = query[k]
        box_area = (q[2] - q[0] + 1) * (q[3] - q[1] + 1)
        iw = np.minimum(boxes[:, 2], q[2]) - np.maximum(boxes[:, 0], q[0]) + 1
        ih = np.minimum(boxes[:, 3], q[3]) - np.maximum(boxes[:, 1], q[1]) + 1
        ok = (iw > 0) & (ih > 0)
        with np.errstate(divide="ignore", invalid="ignore"):      # (pairs the gates drop)
            if intersections:
                v = iw * ih / box_area
            else:
                v = iw * ih / ((boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1) + box_area - iw * ih)
        out[ok, k] = v[ok]
    return out


def strips(rows, per_row, x0, y0, h, gap_y, step=16):
    b = []
    for r in range(rows):
        for i in range(per_row):
            x1, y1 = x0 + i * step, y0 + r * gap_y
            b.append((x1, y1, x1 + 15, y1 + h - 1, 1))
    return np.array(b, np.float32)


def scenes():
    three = np.array([[16, 20, 31, 50, 1], [32, 22, 47, 52, 1], [48, 24, 63, 54, 1]], np.float32)
    far = np.array([[200, 200, 215, 230, 1]], np.float32)
    rng = np.random.default_rng(5)
    big = []
    for r in range(5):
        y = 60 + 100 * r + int(rng.integers(0, 20))
        hh = int(rng.integers(18, 60))
        for i in range(20):
            x = 48 + 16 * i + 16 * 20 * (r % 2)
            big.append((x, y + int(rng.integers(-2, 3)), x + 15, y + hh + int(rng.integers(-2, 3)), 1))
    big = np.array(big, np.float32)
    out = [
        dict(name="three", hf=6, wf=8, im=(96, 128, 1), gt=three),
        dict(name="zero_overlap_box", hf=6, wf=8, im=(96, 128, 1), gt=np.vstack([three, far])),
        dict(name="hard_strip", hf=6, wf=8, im=(96, 128, 1), gt=three, hard=[0, 0, 1]),
        dict(name="dontcare", hf=6, wf=8, im=(96, 128, 1), gt=three, dc=np.array([[0, 0, 60, 95]], np.float32)),
        dict(name="rows_sampled", hf=12, wf=20, im=(192, 320, 1), gt=strips(5, 20, 0, 10, 24, 36)),
        dict(name="map_37x56", hf=37, wf=56, im=(600, 900, 1), gt=big, hash_targets=True),
        # the zero-overlap box again: its column-maximum foreground is what the bg rule, applied last, clobbers
        dict(name="clobber", hf=6, wf=8, im=(96, 128, 1), gt=np.vstack([three, far]), cfg={"RPN_CLOBBER_POSITIVES": True}),
        dict(name="thresholds_half", hf=6, wf=8, im=(96, 128, 1), gt=three, cfg={"RPN_POSITIVE_OVERLAP": 0.5, "RPN_NEGATIVE_OVERLAP": 0.5}),
        dict(name="hard_not_precluded", hf=6, wf=8, im=(96, 128, 1), gt=three, hard=[0, 0, 1], cfg={"PRECLUDE_HARD_SAMPLES": False}),
        dict(name="inside_ones", hf=6, wf=8, im=(96, 128, 1), gt=three, cfg={"RPN_BBOX_INSIDE_WEIGHTS": [1.0, 1.0, 1.0, 1.0]}),
        dict(name="non_integer", hf=12, wf=20, im=(192, 320, 1), gt=(strips(3, 12, 20, 30, 40, 50) * np.float32(0.7324)).astype(np.float32)),
        dict(name="short_image", hf=6, wf=8, im=(95, 128, 1), gt=three),
        dict(name="two_dontcare_hard", hf=12, wf=20, im=(192, 320, 1), gt=strips(2, 10, 32, 40, 30, 70), hard=[0] * 5 + [1] * 3 + [0] * 12,
             dc=np.array([[0, 0, 100, 60], [50, 30, 140, 191]], np.float32)),
    ]
    for s in out:
        s["gt"][:, 4] = 1
    return out


CFG_ORDER = ("RPN_NEGATIVE_OVERLAP", "RPN_POSITIVE_OVERLAP", "RPN_CLOBBER_POSITIVES", "RPN_FG_FRACTION", "RPN_BATCHSIZE", "DONTCARE_AREA_INTERSECTION_HI",
             "PRECLUDE_HARD_SAMPLES")


def cfg12(cfg):
    t = cfg.TRAIN
    return np.array([float(t[k]) for k in CFG_ORDER] + [float(v) for v in t.RPN_BBOX_INSIDE_WEIGHTS] + [float(t.RPN_POSITIVE_WEIGHT)], np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=None, help="a checkout of the reference (default: oracle.make_golden's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "anchor_targets.npz"))
    args = ap.parse_args()
    from oracle import make_golden as MG
    if args.ref:
        MG.REF = args.ref
    MG.install_shim()
    bbox = sys.modules["lib.utils.bbox"]
    bbox.bbox_overlaps = lambda b, q: _pairs(b, q, False)
    bbox.bbox_intersections = lambda b, q: _pairs(b, q, True)
    from lib.fast_rcnn.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(MG.REF, "ctpn", "text.yml"))
    from lib.rpn_msr.anchor_target_layer_tf import anchor_target_layer
    store = {"cfg12": cfg12(cfg)}
    names = []
    for si, s in enumerate(scenes()):
        saved = {k: cfg.TRAIN[k] for k in s.get("cfg", {})}
        for k, v in s.get("cfg", {}).items():
            cfg.TRAIN[k] = v
        score = np.zeros((1, s["hf"], s["wf"], 20), np.float32)
        hard = None if "hard" not in s else np.array(s["hard"], np.int32)
        dc = s.get("dc")
        im = np.array([s["im"]], np.float32)
        seed = 100 + si
        np.random.seed(seed)
        sampled = anchor_target_layer(score, s["gt"], hard, dc, im)
        batch = cfg.TRAIN.RPN_BATCHSIZE
        cfg.TRAIN.RPN_BATCHSIZE = 10 ** 9
        full = anchor_target_layer(score, s["gt"], hard, dc, im)
        cfg.TRAIN.RPN_BATCHSIZE = batch
        p = s["name"] + "/"
        store[p + "map"] = np.array([s["hf"], s["wf"]], np.int32)
        store[p + "im_info"] = im[0]
        store[p + "gt"] = s["gt"]
        if hard is not None:
            store[p + "hard"] = hard
        if dc is not None:
            store[p + "dontcare"] = dc
        store[p + "cfg12"] = cfg12(cfg)
        store[p + "np_seed"] = np.array(seed, np.int64)
        store[p + "labels"] = sampled[0].reshape(-1).astype(np.int8)
        store[p + "labels_presample"] = full[0].reshape(-1).astype(np.int8)
        store[p + "inside_weights"] = sampled[2].reshape(-1, 4).astype(np.float32)
        store[p + "outside_weights"] = sampled[3].reshape(-1, 4).astype(np.float32)
        t = np.ascontiguousarray(full[1].reshape(-1, 4).astype(np.float32))
        assert full[1].dtype == np.float32 and np.array_equal(sampled[1], full[1])
        if s.get("hash_targets"):
            store[p + "targets_sha256"] = np.frombuffer(hashlib.sha256(t.tobytes()).digest(), np.uint8)
        else:
            store[p + "bbox_targets"] = t
        for k, v in saved.items():
            cfg.TRAIN[k] = v
        lab, pre = store[p + "labels"], store[p + "labels_presample"]
        print("%-20s %2d x %2d  G %3d  presample fg %4d bg %5d  sampled fg %4d bg %4d" % (s["name"], s["hf"], s["wf"], len(s["gt"]), (pre == 1).sum(), (pre == 0).sum(),
                                                                                       (lab == 1).sum(), (lab == 0).sum()))
        names.append(s["name"])
    store["scenes"] = np.array(names)
    np.savez_compressed(args.out, **store)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
