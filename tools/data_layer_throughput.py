"""`python tools/data_layer_throughput.py [--out profiles/data_layer_throughput.json]` -- what the training data layer costs at 600 x 900 x 1,
fp32, on one device.

step: one Trainer step preceded by the preparation of its page, three ways in alternation -- `host_prep`: what ctpn/train_net.py without
--data-layer does to a page (imutil.imread, demo.resize_im, score_pages.scale_boxes), then Trainer.step on the host arrays; `layer_prefetch`
and `layer_no_prefetch`: DataLayer.next(), then Trainer.step_record. train_net.py without --data-layer prepares every page ONCE, before its
first step, so `host_prep` is not that loop as it runs: the rows compare the two preparations, each paid per step, and `step_alone` is the
step on arrays prepared beforehand. The folder: four 400 x 600 PNG pages (factor 1.5 -> 600 x 900), three text rows each.

calls: the three C calls alone, whole calls as a caller sees them (a stream, the call's blocks, one synchronise): ctpn_split_labels on
100 000 quads, ctpn_train_page at 600 x 900 (from a 400 x 600 device page by 1.5 with flip and blob; achieved GB/s of the bytes it must
move: the source once, both outputs once), ctpn_train_boxes on 4 000 strips.

Medians of 7 alternating runs after one warm-up of each, one process; host clocks around work that ends in a device synchronise.
Measured, not gated: the numbers are reported as they come."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ctpn_amd  # noqa: E402
from ctpn_amd.ctpn import demo as D  # noqa: E402
from ctpn_amd.ctpn.score_pages import read_labels, scale_boxes  # noqa: E402
from ctpn_amd.data_layer import read_quads  # noqa: E402
from ctpn_amd.lib.utils import image as imutil  # noqa: E402

FH, FW, H, W = 400, 600, 600, 900
ROUNDS = 7
PAGES = 4


def cfg():
    c = ctpn_amd.target_config_default()
    c[4] = 0.0
    return c


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def make_folder(d):
    """-> (image paths, quad label paths, strip label paths): the strips are the quads' own, in file coordinates, as the older format wants"""
    from PIL import Image
    paths, qpaths, spaths = [], [], []
    for k in range(PAGES):
        img = ctpn_amd.weights.synthetic_images(1, FH, FW, 60 + k)[0]
        p = os.path.join(d, "page_%d.png" % k)
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(p)
        quads = np.array([[40 + k, y, 560, y + 2, 561, y + 24, 41, y + 22] for y in (40.0, 160.0, 300.0)], np.float64)
        qp, sp = os.path.join(d, "gt_page_%d.txt" % k), os.path.join(d, "page_%d.txt" % k)
        with open(qp, "w") as f:
            f.write("".join(",".join("%g" % v for v in q) + "\n" for q in quads))
        strips, _ = ctpn_amd.split_labels([[FH, FW, FH, FW]], quads, [0, len(quads)], 0)
        with open(sp, "w") as f:
            f.write("".join("text\t%d\t%d\t%d\t%d\n" % tuple(int(v) for v in s) for s in strips))
        paths.append(p)
        qpaths.append(qp)
        spaths.append(sp)
    return paths, qpaths, spaths


def steps():
    arena = ctpn_amd.make_synthetic_arena(0)
    rows = {"host_prep": [], "layer_prefetch": [], "layer_no_prefetch": [], "step_alone": []}
    prep = {"host_prep": [], "layer_prefetch": [], "layer_no_prefetch": []}
    with tempfile.TemporaryDirectory() as d, ctpn_amd.Context(0, 1, H, W, "fp32", options={"keep_acts": 1}) as ctx:
        paths, qpaths, spaths = make_folder(d)
        quads = [read_quads(p) for p in qpaths]
        tr = ctpn_amd.Trainer(ctx, arena, "Momentum", None, 0.0005, "conv1_1", cfg=cfg())
        with ctpn_amd.DataLayer(0, paths, quads, flipped=True, seed=3, prefetch=True) as on, \
                ctpn_amd.DataLayer(0, paths, quads, flipped=True, seed=3, prefetch=False) as off:
            assert on.max_shape() == (H, W)
            for k in range(ROUNDS + 1):      # round 0 warms everything up
                page = k % PAGES

                def host_prep():
                    img, f = D.resize_im(imutil.imread(paths[page]), scale=600, max_scale=1200)
                    return img, scale_boxes(read_labels(spaths[page]), f)
                t_prep, (img, boxes) = timed(host_prep)
                t_step, _ = timed(lambda: tr.step(img[None], [boxes], seed=k))
                rows["host_prep"].append(t_prep + t_step)
                prep["host_prep"].append(t_prep)
                rows["step_alone"].append(t_step)
                for name, layer in (("layer_prefetch", on), ("layer_no_prefetch", off)):
                    t_prep, rec = timed(layer.next)
                    t_step, _ = timed(lambda: tr.step_record(rec, seed=k))
                    rows[name].append(t_prep + t_step)
                    prep[name].append(t_prep)
    out = {name + "_step_ms": statistics.median(v[1:]) * 1e3 for name, v in rows.items()}
    out.update({name + "_prep_ms": statistics.median(v[1:]) * 1e3 for name, v in prep.items()})
    return out


def calls():
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(1)
    n = 100000
    x0, y0 = rs.uniform(0, 800, n), rs.uniform(0, 560, n)
    bw, bh = rs.uniform(10, 400, n), rs.uniform(8, 40, n)
    quads = np.stack([x0, y0, x0 + bw, y0, x0 + bw, y0 + bh, x0, y0 + bh], axis=1)
    dims, offs = [[H, W, H, W]], [0, n]
    quads_dev = torch.from_numpy(quads).to(dev)
    page_dev = torch.from_numpy(ctpn_amd.weights.synthetic_images(1, FH, FW, 3)[0]).to(dev)
    page_host = page_dev.cpu().numpy()
    strips = ctpn_amd.split_labels(dims, quads[:400], [0, 400], 0, on_device=True)[0][:4000].contiguous()
    assert strips.shape[0] == 4000
    fns = {
        "split_labels_device_ms": lambda: ctpn_amd.split_labels(dims, quads_dev, offs, 0, on_device=True),
        "split_labels_host_ms": lambda: ctpn_amd.split_labels(dims, quads, offs, 0),
        "train_page_device_ms": lambda: ctpn_amd.train_page(page_dev, 1.5, True, 0),
        "train_page_host_ms": lambda: ctpn_amd.train_page(page_host, 1.5, True, 0),
        "train_boxes_device_ms": lambda: ctpn_amd.train_boxes(strips, W, True, 1000.0 / 1200.0, 0),
    }
    acc = {k: [] for k in fns}
    n_strips = 0
    for _ in range(ROUNDS + 1):
        for name, fn in fns.items():
            t, out = timed(fn)
            acc[name].append(t)
            if name == "split_labels_device_ms":
                n_strips = int(out[0].shape[0])
    out = {k: statistics.median(v[1:]) * 1e3 for k, v in acc.items()}
    out["split_labels_quads"], out["split_labels_strips"] = n, n_strips
    moved = FH * FW * 3 + H * W * 3 + H * W * 3 * 4
    out["train_page_bytes"] = moved
    out["train_page_device_GBps"] = moved / (out["train_page_device_ms"] * 1e-3) / 1e9
    out["train_boxes_strips"] = 4000
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_layer_throughput.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_layer_throughput: no device; nothing is measured without one")
    rec = {"device": torch.cuda.get_device_name(0), "shape": [1, H, W], "precision": "fp32", "rounds": ROUNDS,
           "note": "medians of %d alternating runs after one warm-up; host clock around work ending in a device synchronise; host_prep is the "
                   "parent's preparation paid per step, which ctpn/train_net.py without --data-layer pays once per page before its first step" % ROUNDS,
           "step": steps(), "calls": calls()}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
