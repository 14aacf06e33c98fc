#!/usr/bin/env python
"""What ragged batches (ctpn_detect_submit_ragged) buy on a folder of portrait pages: 600-wide images whose heights are drawn from 776
(letter), 800 (3:4), 849 (A4) and 1067 (9:16), detected three ways through the pipelined submit / collect pair:

    (a) grouped by shape, as ctpn/demo_batch.py groups them without --ragged (the uniform path, which this feature does not touch);
    (b) the same images in ragged batches (demo_batch.plan_ragged_batches, --waste);
    (c) (b)'s canvases as UNIFORM batches of the canvas size -- wrong results for the padded images, the same kernels: what the masks and
        the stand-alone conv1_1 of a ragged forward cost.

The three forms run interleaved, --repeats times; every rate is reported with its spread. Images are resident on the device unless
--host is given (then every batch crosses PCIe, the padded rows of (b) and (c) included).

    python tools/ragged_throughput.py --images 64 --out profiles/ragged_throughput.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--waste", type=float, default=None, help="plan_ragged_batches' waste (default: demo_batch.RAGGED_WASTE)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precisions", default="bf16,split")
    ap.add_argument("--host", action="store_true", help="submit host arrays instead of device-resident batches")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctpn_amd
    from ctpn_amd.ctpn.demo_batch import plan_ragged_batches, RAGGED_WASTE
    from ctpn_amd.lib.utils.blob import im_list_to_canvas
    waste = RAGGED_WASTE if args.waste is None else args.waste
    rng = np.random.default_rng(args.seed)
    heights = [int(h) for h in rng.choice([776, 800, 849, 1067], args.images)]
    distinct = {h: ctpn_amd.weights.synthetic_images(1, h, 600, 100 + h)[0] for h in sorted(set(heights))}
    ims = [distinct[h] for h in heights]
    # (a): one batch per shape, at most --batch images each
    jobs_a = []
    for h in sorted(set(heights)):
        idx = [i for i, x in enumerate(heights) if x == h]
        for lo in range(0, len(idx), args.batch):
            jobs_a.append((np.stack([ims[i] for i in idx[lo:lo + args.batch]]), None))
    # (b), (c)
    batches, alone = plan_ragged_batches([(h, 600) for h in heights], args.batch, waste)
    jobs_b, jobs_c = [], []
    for _, members in batches:
        canvas, hts = im_list_to_canvas([ims[i] for i in members])
        jobs_b.append((canvas, hts))
        jobs_c.append((canvas, None))
    for i in alone:
        jobs_b.append((ims[i][None], None))
        jobs_c.append((ims[i][None], None))
    padded = sum(int(c.shape[0] * c.shape[1] - h.sum()) for c, h in jobs_b if h is not None)
    out = {"images": args.images, "width": 600, "heights": {str(h): heights.count(h) for h in sorted(set(heights))}, "max_batch": args.batch, "waste": waste,
           "resident": not args.host, "repeats": args.repeats,
           "batches": {"a_grouped": [int(j[0].shape[0]) for j in jobs_a], "b_ragged": [int(j[0].shape[0]) for j in jobs_b]},
           "b_padded_share_of_rows": round(padded / float(sum(c.shape[0] * c.shape[1] for c, _ in jobs_b)), 4)}
    arena = ctpn_amd.make_synthetic_arena(0)
    for prec in args.precisions.split(","):
        with ctpn_amd.Context(0, args.batch, max(heights), 600, prec) as ctx:
            ctx.load_weights(arena)
            keep = []

            def resident(jobs):
                if args.host:
                    return [(a, None, h) for a, h in jobs]
                import torch
                res = []
                for a, h in jobs:
                    t = torch.from_numpy(a).cuda()
                    keep.append(t)
                    res.append((None, (t.data_ptr(), a.shape[:3]), h))
                torch.cuda.synchronize()
                return res

            def run(jobs):
                t0 = time.perf_counter()
                for k, (a, dev, h) in enumerate(jobs):
                    ctx.detect_submit(a, slot=k & 1, heights=h, device_ptr=dev[0] if dev else None, shape=dev[1] if dev else None)
                    if k:
                        ctx.detect_collect((k - 1) & 1, line_capacity=1024)
                ctx.detect_collect((len(jobs) - 1) & 1, line_capacity=1024)
                return args.images / (time.perf_counter() - t0)
            forms = {"a_grouped": resident(jobs_a), "b_ragged": resident(jobs_b), "c_uniform_canvas": resident(jobs_c)}
            for jobs in forms.values():      # warm-up: every geometry once
                run(jobs)
            rates = {k: [] for k in forms}
            for _ in range(args.repeats):
                for k, jobs in forms.items():
                    rates[k].append(run(jobs))
            out[prec] = {k: {"images_per_s_median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                             "runs": [round(x, 1) for x in v]} for k, v in rates.items()}
            out[prec]["b_over_a"] = round(out[prec]["b_ragged"]["images_per_s_median"] / out[prec]["a_grouped"]["images_per_s_median"], 3)
            out[prec]["b_over_c"] = round(out[prec]["b_ragged"]["images_per_s_median"] / out[prec]["c_uniform_canvas"]["images_per_s_median"], 3)
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
