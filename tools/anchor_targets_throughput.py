#!/usr/bin/env python
"""Cost of the label side of training on one MI355X -> profiles/anchor_targets_throughput.json.

Milliseconds per ctpn_anchor_targets + ctpn_rpn_loss pair (targets chained into the loss, with the gradient) on maps 37 x 56 and 80 x 120,
with G in {100, 1000, 4000} strips per image and n in {1, 32} images, in the host-pointer form (every array crosses the bus, both ways) and in
the on_device form (torch tensors, only the small tables cross). Subsampling is on (text.yml's RPN_BATCHSIZE 300): the radix select runs.
For comparison the numpy restatement (tests/anchor_target_ref.py) on this host at n = 1 (up to 2.5e7 anchor x box pairs: it holds the dense
matrix several times over). Medians of --runs runs, the forms ALTERNATING run by
run so that a drift of the shared host touches all alike; min and max are kept. There is no threshold: this tool states a cost.
Needs a GPU: without one the library's calls fail, there is no fallback.

    python tools/anchor_targets_throughput.py [--runs 7] [--out profiles/anchor_targets_throughput.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ctpn_amd  # noqa: E402


def scene(hf, wf, G, seed):
    """G strips of 16 px in rows of text, like split_label.py's output"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, wf, G) * 16
    y = rng.integers(0, hf * 16 - 64, G)
    h = rng.integers(12, 60, G)
    return np.stack([x, y, x + 15, y + h, np.ones(G)], axis=1).astype(np.float32)


def stat(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_targets_throughput.json"))
    args = ap.parse_args(argv)
    import torch
    import anchor_target_ref as R
    dev = torch.device("cuda", 0)
    rows = []
    for hf, wf in ((37, 56), (80, 120)):
        for G in (100, 1000, 4000):
            for n in (1, 32):
                info = np.array([[hf * 16, wf * 16, 1.0]] * n, np.float32)
                gts = [scene(hf, wf, G, 10 * i + 1) for i in range(n)]
                heads = (np.random.default_rng(0).standard_normal((n, hf, wf, 64)) * 0.5).astype(np.float32)
                offs = (np.arange(n + 1) * G).astype(np.int32)
                d_gt, d_heads = torch.from_numpy(np.concatenate(gts)).to(dev), torch.from_numpy(heads).to(dev)

                def host():
                    t = ctpn_amd.anchor_targets(hf, wf, info, gts, seed=1)
                    return ctpn_amd.rpn_loss(heads, t.labels, t.bbox_targets, t.inside_weights, t.outside_weights, want_grad=True)

                def device():
                    t = ctpn_amd.anchor_targets(hf, wf, info, d_gt, seed=1, gt_offsets=offs)
                    return ctpn_amd.rpn_loss(d_heads, t.labels, t.bbox_targets, t.inside_weights, t.outside_weights, want_grad=True)

                def restatement():
                    t = R.anchor_targets(hf, wf, info[0], gts[0], seed=1)
                    return R.rpn_loss(heads[0].reshape(-1, 64), t["labels"], t["bbox_targets"], t["inside_weights"], t["outside_weights"])

                # the restatement holds the dense anchors x G matrix several times over: only where that stays below a few GB
                forms = [("host_pointers", host), ("on_device", device)] + ([("numpy_restatement", restatement)] if n == 1 and hf * wf * 10 * G <= 25000000 else [])
                a, b = host(), device()                       # warm-up, and the two forms agree
                assert a.losses.tobytes() == b.losses.tobytes()
                times = {k: [] for k, _ in forms}
                for _ in range(args.runs):
                    for k, fn in forms:
                        if k == "numpy_restatement" and len(times[k]) >= 3:
                            continue
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        times[k].append((time.perf_counter() - t0) * 1e3)      # both calls return synchronised
                row = {"map": [hf, wf], "anchors": hf * wf * 10, "G": G, "n": n, "pairs": n * hf * wf * 10 * G, "model_loss_image0": float(a.losses[0, 2])}
                row.update({k: stat(v) for k, v in times.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "what": "ms per ctpn_anchor_targets + ctpn_rpn_loss pair (with d_heads), RPN_BATCHSIZE 300",
           "runs": args.runs, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
