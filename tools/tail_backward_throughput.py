"""`python tools/tail_backward_throughput.py [--out profiles/tail_backward_throughput.json]` -- how long the recurrent tail's forward with saved
activations plus its backward take on device tensors (ctpn_tail_forward + ctpn_tail_backward, no host copy), next to torch-ROCm's autograd
of tests/tail_grad_ref.py's restatement on the same device and tensors, at 37 x 56 x {1, 32} images and 80 x 120 x 1. Medians of 7
alternating runs after one warm-up of each. Measured, not gated.

`--accuracy [--out profiles/tail_backward_accuracy.json]` instead records, for every case of tests/test_gpu_tail_grad.py's stage test, the
device's error and the restatement's float32 error per tensor against float64 autograd, and the worst ratio."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ctpn_amd  # noqa: E402
import tail_grad_cases as K  # noqa: E402
import tail_grad_ref as TR  # noqa: E402

SHAPES = [(1, 37, 56), (32, 37, 56), (1, 80, 120)]
ROUNDS = 7


def throughput():
    dev = torch.device("cuda", 0)
    tail = K.tail_weights("biased")
    rows = []
    for n, hf, wf in SHAPES:
        x = torch.from_numpy(K.features(n, hf, wf, "biased", 1)).to(dev)
        g = torch.from_numpy(K.head_gradient(n, hf, wf, 1)).to(dev)
        td = torch.from_numpy(tail).to(dev)
        w = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev).requires_grad_(True) for k, v in TR.split_tail(tail).items()}
        xg = x.clone().requires_grad_(True)

        def ours():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = ctpn_amd.tail_forward(x, td)
            t1 = time.perf_counter()
            b = ctpn_amd.tail_backward(x, td, f.saved, g, want_dx=True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            return t1 - t0, t2 - t1, b

        def autograd():
            for v in list(w.values()) + [xg]:
                v.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.enable_grad():
                heads = TR.forward(xg, w)["heads"]
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                (heads * g[..., :60]).sum().backward()
            torch.cuda.synchronize()
            return t1 - t0, time.perf_counter() - t1

        ours(), autograd()      # warm-up: code objects, allocator
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(ours()[:2])
            b.append(autograd())
        got = ours()[2]
        ref = torch.cat([w[k].grad.reshape(-1) for k in TR.TAIL_NAMES])
        med = lambda v: statistics.median(v) * 1e3      # noqa: E731
        row = {"n": n, "hf": hf, "wf": wf, "cells": n * hf * wf,
               "device_forward_ms": med([t[0] for t in a]), "device_backward_ms": med([t[1] for t in a]), "device_total_ms": med([t[0] + t[1] for t in a]),
               "torch_forward_ms": med([t[0] for t in b]), "torch_backward_ms": med([t[1] for t in b]), "torch_total_ms": med([t[0] + t[1] for t in b]),
               "max_abs_diff_of_gradients": float((got.d_tail - ref).abs().max()), "max_abs_gradient": float(ref.abs().max())}
        row["torch_over_device"] = row["torch_total_ms"] / row["device_total_ms"]
        rows.append(row)
        print(json.dumps(row))
    return {"what": "recurrent tail forward (saving) + backward on device tensors; medians of %d alternating runs" % ROUNDS,
            "device": torch.cuda.get_device_name(0), "comparator": "torch %s autograd of tests/tail_grad_ref.py, float32, same device and tensors" % torch.__version__,
            "rows": rows}


def accuracy():
    import test_gpu_tail_grad as G
    cases, worst_grad, worst_fwd = [], (0.0, None), (0.0, None)
    for kind, shape in G.CASES:
        errs, _ = G.stage_errors(kind, shape)
        rec = {"kind": kind, "n_hf_wf": list(shape), "tensors": {}}
        for k, (e, e32) in errs.items():
            ratio = 0.0 if e == 0 else (e / e32 if e32 > 0 else float("inf"))
            rec["tensors"][k] = {"device": e, "e32": e32, "ratio": ratio}
            if k in G.GRADIENT_STAGES and ratio > worst_grad[0]:
                worst_grad = (ratio, "%s %s %s" % (kind, shape, k))
            if k in G.FORWARD_STAGES and ratio > worst_fwd[0]:
                worst_fwd = (ratio, "%s %s %s" % (kind, shape, k))
        cases.append(rec)
    return {"what": "max |got - ref64| / max |ref64| per tensor: the device, and the restatement's float32 autograd (e32), against float64 autograd",
            "device": torch.cuda.get_device_name(0), "worst_ratio_gradient_stages": {"ratio": worst_grad[0], "where": worst_grad[1]},
            "worst_ratio_forward_stages": {"ratio": worst_fwd[0], "where": worst_fwd[1]}, "cases": cases}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    res = accuracy() if args.accuracy else throughput()
    out = args.out or os.path.join(ROOT, "profiles", "tail_backward_accuracy.json" if args.accuracy else "tail_backward_throughput.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
