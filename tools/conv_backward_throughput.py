"""`python tools/conv_backward_throughput.py [--out profiles/conv_backward_throughput.json]` -- how long the backward of every conv layer takes
at 600 x 900 x 1 on device tensors (ctpn_conv3x3_backward: mask, weight, bias and data gradient, no host copy), and the whole chain
rpn_conv/3x3 -> conv1_1 with its four pool backwards, next to torch-ROCm's autograd of the same fp32 convs on the same device. Medians of 7
alternating runs after one warm-up of each, one process. Achieved TFLOP/s count 2 x 9 ci co flops per pixel for the weight gradient and as
many for the data gradient (conv1_1 has none), against the 157 TFLOP/s fp32-matrix peak. Measured, not gated. If torch's conv backward does
not run, the record says so and holds the device's times alone.

`--accuracy [--out profiles/conv_backward_accuracy.json]` instead records, for every case of tests/test_gpu_conv_grad.py, the device's error
and the restatement's float32 error per tensor against float64 autograd, and the worst ratios, per call and end to end."""
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
import conv_grad_ref as CR  # noqa: E402
from ctpn_amd import conv_grad as CG  # noqa: E402

H, W = 600, 900
ROUNDS = 7
PEAK_TFLOPS = 157.3


def med(v):
    return statistics.median(v) * 1e3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def torch_layer(x, w, y, d_y):
    """-> a function that runs autograd's backward of relu(conv(x, w) + b) for the upstream gradient d_y, or raises"""
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    bg = torch.zeros(w.shape[3], device=x.device, requires_grad=True)
    with torch.enable_grad():
        out = CR.conv_relu(xg, wg, bg)
    ins = (wg, bg) if x.shape[3] == 3 else (xg, wg, bg)
    return lambda: torch.autograd.grad(out, ins, d_y, retain_graph=True)


def throughput(with_torch=True):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    rows, acts, weights = [], {}, {}
    torch_ok, torch_note = with_torch, None if with_torch else "not run (--no-torch)"
    blob = torch.randn((1, H, W, 3), device=dev, generator=gen) * 60.0
    for name, shape in CR.layer_shapes(1, H, W):
        n, h, w, ci, co = shape
        acts[name] = torch.relu(torch.randn((n, h, w, co), device=dev, generator=gen))
        weights[name + "/weights"] = torch.randn((3, 3, ci, co), device=dev, generator=gen) / float(np.sqrt(9.0 * ci))
    for conv, pool in CR.POOL_AFTER.items():
        acts[pool] = CR.pool(acts[conv]).contiguous()
    for k, (name, shape) in enumerate(CR.layer_shapes(1, H, W)):
        n, h, w, ci, co = shape
        x = blob if k == 0 else acts[CG.POOL_BEFORE[name][0]] if name in CG.POOL_BEFORE else acts[CR.CONVS[k - 1]]
        y, wt = acts[name], weights[name + "/weights"]
        d_y = torch.randn(y.shape, device=dev, generator=gen) * 0.05
        ours = lambda: ctpn_amd.conv_backward(x, wt, y, d_y, want_dx=ci != 3)      # noqa: E731
        theirs = None
        if torch_ok:
            try:
                theirs = torch_layer(x, wt, y, d_y)
                timed(theirs)
            except Exception as e:      # noqa: BLE001
                torch_ok, torch_note, theirs = False, "torch conv backward did not run: %s" % str(e)[:200], None
        timed(ours)      # warm-up: code objects, allocator
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(timed(ours))
            if theirs:
                b.append(timed(theirs))
        flops = (2 if ci != 3 else 1) * 2.0 * n * h * w * 9 * ci * co
        row = {"layer": name, "n_h_w_ci_co": list(shape), "plan_block_pixels_blocks": list(ctpn_amd.conv_backward_plan(*shape)), "device_ms": med(a),
               "device_tflops": flops / (med(a) * 1e-3) / 1e12, "of_fp32_matrix_peak": flops / (med(a) * 1e-3) / 1e12 / PEAK_TFLOPS}
        if b:
            row["torch_ms"] = med(b)
            row["torch_over_device"] = med(b) / med(a)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del theirs
    # the whole chain, pools included
    d_top = torch.randn(acts["rpn_conv/3x3"].shape, device=dev, generator=gen) * 0.05
    ours = lambda: CG.conv_stack_backward(acts, blob, weights, d_top, "conv1_1", 0)      # noqa: E731
    theirs = None
    if torch_ok:
        try:
            wg = {k: v.clone().requires_grad_(True) for k, v in weights.items()}
            wg.update({c + "/biases": torch.zeros(weights[c + "/weights"].shape[3], device=dev, requires_grad=True) for c in CR.CONVS})
            with torch.enable_grad():
                top = CR.stack_forward(blob, wg)["rpn_conv/3x3"]
            leaves = list(wg.values())
            theirs = lambda: torch.autograd.grad(top, leaves, d_top, retain_graph=True)      # noqa: E731
            timed(theirs)
        except Exception as e:      # noqa: BLE001
            torch_ok, torch_note, theirs = False, "torch conv backward did not run: %s" % str(e)[:200], None
    timed(ours)
    a, b = [], []
    for _ in range(ROUNDS):
        a.append(timed(ours))
        if theirs:
            b.append(timed(theirs))
    flops = sum((2 if s[3] != 3 else 1) * 2.0 * s[0] * s[1] * s[2] * 9 * s[3] * s[4] for _, s in CR.layer_shapes(1, H, W))
    chain = {"device_ms": med(a), "device_tflops": flops / (med(a) * 1e-3) / 1e12, "sum_of_layer_device_ms": sum(r["device_ms"] for r in rows)}
    if b:
        chain["torch_ms"] = med(b)
        chain["torch_over_device"] = med(b) / med(a)
    print(json.dumps(chain), flush=True)
    return {"what": "conv backward per layer and rpn_conv/3x3 -> conv1_1 at %d x %d x 1 on device tensors; medians of %d alternating runs" % (H, W, ROUNDS),
            "device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tflops": PEAK_TFLOPS,
            "comparator": "torch %s autograd of the same fp32 convs (tests/conv_grad_ref.py), same device; backward alone, graph retained" % torch.__version__,
            "comparator_note": torch_note, "layers": rows, "chain": chain}


def accuracy():
    import conv_grad_cases as K
    import test_gpu_conv_grad as G
    calls, worst_call = [], (0.0, None)
    for shape in K.ALL_SHAPES:
        rec = {"n_h_w_ci_co": list(shape), "tensors": {}}
        for name, (diff, bound, e, e32) in G.call_errors(shape).items():
            ratio = 0.0 if e == 0 else (e / e32 if e32 > 0 else float("inf"))
            rec["tensors"][name] = {"device": e, "e32": e32, "ratio": ratio, "worst_diff_over_a_priori_bound": float((diff / np.maximum(bound, 1e-300)).max())}
            if ratio > worst_call[0]:
                worst_call = (ratio, "%s %s" % (shape, name))
        calls.append(rec)
    nets, worst_net = [], (0.0, None)
    for hw in K.NET_SIZES:
        rec = {"h_w": list(hw), "tensors": {}}
        for name, (e, e32) in G.end_to_end_ratios(hw).items():
            ratio = 0.0 if e == 0 else (e / e32 if e32 > 0 else float("inf"))
            rec["tensors"][name] = {"device": e, "e32": e32, "ratio": ratio}
            if ratio > worst_net[0]:
                worst_net = (ratio, "%s %s" % (hw, name))
        nets.append(rec)
    return {"what": "max |got - ref64| / max |ref64| per tensor: the device, and the restatement's float32 autograd (e32), against float64 autograd",
            "device": torch.cuda.get_device_name(0), "worst_ratio_per_call": {"ratio": worst_call[0], "where": worst_call[1], "gated": False},
            "worst_ratio_end_to_end": {"ratio": worst_net[0], "where": worst_net[1], "gate": G.END_TO_END_FACTOR}, "per_call": calls, "end_to_end": nets}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--no-torch", action="store_true", help="the device's times alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    res = accuracy() if args.accuracy else throughput(not args.no_torch)
    out = args.out or os.path.join(ROOT, "profiles", "conv_backward_accuracy.json" if args.accuracy else "conv_backward_throughput.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
