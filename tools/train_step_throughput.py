"""`python tools/train_step_throughput.py [--out profiles/train_step_throughput.json]` -- what a training step costs at 600 x 900 x 1, fp32, on
one device, leg by leg, for the resident step (ctpn_amd.Trainer.step: forward, fetch through get_tensor_device, backward, solver_step,
load_weights_device) and for one step of ctpn/finetune.py's host loop (load_weights from the host, forward, fetch through get_tensor,
backward on host arrays, the numpy update); and ctpn_solver_step alone on WEIGHT_FLOATS floats next to torch-ROCm's torch.optim SGD, Adam and
RMSprop (with torch's clip_grad_norm_ in front, as the reference clips) on the same tensors, as GB/s of the bytes each must move.
Medians of 7 alternating runs after one warm-up of each, one process; host clocks around work that ends in a device synchronise.
Measured, not gated: both sets of numbers are reported as they come."""
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
from ctpn_amd import conv_grad as CG  # noqa: E402
from ctpn_amd import solver as S  # noqa: E402
from ctpn_amd.tail_grad import TAIL_OFFSET, momentum_step, tail_backward, tail_forward, tail_views  # noqa: E402

H, W = 600, 900
ROUNDS = 7
LEGS = ("load", "forward", "fetch", "backward", "update")


def page():
    img = ctpn_amd.weights.synthetic_images(1, H, W, 11)
    boxes = np.array([[16.0 * c, y0, 16.0 * c + 15.0, y0 + 20.0] for y0 in (40.0, 200.0, 420.0) for c in range(3, 40)], np.float32)
    return img, [boxes]


def cfg():
    c = ctpn_amd.target_config_default()
    c[4] = 0.0
    return c


class Legs(object):
    def __init__(self):
        self.t = {}
        self.last = None

    def start(self):
        torch.cuda.synchronize()
        self.last = time.perf_counter()

    def __call__(self, leg):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.t[leg] = self.t.get(leg, 0.0) + now - self.last
        self.last = now


def host_step(ctx, arena, velocity, img, gts, k, legs):
    """one step of ctpn/finetune.py's run_steps (network_gradients + momentum_step), cut into its legs"""
    legs.start()
    ctx.load_weights(arena)
    ctx.sync()
    legs("load")
    ctx.forward(img)
    ctx.sync()
    legs("forward")
    fn, hf, wf = ctx.feat_shape()
    need = set(CG.CONVS) | set(p for p, _ in CG.POOL_BEFORE.values())
    acts = {name: np.ascontiguousarray(ctx.get_tensor(name)[:1]) for name in sorted(need)}
    blob = img.astype(np.float32, copy=True)
    blob -= CG.PIXEL_MEANS
    legs("fetch")
    weights, tail, x = ctpn_amd.arena_views(arena), arena[TAIL_OFFSET:], acts["rpn_conv/3x3"]
    fwd = tail_forward(x, tail, True, 0)
    gt5 = [np.concatenate([gts[0], np.ones((len(gts[0]), 1), np.float32)], axis=1)]
    t = ctpn_amd.anchor_targets(hf, wf, np.array([[H, W, 1.0]], np.float32), gt5, None, None, cfg(), k, 0)
    r = ctpn_amd.rpn_loss(fwd.heads, t.labels, t.bbox_targets, t.inside_weights, t.outside_weights, True, 0)
    bwd = tail_backward(x, tail, fwd.saved, r.d_heads, True, 0)
    conv = CG.conv_stack_backward(acts, blob, weights, bwd.d_x, "conv1_1", 0)
    legs("backward")
    conv.update(tail_views(bwd.d_tail))
    g = np.concatenate([conv[name].reshape(-1) for name, _, _ in ctpn_amd.MANIFEST])
    arena, velocity, _ = momentum_step(arena, velocity, g, 0.001, 0.9, 10.0)
    legs("update")
    return arena, velocity


def step_legs():
    img, gts = page()
    arena = ctpn_amd.make_synthetic_arena(0)
    res, host = [], []
    with ctpn_amd.Context(0, 1, H, W, "fp32", options={"keep_acts": 1}) as ctx:
        tr = ctpn_amd.Trainer(ctx, arena, "Momentum", None, 0.0005, "conv1_1", cfg=cfg())
        h_arena, h_vel = arena.copy(), np.zeros_like(arena)
        for k in range(ROUNDS + 1):      # round 0 warms both up
            legs = Legs()
            legs.start()
            tr.step(img, gts, seed=k, mark=legs)
            res.append(legs.t)
            legs = Legs()
            h_arena, h_vel = host_step(ctx, h_arena, h_vel, img, gts, k, legs)
            host.append(legs.t)
            tr._load()      # the ctx holds the resident run's weights again
    out = {}
    for name, runs in (("resident", res[1:]), ("host_loop", host[1:])):
        out[name] = {leg + "_ms": statistics.median(r[leg] for r in runs) * 1e3 for leg in LEGS}
        out[name]["step_ms"] = statistics.median(sum(r.values()) for r in runs) * 1e3
    return out


def solver_alone():
    dev = torch.device("cuda", 0)
    n = ctpn_amd.WEIGHT_FLOATS
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    seg_end, seg_decay = S.decay_table("conv1_1", 0.0005)
    rows = {}
    for name in ("Momentum", "Adam", "RMS"):
        hyper = S.solver_defaults(name)
        w = torch.randn(n, device=dev, generator=gen) * 0.05
        g = torch.randn(n, device=dev, generator=gen) * 0.01
        s1 = torch.full((n,), float(hyper[5]), device=dev)
        s2 = torch.zeros(n, device=dev)
        param = torch.nn.Parameter(w.clone())
        param.grad = g.clone()
        opt = {"Momentum": lambda: torch.optim.SGD([param], lr=1e-3, momentum=0.9, weight_decay=0.0005),
               "Adam": lambda: torch.optim.Adam([param], lr=1e-3, weight_decay=0.0005),
               "RMS": lambda: torch.optim.RMSprop([param], lr=1e-3, alpha=0.9, eps=1e-10, weight_decay=0.0005)}[name]()

        def ours(t):
            S.solver_step(name, w, g, s1, None if name == "Momentum" else s2, hyper, t, seg_end, seg_decay)

        def theirs(t):
            torch.nn.utils.clip_grad_norm_([param], 10.0)
            opt.step()

        mine, torchs = [], []
        for t in range(1, ROUNDS + 2):
            for fn, acc in ((ours, mine), (theirs, torchs)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(t)
                torch.cuda.synchronize()
                acc.append(time.perf_counter() - t0)
        # the bytes each must move. ours: pass 1 reads w, g; pass 2 reads w, g, s1 (s2) and writes w, s1 (s2).
        # torch: the norm reads g, the clip reads and writes g, the step reads w, g and its state and writes w and its state
        state = 1 if name in ("Momentum", "RMS") else 2
        ours_bytes = 4 * n * (2 + (3 if name == "Momentum" else 4) + (2 if name == "Momentum" else 3))
        torch_bytes = 4 * n * (3 + 2 + state + 1 + state)
        m, q = statistics.median(mine[1:]), statistics.median(torchs[1:])
        rows[name] = {"solver_step_ms": m * 1e3, "solver_step_bytes": ours_bytes, "solver_step_GBps": ours_bytes / m / 1e9,
                      "torch_optim_ms": q * 1e3, "torch_optim_bytes": torch_bytes, "torch_optim_GBps": torch_bytes / q / 1e9}
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_throughput.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_throughput: no device; nothing is measured without one")
    rec = {"device": torch.cuda.get_device_name(0), "shape": [1, H, W], "precision": "fp32", "rounds": ROUNDS,
           "note": "medians of %d alternating runs after one warm-up; host clock around work ending in a device synchronise" % ROUNDS,
           "step": step_legs(), "solver_alone": solver_alone()}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
