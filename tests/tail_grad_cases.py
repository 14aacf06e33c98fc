"""Test infrastructure shared by tests/test_tail_grad.py (CPU) and tests/test_gpu_tail_grad.py: the inputs of the tail-gradient checks, the
error measure, and the one labelled page of the fine-tune check with its settings. Everything here is seeded and computed once."""
import numpy as np

import tail_grad_ref as TR
from util import stress_arena

_CACHE = {}


def tail_weights(kind):
    """the last ten tensors of stress_arena(kind): "biased" or "fullscale" (every bias non-zero)"""
    if kind not in _CACHE:
        _CACHE[kind] = np.ascontiguousarray(stress_arena(kind)[-TR.TAIL_FLOATS:])
    return _CACHE[kind]


# what rpn_conv/3x3 hands the tail: post-ReLU features. "biased": magnitudes of the benchmark arena's features; "fullscale": pre-activations far
# beyond +-88.8, gates at exactly 0 and 1 in fp32
X_SCALE = {"biased": 0.25, "fullscale": 64.0}


def features(n, hf, wf, kind, seed):
    rng = np.random.default_rng([seed, n, hf, wf])
    return (np.maximum(rng.standard_normal((n, hf, wf, 512)), 0.0) * X_SCALE[kind]).astype(np.float32)


def head_gradient(n, hf, wf, seed):
    """a d_heads of the size a loss gives: (n, hf, wf, 64), pad columns 0"""
    rng = np.random.default_rng([seed, 7, n, hf, wf])
    g = np.zeros((n, hf, wf, 64), np.float32)
    g[..., :60] = (rng.standard_normal((n, hf, wf, 60)) * 0.05).astype(np.float32)
    return g


def rel_error(got, ref64):
    """max|got - ref64| / max|ref64| (0 / 0 = 0)"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref64, np.float64).reshape(-1)
    top = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    return 0.0 if err == 0.0 else err / top if top > 0 else float("inf")


def reference(n, hf, wf, kind, seed):
    """(x, tail, d_heads, float64 autograd, float32 autograd) of a case, computed once and shared; never modified"""
    key = ("ref", n, hf, wf, kind, seed)
    if key not in _CACHE:
        import torch
        x, tail, g = features(n, hf, wf, kind, seed), tail_weights(kind), head_gradient(n, hf, wf, seed)
        _CACHE[key] = (x, tail, g, TR.gradients(x, tail, g, torch.float64), TR.gradients(x, tail, g, torch.float32))
    return _CACHE[key]


# ---- the fine-tune check: one labelled synthetic page, a handful of Momentum steps on the tail
FT_H, FT_W = 64, 96
FT_STEPS = 7
FT_LR, FT_MOMENTUM = 0.001, 0.9      # lib/fast_rcnn/config.py TRAIN.LEARNING_RATE, TRAIN.MOMENTUM


def finetune_page():
    """(image (1, 64, 96, 3) uint8, [gt boxes (G, 4)]): two text rows as 16-px strips on the anchor grid"""
    import ctpn_amd
    img = ctpn_amd.weights.synthetic_images(1, FT_H, FT_W, 11)
    boxes = [[16.0 * c, y0, 16.0 * c + 15.0, y1] for (y0, y1, cols) in ((10.0, 26.0, range(1, 5)), (36.0, 58.0, range(0, 4))) for c in cols]
    return img, [np.array(boxes, np.float32)]


def finetune_cfg():
    c =np.array([0.3, 0.7, 0.0, 0.5, 300.0, 0.5, 1.0, 0.0, 1.0, 0.0, 1.0, -1.0])      # ctpn_target_config_default
    c[4] = 0.0      # no subsampling: every labelled anchor counts, nothing depends on a seed
    return c
