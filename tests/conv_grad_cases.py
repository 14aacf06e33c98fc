"""Test infrastructure shared by tests/test_conv_grad.py (CPU) and tests/test_gpu_conv_grad.py: the shapes and inputs of the conv-gradient
checks, their float64 references and a priori bounds. Everything here is seeded and computed once."""
import numpy as np
import torch

import conv_grad_ref as CR
from tail_grad_cases import rel_error  # noqa: F401

_CACHE = {}

# (n, h, w, ci, co): the smallest shapes at which each piece can go wrong
SHAPES = [(1, 1, 1, 32, 64),        # every tap but the centre is border
          (1, 2, 3, 32, 64),        # small map
          (1, 5, 7, 64, 64),        # odd sides
          (2, 4, 6, 32, 128),       # image seam
          (1, 16, 17, 32, 64), (1, 9, 33, 64, 128),      # either side of 16- and 32-pixel tiles
          (3, 7, 5, 32, 64),        # batch of three, odd sides
          (1, 2, 3, 512, 512),      # the full channel count
          (1, 6, 10, 3, 64), (2, 5, 5, 3, 64)]      # conv1_1's form, d_x NULL
# read off ctpn_conv3x3_backward_plan (the tests assert it): {shape: (block_pixels, blocks, pixels of the last block)}
PLAN_SHAPES = {(1, 8, 8, 32, 64): (64, 1, 64),          # exactly one block
               (1, 10, 10, 32, 64): (64, 2, 36),        # a short last block
               (1, 12, 17, 32, 64): (64, 4, 12),        # at least three blocks
               (1, 70, 67, 32, 64): (192, 25, 82)}      # blocks longer than the 128 pixels the weight gradient stages at a time
ALL_SHAPES = SHAPES + list(PLAN_SHAPES)
POOL_SHAPES = [(1, 2, 2, 64), (1, 3, 5, 64), (2, 7, 11, 128), (1, 1, 1, 64)]      # (n, h, w, c); the last one's pooled map is empty: all zeros


def _sparse(rng, shape, hi, density):
    return (rng.integers(-hi, hi + 1, shape) * (rng.random(shape) < density)).astype(np.float32)


def exact_case(shape, seed=1):
    """sparse small integers; y holds zeros and positives under non-zero d_y. -> (x, w, y, d_y, (d_w, d_b, d_x) float64). The float64 sums of
    |terms| stay below 2^24, so every product and sum is exact in fp32 whatever the order."""
    key = ("exact", shape, seed)
    if key not in _CACHE:
        n, h, w, ci, co = shape
        rng = np.random.default_rng([seed, n, h, w, ci, co])
        x, wt = _sparse(rng, (n, h, w, ci), 3, 0.5), _sparse(rng, (3, 3, ci, co), 2, 0.3)
        y = np.maximum(_sparse(rng, (n, h, w, co), 3, 0.9), 0.0)
        d_y = rng.integers(1, 3, (n, h, w, co)).astype(np.float32) * rng.choice([-1.0, 1.0], (n, h, w, co)).astype(np.float32)
        assert (y == 0).any() and (y > 0).any() and (d_y[y == 0] != 0).all()
        ref = CR.conv_backward(x, wt, y, d_y, torch.float64)
        bound = CR.conv_backward_abs(x, wt, y, d_y)
        assert max(float(b.max()) for b in bound) < 2.0 ** 24, "the case is not exact in fp32"
        _CACHE[key] = (x, wt, y, d_y, ref)
    return _CACHE[key]


def random_case(shape, seed=2):
    """-> (x, w, y, d_y, ref64 (d_w, d_b, d_x), ref32, abs sums (d_w, d_b, d_x)); y is a post-ReLU map of its own, about half zeros: the mask is
    an input of the call"""
    key = ("random", shape, seed)
    if key not in _CACHE:
        n, h, w, ci, co = shape
        rng = np.random.default_rng([seed, n, h, w, ci, co])
        x = np.maximum(rng.standard_normal((n, h, w, ci)), 0.0).astype(np.float32) if ci != 3 else (rng.standard_normal((n, h, w, ci)) * 60.0).astype(np.float32)
        wt = (rng.standard_normal((3, 3, ci, co)) / np.sqrt(9.0 * ci)).astype(np.float32)
        y = np.maximum(rng.standard_normal((n, h, w, co)), 0.0).astype(np.float32)
        d_y = (rng.standard_normal((n, h, w, co)) * 0.05).astype(np.float32)
        _CACHE[key] = (x, wt, y, d_y, CR.conv_backward(x, wt, y, d_y, torch.float64), CR.conv_backward(x, wt, y, d_y, torch.float32),
                       CR.conv_backward_abs(x, wt, y, d_y))
    return _CACHE[key]


def a_priori_bounds(shape, abs_sums):
    """|got - ref64| <= (K + 2) 2^-24 sum |a_i b_i| elementwise: an fp32 fma sum of K terms in ANY order is within K u of the exact sum relative
    to sum |a_i b_i| (u = 2^-24, to first order; one u each is added for the rounding of the float64 reference to the fp32 result and for
    the second-order terms). K: 9 co for d_x; the pixel count for d_w (the ordered pass over the partials is part of the same sum) and d_b.
    -> (bound d_w, bound d_b, bound d_x)"""
    n, h, w, ci, co = shape
    M = n * h * w
    u = 2.0 ** -24
    return (M + 2) * u * abs_sums[0], (M + 2) * u * abs_sums[1], (9 * co + 2) * u * abs_sums[2]


def pool_exact_case(shape, seed=3):
    """tied integer data: values 0..2, so that most windows hold their maximum more than once; -> (y_full, d_pool, d_full float64)"""
    n, h, w, c = shape
    rng = np.random.default_rng([seed, n, h, w, c])
    y = rng.integers(0, 3, (n, h, w, c)).astype(np.float32)
    d_pool = rng.integers(1, 5, (n, h // 2, w // 2, c)).astype(np.float32)
    return y, d_pool, CR.pool_backward(y, d_pool, torch.float64)


# ---- the network checks: one 48 x 80 image, and one whose conv4 map has odd sides (56 x 88 -> 7 x 11)
NET_SIZES = [(48, 80), (56, 88)]
FT_H, FT_W, FT_STEPS, FT_LR, FT_MOMENTUM = 48, 80, 4, 0.001, 0.9


def net_page(h, w):
    """(image (1, h, w, 3) uint8, [gt boxes (G, 4)]): two text rows as 16-px strips on the anchor grid"""
    import ctpn_amd
    img = ctpn_amd.weights.synthetic_images(1, h, w, 11)
    boxes = [[16.0 * c, y0, 16.0 * c + 15.0, y1] for (y0, y1, cols) in ((6.0, 20.0, range(1, 4)), (26.0, 44.0, range(0, 4))) for c in cols]
    return img, [np.array(boxes, np.float32)]


def net_cfg():
    c = np.array([0.3, 0.7, 0.0, 0.5, 300.0, 0.5, 1.0, 0.0, 1.0, 0.0, 1.0, -1.0])      # ctpn_target_config_default
    c[4] = 0.0      # no subsampling: every labelled anchor counts, nothing depends on a seed
    return c
