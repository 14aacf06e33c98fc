"""The backward pass through the conv stack over the C ABI (include/ctpn_hip.h, "the conv stack: backward"): conv_backward is one conv + bias +
ReLU layer (the data gradient, the weight and the bias gradient), pool_backward the 2x2 max-pool, conv_backward_plan the fixed order of the
weight gradient's sum over pixels. They take numpy arrays, or torch tensors on the device, which go through on_device = 1 with no host copy.
network_gradients chains a ctx's forward into targets, loss, the tail's backward and these calls: the gradient of model_loss at every tensor of
the arena. network_gradients fetches the stored activations through get_tensor, onto the host and back; ctpn_amd.train has the same chain
on device tensors (network_gradients_device) and the optimisers around it; the data layers: data_layer.py."""
import collections
import ctypes as C

import numpy as np

from . import _binding as B
from .targets import _dev_ptr, _is_torch, anchor_targets, rpn_loss
from .tail_grad import TAIL_OFFSET, tail_backward, tail_forward, tail_views
from .weights import WEIGHT_FLOATS, arena_views

CONVS = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2", "conv5_3",
         "rpn_conv/3x3"]
POOL_BEFORE = {"conv2_1": ("pool1", "conv1_2"), "conv3_1": ("pool2", "conv2_2"), "conv4_1": ("pool3", "conv3_3"), "conv5_1": ("pool4", "conv4_3")}
PIXEL_MEANS = np.array([[[102.9801, 115.9465, 122.7717]]])      # lib/fast_rcnn/config.py:200

ConvBackward = collections.namedtuple("ConvBackward", "d_w d_b d_x")


def conv_backward_plan(n, h, w, ci, co):
    """ctpn_conv3x3_backward_plan -> (block_pixels, blocks): the n h w pixels, in (image, row, column) order, are summed in `blocks` consecutive
    blocks of `block_pixels` (the last may be short). Host arithmetic on the shape alone; needs no device."""
    bp, nb = C.c_longlong(0), C.c_int(0)
    B._check(B.load_library().ctpn_conv3x3_backward_plan(int(n), int(h), int(w), int(ci), int(co), C.byref(bp), C.byref(nb)))
    return int(bp.value), int(nb.value)


def _nhwc(x, what):
    if x.ndim != 4:
        raise ValueError("%s is (n, h, w, c)" % what)
    return tuple(int(v) for v in x.shape)


def conv_backward(x, w, y, d_y, want_dx=True, device_id=0, out=None):
    """ctpn_conv3x3_backward for the layer y = relu(conv(x, w) + b) -> ConvBackward(d_w (3, 3, ci, co), d_b (co,), d_x (n, h, w, ci) or None).
    x: (n, h, w, ci) float32, the layer's input; w: (3, 3, ci, co) in TF's HWIO; y: (n, h, w, co), the stored post-ReLU output; d_y: the gradient at
    y. ci = 3 is conv1_1: want_dx must be False. All numpy, or all torch tensors on cuda:device_id (the results are then tensors there).
    out: (d_w, d_b), device tensors of 9 ci co and co floats the two gradients are written to (views of a flat gradient vector)."""
    lib = B.load_library()
    n, h, wd, ci = _nhwc(x, "x")
    co = int(w.shape[3]) if w.ndim == 4 else -1
    if tuple(int(v) for v in w.shape) != (3, 3, ci, co) or _nhwc(y, "y") != (n, h, wd, co) or _nhwc(d_y, "d_y") != (n, h, wd, co):
        raise ValueError("conv_backward: x (n, h, w, ci), w (3, 3, ci, co), y and d_y (n, h, w, co)")
    if _is_torch(x):
        import torch
        dev = torch.device("cuda", int(device_id))
        ptrs = [_dev_ptr(t, torch.float32, device_id, name) for t, name in ((x, "x"), (w, "w"), (y, "y"), (d_y, "d_y"))]
        if out is None:
            d_w = torch.empty((3, 3, ci, co), dtype=torch.float32, device=dev)
            d_b = torch.empty((co,), dtype=torch.float32, device=dev)
        else:
            d_w, d_b = out
            _dev_ptr(d_w, torch.float32, device_id, "out[0]"), _dev_ptr(d_b, torch.float32, device_id, "out[1]")
            if d_w.numel() != 9 * ci * co or d_b.numel() != co:
                raise ValueError("conv_backward: out is (9 ci co floats, co floats)")
            d_w = d_w.view(3, 3, ci, co)
        d_x = torch.empty((n, h, wd, ci), dtype=torch.float32, device=dev) if want_dx else None
        outs = [C.c_void_p(d_w.data_ptr()), C.c_void_p(d_b.data_ptr()), None if d_x is None else C.c_void_p(d_x.data_ptr())]
        torch.cuda.current_stream(dev).synchronize()      # the call runs on a stream of its own: what torch queued for these tensors is done first
        on_dev = 1
    else:
        if out is not None:
            raise ValueError("conv_backward: out= goes with device tensors")
        x, w, y, d_y = B._f32(x), B._f32(w), B._f32(y), B._f32(d_y)
        d_w, d_b = np.empty((3, 3, ci, co), np.float32), np.empty((co,), np.float32)
        d_x = np.empty((n, h, wd, ci), np.float32) if want_dx else None
        ptrs = [a.ctypes.data_as(C.c_void_p) for a in (x, w, y, d_y)]
        outs = [d_w.ctypes.data_as(C.c_void_p), d_b.ctypes.data_as(C.c_void_p), None if d_x is None else d_x.ctypes.data_as(C.c_void_p)]
        on_dev = 0
    B._check(lib.ctpn_conv3x3_backward(int(device_id), n, h, wd, ci, co, ptrs[0], ptrs[1], ptrs[2], ptrs[3], on_dev, outs[0], outs[1], outs[2]))
    return ConvBackward(d_w, d_b, d_x)


def pool_backward(y_full, d_pool, device_id=0):
    """ctpn_maxpool2x2_backward -> d_full (n, h, w, c): d_pool (n, h // 2, w // 2, c) at the first maximum of each 2x2 window of y_full
    (n, h, w, c) in (row, column) scan order, zero elsewhere. With h or w = 1 the pooled map is empty and d_full is all zeros."""
    lib = B.load_library()
    n, h, w, c = _nhwc(y_full, "y_full")
    if _nhwc(d_pool, "d_pool") != (n, h // 2, w // 2, c):
        raise ValueError("pool_backward: d_pool is (n, h // 2, w // 2, c) for y_full's (n, h, w, c)")
    if _is_torch(y_full):
        import torch
        dev = torch.device("cuda", int(device_id))
        py, pd = _dev_ptr(y_full, torch.float32, device_id, "y_full"), _dev_ptr(d_pool, torch.float32, device_id, "d_pool")
        d_full = torch.empty((n, h, w, c), dtype=torch.float32, device=dev)
        po = C.c_void_p(d_full.data_ptr())
        torch.cuda.current_stream(dev).synchronize()
        on_dev = 1
    else:
        y_full, d_pool = B._f32(y_full), B._f32(d_pool)
        d_full = np.empty((n, h, w, c), np.float32)
        py, po = y_full.ctypes.data_as(C.c_void_p), d_full.ctypes.data_as(C.c_void_p)
        pd = d_pool.ctypes.data_as(C.c_void_p) if d_pool.size else None
        on_dev = 0
    B._check(lib.ctpn_maxpool2x2_backward(int(device_id), n, h, w, c, py, pd, on_dev, po))
    return d_full


def conv_stack_backward(acts, blob, weights, d_top, from_layer="conv1_1", device_id=0, each=None, outs=None):
    """The walk from rpn_conv/3x3 back to from_layer. acts: {name: stored post-ReLU output (n, h, w, c)} for the convs walked, and for the convs
    a pool follows (their full-resolution maps) and the pools in between; blob: conv1_1's input; weights: {name + "/weights": HWIO}; d_top: the
    gradient at rpn_conv/3x3's output. each(name, x, y, d_y, result) is called per conv, each(pool, y_full, None, d_pool, d_full) per pool (tests).
    outs: {name + "/weights" | "/biases": device tensor the gradient is written to} (conv_backward's out=). -> {name + "/weights" | "/biases": gradient}"""
    if from_layer not in CONVS:
        raise ValueError("from_layer is one of " + ", ".join(CONVS))
    first = CONVS.index(from_layer)
    grads = {}
    d_y = d_top
    for k in range(len(CONVS) - 1, first - 1, -1):
        name = CONVS[k]
        if k == 0:
            x = blob
        elif name in POOL_BEFORE:
            x = acts[POOL_BEFORE[name][0]]
        else:
            x = acts[CONVS[k - 1]]
        want_dx = k > first
        out = None if outs is None else (outs[name + "/weights"], outs[name + "/biases"])
        r = conv_backward(x, weights[name + "/weights"], acts[name], d_y, want_dx, device_id, out)
        if each:
            each(name, x, acts[name], d_y, r)
        grads[name + "/weights"], grads[name + "/biases"] = r.d_w, r.d_b
        if want_dx:
            d_y = r.d_x
            if name in POOL_BEFORE:
                pool, full = POOL_BEFORE[name]
                d_pool, d_y = d_y, pool_backward(acts[full], d_y, device_id)
                if each:
                    each(pool, acts[full], None, d_pool, d_y)
    return grads


def network_gradients(ctx, images, gt_boxes, gt_hard=None, dontcare=None, cfg=None, seed=0, arena=None, from_layer="conv1_1"):
    """The gradient of the batch's summed model_loss at every tensor of the arena from from_layer on. One ctx.forward over `images` ((n, h, w, 3)
    uint8 BGR, one size) with the ctx option keep_acts = 1 (ValueError if it is 0: the option is the caller's to set); the stored activations
    come back through get_tensor, the conv1_1 input blob is image - PIXEL_MEANS in float32 as the reference forms it; then tail_forward ->
    anchor_targets -> rpn_loss -> tail_backward(want_dx=True), and conv_backward / pool_backward from rpn_conv/3x3 back to from_layer.
    The result is the gradient of the FP32 network at the ctx's stored activations: exact for a CTPN_PREC_FP32 ctx, straight-through for the
    rounded activations of the other precisions. It is tested in fp32. arena: the WEIGHT_FLOATS weights, by default the ones ctx.load_weights
    was given. -> (one dict per image as score_pages returns, {name: gradient array} keyed like arena_views: the conv weights and biases from
    from_layer on, then the ten tail tensors)."""
    return _network_gradients(ctx, images, gt_boxes, gt_hard, dontcare, cfg, seed, arena, from_layer, None)


def _network_gradients(ctx, images, gt_boxes, gt_hard, dontcare, cfg, seed, arena, from_layer, each):
    """network_gradients; each: conv_stack_backward's per-layer hook (tests)"""
    from .targets import STAT_NAMES
    if from_layer not in CONVS:
        raise ValueError("from_layer is one of " + ", ".join(CONVS))
    if ctx.get_option("keep_acts") != 1:
        raise ValueError("network_gradients: the ctx option keep_acts is 0; set keep_acts = 1 so that the forward stores every activation")
    if arena is None:
        arena = getattr(ctx, "arena_weights", None)
        if arena is None:
            raise ValueError("network_gradients: the ctx's weights did not come through load_weights; pass arena=")
    arena = B._f32(arena).reshape(-1)
    if arena.shape[0] != WEIGHT_FLOATS:
        raise ValueError("the arena holds %d floats" % WEIGHT_FLOATS)
    weights = arena_views(arena)
    tail = arena[TAIL_OFFSET:]
    images = np.asarray(images)
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    ctx.forward(images)
    fn, hf, wf = ctx.feat_shape()
    first = CONVS.index(from_layer)
    need = set(CONVS[max(first - 1, 0):])
    for conv, (pool, full) in POOL_BEFORE.items():
        if CONVS.index(conv) >= first:
            need.add(pool)
        if CONVS.index(conv) > first:
            need.add(full)
    acts = {name: np.ascontiguousarray(ctx.get_tensor(name)[:n]) for name in sorted(need)}
    blob = images.astype(np.float32, copy=True)
    blob -= PIXEL_MEANS
    x = acts["rpn_conv/3x3"]
    fwd = tail_forward(x, tail, True, ctx.device_id)
    gts = []
    for g in gt_boxes:
        g = np.asarray(g, np.float32).reshape(-1, np.asarray(g).shape[-1] if np.asarray(g).size else 5)
        if g.shape[1] == 4:
            g = np.concatenate([g, np.ones((g.shape[0], 1), np.float32)], axis=1)
        gts.append(g)
    info = np.array([[h, w, 1.0]] * n, np.float32)
    t = anchor_targets(hf, wf, info, gts, gt_hard, dontcare, cfg, seed, ctx.device_id)
    r = rpn_loss(fwd.heads, t.labels, t.bbox_targets, t.inside_weights, t.outside_weights, True, ctx.device_id)
    bwd = tail_backward(x, tail, fwd.saved, r.d_heads, True, ctx.device_id)
    conv = conv_stack_backward(acts, blob, weights, bwd.d_x, from_layer, ctx.device_id, each)
    grads = collections.OrderedDict()
    for name in CONVS[first:]:
        grads[name + "/weights"], grads[name + "/biases"] = conv[name + "/weights"], conv[name + "/biases"]
    grads.update(tail_views(bwd.d_tail))
    out = []
    for i in range(n):
        out.append({"rpn_cross_entropy": float(r.losses[i, 0]), "rpn_loss_box": float(r.losses[i, 1]), "model_loss": float(r.losses[i, 2]),
                    "kept": int(r.counts[i, 0]), "fg": int(r.counts[i, 1]), "stats": {k: int(v) for k, v in zip(STAT_NAMES, t.stats[i])}})
    return out, grads
