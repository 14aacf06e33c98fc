"""The backward pass through the recurrent tail over the C ABI (include/ctpn_hip.h, "the recurrent tail: forward with saved activations,
backward"): the gradient of the RPN loss at the BiLSTM, the lstm_o FC and the two heads -- the arena's last ten tensors, TAIL_FLOATS floats.
tail_forward / tail_backward take numpy arrays, or torch tensors on the device, which go through on_device = 1 with no host copy;
tail_gradients chains a ctx's forward into targets, loss and gradient. The backward of the 14 convs in front of the tail starts at d_x:
conv_grad.py. ctpn/finetune_tail.py is the Momentum branch on the host; the optimisers on the device: solver.py, train.py; the data layers: data_layer.py."""
import collections
import ctypes as C

import numpy as np

from . import _binding as B
from .targets import _dev_ptr, _is_torch, anchor_targets, rpn_loss
from .weights import MANIFEST, WEIGHT_FLOATS

TAIL_FLOATS = 818748
TAIL_OFFSET = WEIGHT_FLOATS - TAIL_FLOATS      # arena[TAIL_OFFSET:] is the tail
TAIL_MANIFEST = [(name, shape, off - TAIL_OFFSET) for name, shape, off in MANIFEST[-10:]]
assert TAIL_MANIFEST[0][2] == 0 and TAIL_OFFSET == 17074496
SAVED_PER_CELL = 2048

TailForward = collections.namedtuple("TailForward", "heads saved")
TailBackward = collections.namedtuple("TailBackward", "d_tail d_x")


def tail_views(flat):
    """name -> array views (TF layout) of a TAIL_FLOATS vector -- the tail weights or their gradient -- keyed like arena_views"""
    a = flat.reshape(-1)
    if int(a.shape[0]) != TAIL_FLOATS:
        raise ValueError("a tail vector holds %d floats" % TAIL_FLOATS)
    return {name: a[off: off + int(np.prod(shape))].reshape(shape) for name, shape, off in TAIL_MANIFEST}


def saved_views(saved, n, hf, wf):
    """the saved block of tail_forward -> {"lstm_out": (n, hf, wf, 256), "lstm_o": (n, hf, wf, 512), "gates": (n, hf, wf, 2, 5, 128)}; gates'
    axis of 5 is i, j, f, o (activated) and the cell state c, its axis of 2 fw, bw"""
    M = n * hf * wf
    s = saved.reshape(-1)
    return {"lstm_out": s[: 256 * M].reshape(n, hf, wf, 256), "lstm_o": s[256 * M: 768 * M].reshape(n, hf, wf, 512),
            "gates": s[768 * M:].reshape(n, hf, wf, 2, 5, 128)}


def _shape4(x, c, what):
    if x.ndim != 4 or int(x.shape[3]) != c:
        raise ValueError("%s is (n, hf, wf, %d)" % (what, c))
    return int(x.shape[0]), int(x.shape[1]), int(x.shape[2])


def _saved_floats(lib, n, hf, wf):
    k = int(lib.ctpn_tail_saved_floats(n, hf, wf))
    if k < 0:
        B._check(-1)
    return k


def tail_forward(x, tail, want_saved=True, device_id=0):
    """ctpn_tail_forward -> TailForward(heads (n, hf, wf, 64), saved flat or None). x: (n, hf, wf, 512) float32 = rpn_conv/3x3's output; tail:
    TAIL_FLOATS float32. Both numpy, or both torch tensors on cuda:device_id (the results are then tensors there)."""
    lib = B.load_library()
    n, hf, wf = _shape4(x, 512, "x")
    ns = _saved_floats(lib, n, hf, wf)
    if _is_torch(x):
        import torch
        dev = torch.device("cuda", int(device_id))
        px, pt = _dev_ptr(x, torch.float32, device_id, "x"), _dev_ptr(tail, torch.float32, device_id, "tail")
        if tail.numel() != TAIL_FLOATS:
            raise ValueError("tail holds %d floats" % TAIL_FLOATS)
        heads = torch.empty((n, hf, wf, 64), dtype=torch.float32, device=dev)
        saved = torch.empty((ns,), dtype=torch.float32, device=dev) if want_saved else None
        ph, ps = C.c_void_p(heads.data_ptr()), None if saved is None else C.c_void_p(saved.data_ptr())
        torch.cuda.current_stream(dev).synchronize()      # the call runs on a stream of its own: what torch queued for these tensors is done first
        on_dev = 1
    else:
        x, tail = B._f32(x), B._f32(tail).reshape(-1)
        if tail.shape[0] != TAIL_FLOATS:
            raise ValueError("tail holds %d floats" % TAIL_FLOATS)
        heads = np.empty((n, hf, wf, 64), np.float32)
        saved = np.empty((ns,), np.float32) if want_saved else None
        px, pt, ph = (a.ctypes.data_as(C.c_void_p) for a in (x, tail, heads))
        ps = None if saved is None else saved.ctypes.data_as(C.c_void_p)
        on_dev = 0
    B._check(lib.ctpn_tail_forward(int(device_id), n, hf, wf, px, pt, on_dev, ph, ps))
    return TailForward(heads, saved)


def tail_backward(x, tail, saved, d_heads, want_dx=False, device_id=0, out=None):
    """ctpn_tail_backward -> TailBackward(d_tail TAIL_FLOATS (tail_views names it), d_x (n, hf, wf, 512) or None). saved: tail_forward's block
    for the same x and tail; d_heads: (n, hf, wf, 64), columns 60..63 ignored (rpn_loss(want_grad=True).d_heads of 64-wide heads). out: a
    device tensor of TAIL_FLOATS floats d_tail is written to (a view of a flat gradient vector)."""
    lib = B.load_library()
    n, hf, wf = _shape4(x, 512, "x")
    ns = _saved_floats(lib, n, hf, wf)
    if _shape4(d_heads, 64, "d_heads") != (n, hf, wf):
        raise ValueError("d_heads is (n, hf, wf, 64) for x's n, hf, wf")
    if _is_torch(x):
        import torch
        dev = torch.device("cuda", int(device_id))
        ptrs = [_dev_ptr(t, torch.float32, device_id, w) for t, w in ((x, "x"), (tail, "tail"), (saved, "saved"), (d_heads, "d_heads"))]
        if tail.numel() != TAIL_FLOATS or saved.numel() != ns:
            raise ValueError("tail holds %d floats, saved %d" % (TAIL_FLOATS, ns))
        if out is None:
            d_tail = torch.empty((TAIL_FLOATS,), dtype=torch.float32, device=dev)
        else:
            d_tail = out
            _dev_ptr(d_tail, torch.float32, device_id, "out")
            if d_tail.dim() != 1 or d_tail.numel() != TAIL_FLOATS:
                raise ValueError("tail_backward: out holds %d floats" % TAIL_FLOATS)
        d_x = torch.empty((n, hf, wf, 512), dtype=torch.float32, device=dev) if want_dx else None
        pg, pdx = C.c_void_p(d_tail.data_ptr()), None if d_x is None else C.c_void_p(d_x.data_ptr())
        torch.cuda.current_stream(dev).synchronize()
        on_dev = 1
    else:
        if out is not None:
            raise ValueError("tail_backward: out= goes with device tensors")
        x, tail, saved, d_heads = B._f32(x), B._f32(tail).reshape(-1), B._f32(saved).reshape(-1), B._f32(d_heads)
        if tail.shape[0] != TAIL_FLOATS or saved.shape[0] != ns:
            raise ValueError("tail holds %d floats, saved %d" % (TAIL_FLOATS, ns))
        d_tail = np.empty((TAIL_FLOATS,), np.float32)
        d_x = np.empty((n, hf, wf, 512), np.float32) if want_dx else None
        ptrs = [a.ctypes.data_as(C.c_void_p) for a in (x, tail, saved, d_heads)]
        pg, pdx = d_tail.ctypes.data_as(C.c_void_p), None if d_x is None else d_x.ctypes.data_as(C.c_void_p)
        on_dev = 0
    B._check(lib.ctpn_tail_backward(int(device_id), n, hf, wf, ptrs[0], ptrs[1], ptrs[2], ptrs[3], on_dev, pg, pdx))
    return TailBackward(d_tail, d_x)


def debug_tail_bptt(d_lstm_out, gates, tail, device_id=0):
    """ctpn_debug_tail_bptt (test hook): the backward recurrence alone. d_lstm_out (rows, T, 256), gates (rows, T, 2, 5, 128) -> d_pre (rows, T, 1024)"""
    d, g, t = B._f32(d_lstm_out), B._f32(gates), B._f32(tail).reshape(-1)
    rows, T = int(d.shape[0]), int(d.shape[1])
    if d.shape != (rows, T, 256) or g.shape != (rows, T, 2, 5, 128) or t.shape[0] != TAIL_FLOATS:
        raise ValueError("debug_tail_bptt: d_lstm_out (rows, T, 256), gates (rows, T, 2, 5, 128), tail TAIL_FLOATS")
    out = np.empty((rows, T, 1024), np.float32)
    B._check(B.load_library().ctpn_debug_tail_bptt(int(device_id), rows, T, B._ptr(d, C.c_float), B._ptr(g, C.c_float), B._ptr(t, C.c_float), B._ptr(out, C.c_float)))
    return out


def tail_gradients(ctx, images, gt_boxes, gt_hard=None, dontcare=None, cfg=None, seed=0, tail=None):
    """The gradient of the batch's summed model_loss at the tail weights: ctx.forward over `images` ((n, h, w, 3) uint8 BGR, one size), the
    ctx's rpn_conv/3x3, tail_forward on the ctx's own tail weights, anchor_targets of the labels, rpn_loss with its gradient, tail_backward.
    Works in every ctx precision: the tail is recomputed in fp32 from the ctx's features, so the loss and the gradient belong to each other.
    tail: the TAIL_FLOATS weights, by default the ones ctx.load_weights was given. -> (one dict per image as score_pages returns, {name:
    gradient array} keyed like arena_views)."""
    from .targets import STAT_NAMES
    if tail is None:
        tail = getattr(ctx, "tail_weights", None)
        if tail is None:
            raise ValueError("tail_gradients: the ctx's weights did not come through load_weights; pass tail=arena[TAIL_OFFSET:]")
    images = np.asarray(images)
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    ctx.forward(images)
    fn, hf, wf = ctx.feat_shape()
    x = np.ascontiguousarray(ctx.get_tensor("rpn_conv/3x3").reshape(fn, hf, wf, 512)[:n])
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
    bwd = tail_backward(x, tail, fwd.saved, r.d_heads, False, ctx.device_id)
    out = []
    for i in range(n):
        out.append({"rpn_cross_entropy": float(r.losses[i, 0]), "rpn_loss_box": float(r.losses[i, 1]), "model_loss": float(r.losses[i, 2]),
                    "kept": int(r.counts[i, 0]), "fg": int(r.counts[i, 1]), "stats": {k: int(v) for k, v in zip(STAT_NAMES, t.stats[i])}})
    return out, tail_views(bwd.d_tail)


def momentum_step(tail, velocity, grad, lr, momentum, clip=10.0):
    """One step of lib/fast_rcnn/train.py:94-109's Momentum branch on flat float32 vectors: tf.clip_by_global_norm(grads, 10.0), then
    tf.train.MomentumOptimizer (accum = momentum * accum + grad; var -= lr * accum). -> (tail, velocity, the global norm before clipping)"""
    g = np.asarray(grad, np.float32).reshape(-1)
    norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    if norm > clip:
        g = g * np.float32(clip / norm)
    velocity = np.float32(momentum) * velocity + g
    return (tail - np.float32(lr) * velocity).astype(np.float32), velocity.astype(np.float32), norm
