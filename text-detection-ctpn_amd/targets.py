"""The label side of training over the C ABI (include/ctpn_hip.h, "anchor targets and the RPN loss"): lib/utils/bbox.pyx's two functions,
anchor_target_layer and Network.build_loss up to model_loss, with the loss's gradient at the heads. Every function takes numpy arrays, or
torch tensors on the device, which go through on_device = 1 with no host copy; score_pages chains a ctx's forward into targets and losses."""
import collections
import ctypes as C

import numpy as np

from . import _binding as B

CFG_NAMES = ("RPN_NEGATIVE_OVERLAP", "RPN_POSITIVE_OVERLAP", "RPN_CLOBBER_POSITIVES", "RPN_FG_FRACTION", "RPN_BATCHSIZE", "DONTCARE_AREA_INTERSECTION_HI",
             "PRECLUDE_HARD_SAMPLES", "RPN_BBOX_INSIDE_WEIGHTS[0]", "RPN_BBOX_INSIDE_WEIGHTS[1]", "RPN_BBOX_INSIDE_WEIGHTS[2]", "RPN_BBOX_INSIDE_WEIGHTS[3]",
             "RPN_POSITIVE_WEIGHT")

AnchorTargets = collections.namedtuple("AnchorTargets", "labels bbox_targets inside_weights outside_weights stats labels_presample max_overlap argmax")
RpnLoss = collections.namedtuple("RpnLoss", "losses counts d_heads")


def target_config_default():
    """ctpn_target_config_default -> the 12 settings, in CFG_NAMES' order"""
    c = np.zeros((12,), np.float64)
    B._check(B.load_library().ctpn_target_config_default(B._ptr(c, C.c_double)))
    return c


def _cfg12(cfg):
    if cfg is None:
        return None
    c = np.ascontiguousarray(cfg, dtype=np.float64).reshape(-1)
    if c.shape[0] != 12:
        raise ValueError("cfg is the 12 values of ctpn_target_config_default")
    return c


def _pairs(boxes, query, intersections, device_id):
    b = np.ascontiguousarray(boxes, dtype=np.float64)
    q = np.ascontiguousarray(query, dtype=np.float64)
    if b.ndim != 2 or q.ndim != 2 or b.shape[1] < 4 or q.shape[1] < 4:
        raise ValueError("boxes and query_boxes are (N, >= 4) arrays")
    b, q = np.ascontiguousarray(b[:, :4]), np.ascontiguousarray(q[:, :4])
    out = np.zeros((b.shape[0], q.shape[0]), np.float64)
    B._check(B.load_library().ctpn_bbox_overlaps(int(device_id), B._ptr(b, C.c_double), int(b.shape[0]), B._ptr(q, C.c_double), int(q.shape[0]),
                                                 B._ptr(out, C.c_double), int(intersections)))
    return out


def bbox_overlaps(boxes, query_boxes, device_id=0):
    """lib/utils/bbox.pyx bbox_overlaps: (N, K) float64, bit-equal to the reference's arithmetic"""
    return _pairs(boxes, query_boxes, 0, device_id)


def bbox_intersections(boxes, query_boxes, device_id=0):
    """lib/utils/bbox.pyx bbox_intersections: (N, K) float64"""
    return _pairs(boxes, query_boxes, 1, device_id)


def _is_torch(x):
    return x is not None and type(x).__module__.split(".")[0] == "torch"


def _dev_ptr(t, dtype, device_id, what):
    """a contiguous torch tensor of `dtype` on cuda:device_id -> its address"""
    if t is None:
        return None
    if not t.is_cuda or t.device.index != int(device_id) or t.dtype != dtype or not t.is_contiguous():
        raise ValueError("%s: a contiguous %s tensor on cuda:%d" % (what, dtype, device_id))
    return C.c_void_p(t.data_ptr()) if t.numel() else None


def _ragged(rows, width, dtype):
    """a list of per-image (k_i, width) arrays -> (flat, offsets)"""
    parts = [np.asarray(r, dtype=dtype).reshape(-1, width) if width > 1 else np.asarray(r, dtype=dtype).reshape(-1) for r in rows]
    offs = np.zeros((len(parts) + 1,), np.int32)
    offs[1:] = np.cumsum([p.shape[0] for p in parts])
    flat = np.ascontiguousarray(np.concatenate(parts, axis=0)) if parts else np.zeros((0, width), dtype)
    return flat, offs


def anchor_targets(hf, wf, im_info, gt_boxes, gt_hard=None, dontcare=None, cfg=None, seed=0, device_id=0, stages=False, gt_offsets=None, dc_offsets=None):
    """ctpn_anchor_targets for n = len(im_info) images on one hf x wf map -> AnchorTargets.

    Host form: gt_boxes a list of n (G_i, 5) arrays, gt_hard a list of n (G_i,) int arrays or None, dontcare a list of n (D_i, 4) arrays or None;
    the results are numpy arrays. Device form: gt_boxes a float32 tensor (total, 5) on cuda:device_id with gt_offsets (n + 1 ints, host),
    gt_hard an int32 tensor (total,), dontcare a float32 tensor (totalD, 4) with dc_offsets; the results are torch tensors on that device and
    nothing tensor-sized crosses to the host. stats is a host array in both. stages: also labels_presample, max_overlap, argmax."""
    lib = B.load_library()
    info = B._f32(im_info).reshape(-1, 3)
    n = int(info.shape[0])
    c12 = _cfg12(cfg)
    stats = np.zeros((n, 6), np.int32)
    i32p, f64p = C.POINTER(C.c_int), C.POINTER(C.c_double)
    on_dev = _is_torch(gt_boxes)
    if on_dev:
        import torch
        if gt_offsets is None:
            raise ValueError("anchor_targets: the device form takes gt_offsets")
        offs = np.ascontiguousarray(gt_offsets, dtype=np.int32).reshape(-1)
        dco = None if dontcare is None else np.ascontiguousarray(dc_offsets, dtype=np.int32).reshape(-1)
        if offs.shape[0] != n + 1 or (dco is not None and dco.shape[0] != n + 1):
            raise ValueError("anchor_targets: offsets are n + 1 ints")
        if int(gt_boxes.shape[0]) != int(offs[-1]) or (gt_hard is not None and int(gt_hard.shape[0]) != int(offs[-1])) or \
                (dontcare is not None and int(dontcare.shape[0]) != int(dco[-1])):
            raise ValueError("anchor_targets: an array's rows differ from its offsets' total")
        dev = torch.device("cuda", int(device_id))
        p_gt = _dev_ptr(gt_boxes, torch.float32, device_id, "gt_boxes")
        p_hard = _dev_ptr(gt_hard, torch.int32, device_id, "gt_hard")
        p_dc = _dev_ptr(dontcare, torch.float32, device_id, "dontcare")
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
        labels, tgt, win, wout = mk((n, hf, wf, 10), torch.float32), mk((n, hf, wf, 40), torch.float32), mk((n, hf, wf, 40), torch.float32), mk((n, hf, wf, 40), torch.float32)
        pre, mx, am = (mk((n, hf, wf, 10), torch.float32), mk((n, hf, wf, 10), torch.float64), mk((n, hf, wf, 10), torch.int32)) if stages else (None, None, None)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
        torch.cuda.current_stream(dev).synchronize()      # the call runs on a stream of its own: what torch queued for these tensors is done first
    else:
        if len(gt_boxes) != n or (gt_hard is not None and len(gt_hard) != n) or (dontcare is not None and len(dontcare) != n):
            raise ValueError("anchor_targets: one entry per image")
        gt, offs = _ragged(gt_boxes, 5, np.float32)
        hard = None if gt_hard is None else _ragged(gt_hard, 1, np.int32)[0]
        if hard is not None and hard.shape[0] != gt.shape[0]:
            raise ValueError("anchor_targets: gt_hard has one flag per box")
        dc, dco = (None, None) if dontcare is None else _ragged(dontcare, 4, np.float32)
        hptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)      # noqa: E731
        p_gt, p_hard, p_dc = hptr(gt), hptr(hard), hptr(dc)
        labels, tgt, win, wout = (np.empty((n, hf, wf, 10), np.float32), np.empty((n, hf, wf, 40), np.float32), np.empty((n, hf, wf, 40), np.float32),
                                  np.empty((n, hf, wf, 40), np.float32))
        pre, mx, am = (np.empty((n, hf, wf, 10), np.float32), np.empty((n, hf, wf, 10), np.float64), np.empty((n, hf, wf, 10), np.int32)) if stages else (None, None, None)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    B._check(lib.ctpn_anchor_targets(int(device_id), n, int(hf), int(wf), B._ptr(info, C.c_float), p_gt, offs.ctypes.data_as(i32p), p_hard, p_dc,
                                     None if dco is None else dco.ctypes.data_as(i32p), None if c12 is None else c12.ctypes.data_as(f64p),
                                     C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), 1 if on_dev else 0, ptr(labels), ptr(tgt), ptr(win), ptr(wout),
                                     stats.ctypes.data_as(i32p), ptr(pre), ptr(mx), ptr(am)))
    return AnchorTargets(labels, tgt, win, wout, stats, pre, mx, am)


def rpn_loss(heads, labels, bbox_targets, inside_weights, outside_weights, want_grad=False, device_id=0):
    """ctpn_rpn_loss -> RpnLoss(losses (n, 3) float64 = rpn_cross_entropy, rpn_loss_box, model_loss; counts (n, 2) = kept, fg; d_heads or None).
    heads: (n, hf, wf, 60 | 64) float32; the four target arrays as anchor_targets returns them. All numpy, or all torch tensors on cuda:device_id
    (d_heads is then a tensor there)."""
    lib = B.load_library()
    on_dev = _is_torch(heads)
    n, hf, wf, ld = (int(v) for v in heads.shape)
    losses, counts = np.zeros((n, 3), np.float64), np.zeros((n, 2), np.int32)
    arrays = (heads, labels, bbox_targets, inside_weights, outside_weights)
    if on_dev:
        import torch
        dev = torch.device("cuda", int(device_id))
        ptrs = [_dev_ptr(t, torch.float32, device_id, "rpn_loss") for t in arrays]
        d = torch.empty((n, hf, wf, ld), dtype=torch.float32, device=dev) if want_grad else None
        p_d = None if d is None else C.c_void_p(d.data_ptr())
        torch.cuda.current_stream(dev).synchronize()
    else:
        arrays = [B._f32(a) for a in arrays]
        ptrs = [a.ctypes.data_as(C.c_void_p) for a in arrays]
        d = np.empty((n, hf, wf, ld), np.float32) if want_grad else None
        p_d = None if d is None else d.ctypes.data_as(C.c_void_p)
    want = (n * hf * wf * 10, n * hf * wf * 40, n * hf * wf * 40, n * hf * wf * 40)
    for a, w in zip(arrays[1:], want):
        if int(np.prod(a.shape)) != w:
            raise ValueError("rpn_loss: the target arrays are (n, hf, wf, 10) and (n, hf, wf, 40)")
    B._check(lib.ctpn_rpn_loss(int(device_id), n, hf, wf, ptrs[0], ld, ptrs[1], ptrs[2], ptrs[3], ptrs[4], 1 if on_dev else 0, B._ptr(losses, C.c_double),
                               B._ptr(counts, C.c_int), p_d))
    return RpnLoss(losses, counts, d)


STAT_NAMES = ("inside", "fg_presample", "bg_presample", "fg", "bg", "disabled")


def score_pages(ctx, images, gt_boxes, gt_hard=None, dontcare=None, cfg=None, seed=0):
    """How good is the ctx's model on labelled pages: one forward over `images` ((n, h, w, 3) uint8 BGR, one size), then the anchor targets of
    the labels (gt_boxes: per image (G_i, 4 | 5) boxes in the images' pixel coordinates) and the RPN loss of the ctx's heads against them.
    Works in every precision: the heads are fp32 in all four. -> one dict per image: rpn_cross_entropy, rpn_loss_box, model_loss, kept, fg,
    and stats (STAT_NAMES)."""
    images = np.asarray(images)
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    ctx.forward(images)
    heads = ctx.get_tensor("heads")
    fn, hf, wf = ctx.feat_shape()
    heads = heads.reshape(fn, hf, wf, -1)[:n]
    gts = []
    for g in gt_boxes:
        g = np.asarray(g, np.float32).reshape(-1, np.asarray(g).shape[-1] if np.asarray(g).size else 5)
        if g.shape[1] == 4:
            g = np.concatenate([g, np.ones((g.shape[0], 1), np.float32)], axis=1)
        gts.append(g)
    info = np.array([[h, w, 1.0]] * n, np.float32)
    t = anchor_targets(hf, wf, info, gts, gt_hard, dontcare, cfg, seed, ctx.device_id)
    r = rpn_loss(heads, t.labels, t.bbox_targets, t.inside_weights, t.outside_weights, False, ctx.device_id)
    out = []
    for i in range(n):
        d = {"rpn_cross_entropy": float(r.losses[i, 0]), "rpn_loss_box": float(r.losses[i, 1]), "model_loss": float(r.losses[i, 2]),
             "kept": int(r.counts[i, 0]), "fg": int(r.counts[i, 1]), "stats": {k: int(v) for k, v in zip(STAT_NAMES, t.stats[i])}}
        out.append(d)
    return out
