"""Independent restatement of the label side of training in vectorised float64 numpy, written from the semantics include/ctpn_hip.h states
("anchor targets and the RPN loss"), not from the device text: the dense overlap of lib/utils/bbox.pyx, the anchor target layer, this
library's splitmix subsampling rule, the RPN loss, and the loss once more in torch float64 so that autograd supplies d model_loss / d heads.
numpy evaluates every ufunc on its own, so no expression below is contracted into an FMA."""
import os

import numpy as np

A = 10
DEFAULT_CFG = (0.3, 0.7, 0.0, 0.5, 300.0, 0.5, 1.0, 0.0, 1.0, 0.0, 1.0, -1.0)
_MASK = (1 << 64) - 1


def base_anchors():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchors.npz"))["anchors"].astype(np.int64)


def all_anchors(hf, wf):
    """(hf * wf * 10, 4) int64: index (y * wf + x) * 10 + a"""
    sx, sy = np.meshgrid(np.arange(wf) * 16, np.arange(hf) * 16)
    shifts = np.stack([sx.ravel(), sy.ravel(), sx.ravel(), sy.ravel()], axis=1)
    return (base_anchors()[None, :, :] + shifts[:, None, :]).reshape(-1, 4)


def overlaps(boxes, query, intersections=False):
    """out[i, j] for boxes (n, 4) and query (k, 4), float64: iw ih / (area_i + area_j - iw ih), or iw ih / area_j"""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    q = np.asarray(query, np.float64).reshape(-1, 4)
    barea = (b[:, 2] - b[:, 0] + 1.0) * (b[:, 3] - b[:, 1] + 1.0)
    qarea = (q[:, 2] - q[:, 0] + 1.0) * (q[:, 3] - q[:, 1] + 1.0)
    iw = np.minimum(b[:, None, 2], q[None, :, 2]) - np.maximum(b[:, None, 0], q[None, :, 0]) + 1.0
    ih = np.minimum(b[:, None, 3], q[None, :, 3]) - np.maximum(b[:, None, 1], q[None, :, 1]) + 1.0
    inter = iw * ih
    with np.errstate(divide="ignore", invalid="ignore"):
        r = inter / qarea[None, :] if intersections else inter / (barea[:, None] + qarea[None, :] - inter)
    return np.where((iw > 0) & (ih > 0), r, 0.0)


def keys(seed, image, anchors):
    """splitmix64's finaliser over seed ^ (image << 32 | anchor), as Python integers -> uint64 array"""
    out = np.empty(len(anchors), np.uint64)
    for i, a in enumerate(anchors):
        z = (int(seed) ^ ((int(image) << 32) | int(a))) & _MASK
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
        out[i] = z ^ (z >> 31)
    return out


def subsample(labels, cls, keep, seed, image):
    """the anchors of class cls beyond the `keep` smallest (key, anchor) pairs become -1"""
    idx = np.nonzero(labels == cls)[0]
    if len(idx) <= keep:
        return
    k = keys(seed, image, idx)
    order = np.lexsort((idx, k))
    labels[idx[order[max(keep, 0):]]] = -1


def anchor_targets(hf, wf, im_info, gt, hard=None, dontcare=None, cfg=None, seed=0, image=0):
    """One image. gt (G, 5) float32. -> dict: labels, labels_presample (int8, hf*wf*10), bbox_targets / inside / outside (float32, (N, 4)),
    max_overlap (float64), argmax (int32), stats (6 ints)."""
    c = DEFAULT_CFG if cfg is None else tuple(float(v) for v in cfg)
    neg, pos, clobber, fgfrac, batch, dc_hi, preclude = c[0], c[1], c[2] != 0, c[3], int(c[4]), c[5], c[6] != 0
    anc = all_anchors(hf, wf)
    N = anc.shape[0]
    im_h, im_w = float(np.float32(im_info[0])), float(np.float32(im_info[1]))
    inside = (anc[:, 0] >= 0) & (anc[:, 1] >= 0) & (anc[:, 2] < im_w) & (anc[:, 3] < im_h)
    ii = np.nonzero(inside)[0]
    an = anc[ii].astype(np.float64)
    g = np.asarray(gt, np.float32).reshape(-1, 5).astype(np.float64)
    G = g.shape[0]
    lab = np.full(len(ii), -1, np.int64)
    tgt = np.zeros((len(ii), 4), np.float64)
    mx = np.zeros(len(ii), np.float64)
    am = np.full(len(ii), -1, np.int64)
    disabled = np.zeros(len(ii), bool)
    ov = None
    if G == 0:
        lab[:] = 0
    elif len(ii):
        ov = overlaps(an, g[:, :4])
        am = ov.argmax(axis=1)
        mx = ov[np.arange(len(ii)), am]
        colmax = ov.max(axis=0)
        is_colmax = (ov == colmax[None, :]).any(axis=1)
        if not clobber:
            lab[mx < neg] = 0
        lab[is_colmax] = 1
        lab[mx >= pos] = 1
        if clobber:
            lab[mx < neg] = 0
        ew, eh = an[:, 2] - an[:, 0] + 1.0, an[:, 3] - an[:, 1] + 1.0
        ex, ey = an[:, 0] + 0.5 * ew, an[:, 1] + 0.5 * eh
        m = np.asarray(gt, np.float32).reshape(-1, 5)[am]      # the reference's gt side of bbox_transform is float32 arithmetic
        one, half = np.float32(1.0), np.float32(0.5)
        gw, gh = m[:, 2] - m[:, 0] + one, m[:, 3] - m[:, 1] + one
        gx, gy = (m[:, 0] + half * gw).astype(np.float64), (m[:, 1] + half * gh).astype(np.float64)
        gw, gh = gw.astype(np.float64), gh.astype(np.float64)
        tgt = np.stack([(gx - ex) / ew, (gy - ey) / eh, np.log(gw / ew), np.log(gh / eh)], axis=1)
    if dontcare is not None and len(dontcare) and len(ii):
        cover = overlaps(np.asarray(dontcare, np.float32).reshape(-1, 4), an, intersections=True)
        s = np.zeros(len(ii), np.float64)
        for row in cover:                      # index order
            s = s + row
        disabled |= s > dc_hi
    if preclude and hard is not None and G and len(ii):
        hsel = np.nonzero(np.asarray(hard).reshape(-1).astype(np.int64) == 1)[0]
        if len(hsel):
            ho = ov[:, hsel]
            disabled |= ho.max(axis=1) >= pos
            disabled[ho.argmax(axis=0)] = True      # every hard box's FIRST maximal anchor
    lab[disabled] = -1
    pre = lab.copy()
    fg0, bg0 = int((lab == 1).sum()), int((lab == 0).sum())
    full = np.full(N, -1, np.int64)
    full[ii] = lab
    if batch > 0:
        num_fg = int(fgfrac * batch)
        subsample(full, 1, num_fg, seed, image)
        subsample(full, 0, batch - int((full == 1).sum()), seed, image)
    out = {"labels": full.astype(np.int8), "labels_presample": np.full(N, -1, np.int8), "bbox_targets": np.zeros((N, 4), np.float32),
           "inside_weights": np.zeros((N, 4), np.float32), "outside_weights": np.zeros((N, 4), np.float32), "max_overlap": np.zeros(N, np.float64),
           "argmax": np.full(N, -1, np.int32)}
    out["labels_presample"][ii] = pre
    out["bbox_targets"][ii] = tgt.astype(np.float32)
    out["max_overlap"][ii] = mx
    out["argmax"][ii] = am
    out["inside_weights"][full == 1] = np.asarray(c[7:11], np.float32)
    out["outside_weights"][full == 1] = 1.0
    out["stats"] = np.array([len(ii), fg0, bg0, int((full == 1).sum()), int((full == 0).sum()), int(disabled.sum())], np.int32)
    return out


def rpn_loss(heads, labels, bbox_targets, inside_weights, outside_weights):
    """One image in float64. heads (cells, ld); labels (cells * 10,); the others (cells * 10, 4).
    -> (rpn_cross_entropy, rpn_loss_box, model_loss, kept, fg)"""
    h = np.asarray(heads, np.float32).astype(np.float64)
    cells = h.shape[0]
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    pred = h[:, :40].reshape(cells * A, 4)
    pair = h[:, 40:60].reshape(cells * A, 2)
    keep = lab != -1
    K, F = int(keep.sum()), int((lab == 1).sum())
    p = pair[keep]
    m = p.max(axis=1)
    lse = m + np.log(np.exp(p[:, 0] - m) + np.exp(p[:, 1] - m))
    ce_n = lse - p[np.arange(K), (lab[keep] == 1).astype(np.int64)]
    ce = float(ce_n.sum() / K) if K else 0.0
    x = np.asarray(inside_weights, np.float64).reshape(-1, 4)[keep] * (pred[keep] - np.asarray(bbox_targets, np.float64).reshape(-1, 4)[keep])
    ax = np.abs(x)
    sl1 = np.where(ax < 1.0 / 9.0, x * x * 0.5 * 9.0, ax - 0.5 / 9.0)
    box = float((np.asarray(outside_weights, np.float64).reshape(-1, 4)[keep] * sl1).sum() / (F + 1.0))
    return ce, box, ce + box, K, F


def rpn_loss_torch(heads, labels, bbox_targets, inside_weights, outside_weights):
    """The same loss in torch float64 -> (model_loss, d model_loss / d heads as a float64 array in the shape of heads; the pad columns 0)"""
    import torch
    h = torch.tensor(np.asarray(heads, np.float32).astype(np.float64), requires_grad=True)
    cells = h.shape[0]
    lab = torch.tensor(np.asarray(labels).reshape(-1).astype(np.int64))
    keep = lab != -1
    K, F = int(keep.sum()), int((lab == 1).sum())
    pred = h[:, :40].reshape(cells * A, 4)[keep]
    pair = h[:, 40:60].reshape(cells * A, 2)[keep]
    ce = (torch.logsumexp(pair, dim=1) - pair.gather(1, (lab[keep] == 1).long()[:, None])[:, 0]).sum() / K if K else h.sum() * 0.0
    t = torch.tensor(np.asarray(bbox_targets, np.float64).reshape(-1, 4))[keep]
    wi = torch.tensor(np.asarray(inside_weights, np.float64).reshape(-1, 4))[keep]
    wo = torch.tensor(np.asarray(outside_weights, np.float64).reshape(-1, 4))[keep]
    x = wi * (pred - t)
    sl1 = torch.where(x.abs() < 1.0 / 9.0, x * x * 0.5 * 9.0, x.abs() - 0.5 / 9.0)
    loss = ce + (wo * sl1).sum() / (F + 1.0)
    loss.backward()
    return float(loss.detach()), h.grad.numpy()
