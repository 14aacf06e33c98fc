"""TEST INFRASTRUCTURE ONLY: the definition of a text-line crop (include/ctpn_hip.h, ctpn_crop_lines) restated in numpy -- float64 widths and
sample positions, a float32 fraction, cv2.resize's 11-bit integer formula with the border replicated on both axes. Written from the
definition, not from csrc/crop_pixel.h: tests/test_crop.py holds that source text (compiled with g++) against this file bit for bit, and
tests/test_gpu_crop.py the kernel.

A record is [x0,y0,x1,y1,x2,y2,x3,y3,score]: P0 top-left, P1 top-right, P2 bottom-left, P3 bottom-right."""
import math

import numpy as np


def width(rec, crop_h, max_w):
    x0, y0, x1, y1, x2, y2, x3, y3 = [float(v) for v in rec[:8]]

    def length(dx, dy):
        return math.sqrt(dx * dx + dy * dy)
    top, bottom = length(x1 - x0, y1 - y0), length(x3 - x2, y3 - y2)
    left, right = length(x2 - x0, y2 - y0), length(x3 - x1, y3 - y1)
    wlen, hlen = (top + bottom) / 2, (left + right) / 2
    if not hlen >= 1.0:
        hlen = 1.0
    wc = int(np.rint(np.float64(crop_h) * wlen / hlen))          # np.rint: half to even
    return min(max(wc, 1), max_w)


def positions(rec, wc, crop_h):
    """-> X, Y: (crop_h, wc) float64 source positions of the output pixels"""
    q = np.asarray(rec[:8], np.float64)
    s = ((np.arange(wc, dtype=np.float64) + 0.5) / np.float64(wc))[None, :]
    t = ((np.arange(crop_h, dtype=np.float64) + 0.5) / np.float64(crop_h))[:, None]
    tx, bx = q[0] + s * (q[2] - q[0]), q[4] + s * (q[6] - q[4])
    ty, by = q[1] + s * (q[3] - q[1]), q[5] + s * (q[7] - q[5])
    return tx + t * (bx - tx) - 0.5, ty + t * (by - ty) - 0.5


def _axis(pos, dim):
    f = pos.astype(np.float32)
    fl = np.floor(f)
    f = (f - fl).astype(np.float32)
    i0 = fl.astype(np.int64)
    lo, hi = i0 < 0, i0 >= dim - 1
    i0 = np.where(lo, 0, np.where(hi, dim - 1, i0))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    i1 = np.minimum(i0 + 1, dim - 1)

    def short(v):
        return np.clip(np.rint(v.astype(np.float32)), -32768, 32767).astype(np.int64)
    return i0, i1, short((np.float32(1) - f) * np.float32(2048)), short(f * np.float32(2048))


def sample(img, X, Y):
    """img (h, w, 3) uint8 at the float64 positions X, Y (same shape) -> (..., 3) uint8"""
    h, w = img.shape[:2]
    x0, x1, a0, a1 = _axis(X, w)
    y0, y1, b0, b1 = _axis(Y, h)
    src = img.astype(np.int64)
    S0 = src[y0, x0] * a0[..., None] + src[y0, x1] * a1[..., None]
    S1 = src[y1, x0] * a0[..., None] + src[y1, x1] * a1[..., None]
    v = (((b0[..., None] * (S0 >> 4)) >> 16) + ((b1[..., None] * (S1 >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def crop_line(img, rec, crop_h, max_w, pad=0, wc=None):
    """-> ((crop_h, max_w, 3) uint8, Wc); wc overrides the record's own width (the tests that need a given width)"""
    wc = width(rec, crop_h, max_w) if wc is None else wc
    out = np.full((crop_h, max_w, 3), pad, np.uint8)
    X, Y = positions(rec, wc, crop_h)
    out[:, :wc] = sample(img, X, Y)
    return out, wc


def crop_lines(images, recs, crop_h, max_w, pad=0):
    """images (n, h, w, 3); recs: one (M_i, 9) array per image -> ((total, crop_h, max_w, 3) uint8, (total,) int32 widths)"""
    crops, widths = [], []
    for img, rr in zip(images, recs):
        for rec in np.asarray(rr, np.float64).reshape(-1, 9):
            c, wc = crop_line(img, rec, crop_h, max_w, pad)
            crops.append(c)
            widths.append(wc)
    if not crops:
        return np.zeros((0, crop_h, max_w, 3), np.uint8), np.zeros((0,), np.int32)
    return np.stack(crops), np.array(widths, np.int32)


def bilinear_exact(img, X, Y):
    """the float64 bilinear value at (X, Y) with the border replicated, before rounding: an oracle independent of the fixed-point formula"""
    h, w = img.shape[:2]
    Xc, Yc = np.clip(X, 0, w - 1), np.clip(Y, 0, h - 1)
    x0, y0 = np.minimum(np.floor(Xc).astype(np.int64), w - 1), np.minimum(np.floor(Yc).astype(np.int64), h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (Xc - x0)[..., None], (Yc - y0)[..., None]
    src = img.astype(np.float64)
    return (src[y0, x0] * (1 - fx) + src[y0, x1] * fx) * (1 - fy) + (src[y1, x0] * (1 - fx) + src[y1, x1] * fx) * fy
