"""TEST INFRASTRUCTURE: the cases of the canvas-pack tests (tests/test_canvas_pack.py on the CPU, tests/test_gpu_canvas_pack.py on the GPU).

A case is a ragged canvas n x hc x wc x 3 and n source images (h, w, f): image i resized by f_i fills rows [0, dh_i) of slot i, zeros
below. The shapes are the smallest at which canvas_pack_kernel (csrc/canvas_pack_dev.h) can go wrong:
  wc in 17, 18, 19, 20   every residue mod 4: a thread's four pixels straddle rows and, at slot seams, images
  hc in 16, 23           16: every image fills its slot (no zero rows); 23: heights 16, 23 and in between
  n  in 1, 2, 5          n x hc x wc is a multiple of 4 in some cases and not in others (the byte-wise tail)
and the images of a case are drawn in turn from the kinds that can map to (hc, wc) at all:
  copy       f = 1: (dh, wc) copied
  narrow     a source 1, 2 and 3 pixels wide and high, f = wc / w: every clamp of rs_coord. With ONE factor for both axes such a source
             maps to a height of about wc >= 17, so these exist for hc = 23 only; at hc = 16 the search below finds none (a height of 16
             beside a width of 17 .. 20 needs h < w, and then w <= 3 leaves no h whose h * f rounds to 16)
  down43     a source 43 wide, f = wc / 43: a factor that does not terminate in binary
  up / down  whatever else a search over small (h, w) finds for a wanted height: 16, hc, or in between
Every (h, w, f) is checked against oracle/resize_ref.out_dim here, so a case cannot ask for a width the library refuses.
Source bytes are random over 0 .. 255; `expected` is the oracle's canvas, computed once per case."""
import functools

import numpy as np

from oracle import resize_ref

WCS = (17, 18, 19, 20)
HCS = (16, 23)
NS = (1, 2, 5)
PITCH_EXTRA = (0, 1, 7)          # device / host-program sources at pitch 3 w + this


def dims(h, w, f):
    """what the library maps (h, w) to by f (ctpn_resize_dims; f == 1: the size itself)"""
    return (h, w) if f == 1.0 else (resize_ref.out_dim(h, f), resize_ref.out_dim(w, f))


def find(wc, w, want):
    """(h, w, f) with f near wc / w whose width maps to wc and whose height maps into `want` (a range), or None"""
    for e in (0.0, 0.004, -0.004, 0.011, -0.011):
        f = wc / float(w) * (1.0 + e)
        if f == 1.0 or resize_ref.out_dim(w, f) != wc:
            continue
        for h in range(1, 96):
            if resize_ref.out_dim(h, f) in want:
                return (h, w, f)
    return None


@functools.lru_cache(maxsize=None)
def pool(hc, wc):
    """the kinds of image that exist for (hc, wc): a list of (kind, (h, w, f))"""
    out = [("copy16", (16, wc, 1.0))] + ([("copy_hc", (hc, wc, 1.0))] if hc > 16 else [])
    for w in (1, 2, 3):
        got = find(wc, w, range(16, hc + 1))
        if got:
            out.append(("narrow%d" % w, got))
    for name, want in (("down43_16", range(16, 17)), ("down43_hc", range(hc, hc + 1))):
        got = find(wc, 43, want)
        assert got, (name, hc, wc)
        if got not in [g for _, g in out]:      # (hc = 16: the two heights are one)
            out.append((name, got))
    mid = range(17, hc) if hc > 17 else range(16, 17)
    for name, ws, want in (("up_mid", range(4, wc), mid), ("up_hc", range(5, wc), range(hc, hc + 1)), ("down_mid", range(wc + 1, 3 * wc), mid)):
        for w in ws:
            got = find(wc, w, want)
            if got:
                if got not in [g for _, g in out]:
                    out.append((name, got))
                break
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, hc, wc, ((h, w, f), ...), (kind, ...))]: every (wc, hc, n), the images taken in turn from the pool so that every kind is used"""
    out = []
    for hc in HCS:
        k = 0                                      # runs on from width to width (+ 1), so that n = 1 does not always meet the pool's first kind
        for wc in WCS:
            p = pool(hc, wc)
            k += 1
            for n in NS:
                pick = [p[(k + j) % len(p)] for j in range(n)]
                k += n
                out.append(("wc%d_hc%d_n%d" % (wc, hc, n), hc, wc, tuple(g for _, g in pick), tuple(kind for kind, _ in pick)))
    return out


def names():
    return [c[0] for c in cases()]


def case(name):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def _data(name):
    _, hc, wc, imgs, _ = case(name)
    rng = np.random.RandomState(sum(map(ord, name)) * 7919 % (2 ** 31))
    srcs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w, _ in imgs]
    for s in srcs:
        s.setflags(write=False)
    canvas = np.zeros((len(imgs), hc, wc, 3), np.uint8)
    heights = []
    for i, ((h, w, f), s) in enumerate(zip(imgs, srcs)):
        r = s if f == 1.0 else resize_ref.resize_linear(s, f, f)
        assert r.shape[1] == wc and 16 <= r.shape[0] <= hc, (name, i, r.shape)
        canvas[i, : r.shape[0]] = r
        heights.append(r.shape[0])
    canvas.setflags(write=False)
    return srcs, canvas, np.asarray(heights, np.int32)


def sources(name):
    """the case's source images: read-only (h, w, 3) uint8 arrays"""
    return _data(name)[0]


def expected(name):
    """(canvas, heights) of the case by oracle/resize_ref.py: what lib/utils/blob.py im_list_to_canvas makes of the individually resized images"""
    return _data(name)[1], _data(name)[2]


def factors(name):
    return [f for _, _, f in case(name)[3]]


def pitched(src, extra, front=0, guard=0, fill=0xA5):
    """src in a flat buffer at byte offset guard + front, rows 3 w + extra bytes apart, `guard` bytes of `fill` behind the last pixel too; every
    byte that is not a pixel is `fill`. -> (buffer, offset of the first pixel, pitch)"""
    h, w, _ = src.shape
    pitch = 3 * w + extra
    used = (h - 1) * pitch + 3 * w
    buf = np.full((guard + front + used + guard,), fill, np.uint8)
    for y in range(h):
        o = guard + front + y * pitch
        buf[o: o + 3 * w] = src[y].reshape(-1)
    return buf, guard + front, pitch
