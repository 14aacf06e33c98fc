"""Shared by tests/test_jpeg_ragged.py (CPU) and tests/test_gpu_jpeg_ragged.py: the five-file set of the ragged JPEG decode
(ctpn_decode_jpeg_batch_ragged) -- the smallest geometry at which each part can go wrong -- and its expected canvas from Pillow's decode and
the oracle's resize. Test infrastructure only.

    turned h x w   layout / extras               factor    rows in the canvas
    96 x 82        4:2:0                         1         96   (the no-resize branch)
    40 x 41        gray                          2         80   (upscale)
    74 x 123       4:4:4, restart interval 3     82/123    49
    33 x 164       4:2:2                         0.5       16   (16.5 rounds half to even: the ragged minimum)
    66 x 164       4:4:0, EXIF orientation 6     0.5       33   (stored 164 x 66)

Canvas 96 x 82: odd block counts everywhere, a width that is no multiple of 4, IDCT workgroups that straddle images."""
import numpy as np

import util_jpeg as U

WC, HC = 82, 96
SIZES = ((96, 82), (40, 41), (74, 123), (33, 164), (66, 164))          # as ctpn_jpeg_probe reports them (turned)
FACTORS = (1.0, 2.0, 82.0 / 123.0, 0.5, 0.5)
HEIGHTS = (96, 80, 49, 16, 33)
_CACHE = {}


def files():
    """the five files' bytes (generated once per process)"""
    if "files" not in _CACHE:
        _CACHE["files"] = [
            U.encode(U.scene(96, 82, 21), 90, 2),
            U.encode(U.scene(40, 41, 22, gray=True), 85),
            U.encode(U.scene(74, 123, 23), 88, 0, restart_marker_blocks=3),
            U.encode(U.scene(33, 164, 24), 90, 1),
            U.encode_custom(U.scene(164, 66, 25), 1, 2, q=6, orientation=6),
        ]
    return list(_CACHE["files"])


def resized(data, f):
    """cv2.resize(cv2.imread(file), f) by the pins the project has for both: Pillow's decode turned by the EXIF orientation, and the oracle's resize"""
    from oracle import resize_ref
    im = U.cv2_like_bgr(data)
    return im if f == 1.0 else resize_ref.resize_linear(im, f, f)


def canvas_of(images, hc, wc=WC):
    """a zero canvas with image i in rows [0, h_i) of slot i -> (canvas, heights)"""
    canvas = np.zeros((len(images), hc, wc, 3), np.uint8)
    for i, im in enumerate(images):
        assert im.shape[1] == wc and im.shape[0] <= hc
        canvas[i, :im.shape[0]] = im
    return canvas, np.array([im.shape[0] for im in images], np.int32)


def expected(order=None, hc=HC):
    """-> (canvas, heights) of the set in the given order (default 0 .. 4), from Pillow + oracle/resize_ref.py"""
    order = list(range(5)) if order is None else list(order)
    if "resized" not in _CACHE:
        _CACHE["resized"] = [resized(d, f) for d, f in zip(files(), FACTORS)]
    return canvas_of([_CACHE["resized"][i] for i in order], hc)
