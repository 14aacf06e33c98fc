"""Shared by tests/test_out_ragged.py (CPU) and tests/test_gpu_out_ragged.py: the ragged canvas, scales and text lines of the ragged output
stage (ctpn_write_annotated_files_ragged, ctpn_crop_lines_ragged, ctpn_write_line_crops_ragged). Test infrastructure only.

The canvas is the set of tests/jpeg_ragged_cases.py: 96 x 82 slots, heights (96, 80, 49, 16, 33) -- a width that is no multiple of 4, the
ragged minimum of 16 rows, a full-height slot. As a HOST canvas its dead rows hold the sentinel 0xAB: a read below an image changes bytes.

    slot  rows  scale    written at      lines
    0     96    1        96 x 82         green, red, green (two colour changes: two barriers), one thinner than 5 px (not drawn, cropped)
    1     80    0.5      160 x 164       none
    2     49    82/123   74 x 123        one across the image's bottom row, one wholly below the image inside the canvas, one a pixel wide
    3     16    2        8 x 41          one squeezed to max_w, one drawn
    4     33    1        33 x 82         red, then green across the bottom row (an unresized slot behind resized ones)
"""
import numpy as np

import jpeg_ragged_cases as JR

HC, WC = JR.HC, JR.WC
HEIGHTS = JR.HEIGHTS
SCALES = (1.0, 0.5, 82.0 / 123.0, 2.0, 1.0)
SENTINEL = 0xAB
CROP_H, MAX_W, PAD = 32, 64, 77


def line(x, y, ws, hs, score, slant=0.0, shear=0.0):
    return [x, y, x + ws, y + slant, x + shear, y + hs, x + ws + shear, y + hs + slant, score]


# (ctpn_draw_boxes skips a line with |x0 - y0| < 5 or |y1 - x0| < 5 -- the reference's test for a thin one)
LINES = (
    [line(10.0, 30.0, 60.0, 12.0, 0.95, slant=2.0), line(5.0, 60.0, 70.0, 10.0, 0.5), line(40.0, 70.0, 30.0, 14.0, 0.92, slant=-3.0),
     line(20.0, 22.0, 40.0, 3.0, 0.95)],
    [],
    [line(8.0, 40.0, 60.0, 20.0, 0.91), line(10.0, 60.0, 50.0, 12.0, 0.3), line(7.0, 20.0, 0.25, 8.0, 0.9)],
    [line(1.0, 2.0, 79.0, 4.0, 0.95), line(12.0, 3.0, 50.0, 9.0, 0.95, shear=1.5)],
    [line(30.0, 10.0, 45.0, 15.0, 0.89, shear=2.0), line(2.0, 25.0, 70.0, 16.0, 0.93, slant=1.0)],
)


def recs():
    """one (M_i, 9) float64 array per image"""
    return [np.array(r, np.float64).reshape(-1, 9) for r in LINES]


def host_canvas(order=None):
    """-> (canvas with SENTINEL in the dead rows, heights int32) of the set in the given order (default 0 .. 4); a fresh array every call"""
    order = list(range(5)) if order is None else list(order)
    canvas, heights = JR.expected(order)
    canvas = canvas.copy()
    for i, h in enumerate(heights):
        canvas[i, h:] = SENTINEL
    return canvas, heights


def lone(canvas, heights, i):
    """image i alone: rows [0, heights[i]) of slot i, a contiguous copy"""
    return np.ascontiguousarray(canvas[i, :heights[i]])


def out_dims(h, w, scale):
    """the size image (h, w) is written at: no resize at scale 1, else cvRound of the size times 1 / scale"""
    from oracle import resize_ref
    f = 1.0 / scale
    return (h, w) if f == 1.0 else (resize_ref.out_dim(h, f), resize_ref.out_dim(w, f))
