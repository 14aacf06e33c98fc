"""Generated inputs of the page tests (tests/test_page_plan.py on the CPU, tests/test_gpu_page.py on the device): column-aligned boxes for the
page NMS, tile rois for the merge, the seam scene. Everything comes from a seed; nothing here calls the library."""
import numpy as np

F32 = np.float32
TILE_H, TILE_W, OVERLAP = 64, 96, 32      # the tests' tile: the smallest with more than one tile a side at pages of a few hundred pixels


def column_boxes(seed, r, ncols, span=600.0, crowd=None, equal_scores=0, heights=(8.0, 40.0)):
    """r score-sorted rows [x1, y1, x2, y2, score] on the 16-px column grid: x1 = 16 c, x2 = 16 c + 15 or (one in four) 16 c + 16, y in quarter
    pixels inside [0, span), so that a column's boxes overlap at every IoU. The highest column, ncols - 1, is always used.
    crowd = (column, count): the first `count` rows lie in that column. equal_scores = g > 0: scores come in runs of g equal values."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, ncols, r)
    if r:
        c[rng.integers(0, r)] = ncols - 1
    if crowd:
        c[:crowd[1]] = crowd[0]
        c = c[rng.permutation(r)]
    h = np.round(rng.uniform(heights[0], heights[1], r) * 4) / 4
    y1 = np.round(rng.uniform(0, max(span - heights[1], 1.0), r) * 4) / 4
    wide = rng.integers(0, 4, r) == 0
    b = np.zeros((r, 5), F32)
    b[:, 0] = 16 * c
    b[:, 1] = y1
    b[:, 2] = 16 * c + 15 + wide
    b[:, 3] = y1 + h - 1
    s = np.sort(rng.uniform(0.7, 1.0, r).astype(F32))[::-1]
    if equal_scores:
        s = s[(np.arange(r) // equal_scores) * equal_scores]
    b[:, 4] = s
    return b


def iou32(a, b):
    """fp32 IoU of two boxes in the kernels' order of evaluation"""
    one = F32(1)
    sa = F32(F32(a[2] - a[0] + one) * F32(a[3] - a[1] + one))
    sb = F32(F32(b[2] - b[0] + one) * F32(b[3] - b[1] + one))
    w = max(F32(F32(min(a[2], b[2]) - max(a[0], b[0])) + one), F32(0))
    h = max(F32(F32(min(a[3], b[3]) - max(a[1], b[1])) + one), F32(0))
    inter = F32(w * h)
    return F32(inter / F32(F32(sa + sb) - inter))


def threshold_pairs(thresh, columns=(0, 3, 7)):
    """Per column a pair (A, B) of boxes, A ranked first, whose fp32 IoU is the float below the threshold, the threshold itself, and the float
    above it: B is suppressed in the last case only. B shares A's top; its bottom walks float by float through the crossing. -> rows, and
    per column whether B survives."""
    thr = F32(thresh)
    want = [np.nextafter(thr, F32(0)), thr, np.nextafter(thr, F32(1))]
    rows, survives = [], []
    for k, c in enumerate(columns):
        found = None
        for height in np.arange(40.0, 80.0, 0.25):      # IoU = hb / height, B inside A: the crossing lies within a few floats of thresh x height
            a = np.array([16 * c, 10.0, 16 * c + 15, 10.0 + height - 1], F32)
            y = F32(10.0 + float(thr) * height - 1)
            for _ in range(32):
                y = np.nextafter(y, F32(0))
            for _ in range(64):
                bb = np.array([a[0], a[1], a[2], y], F32)
                if iou32(a, bb) == want[k]:
                    found = (a, bb)
                    break
                y = np.nextafter(y, F32(1e9))
            if found:
                break
        assert found is not None, (thresh, k)
        rows += [found[0], found[1]]
        survives.append(k < 2)
    out = np.zeros((len(rows), 5), F32)
    out[:, :4] = np.array(rows, F32)
    out[:, 4] = np.linspace(0.99, 0.9, len(rows)).astype(F32)
    return out, survives


def seam_scene():
    """A 64 x 352 page, tile 64 x 96, overlap 32 (five tiles in a row): one row of column boxes across the page, as every tile that sees a
    column reports it -- twice in the overlaps. -> page size, per-tile rois (5, capacity, 5) in tile coordinates with their counts, and the same
    set built directly in page coordinates (boxes, scores), one box per page column, distinct scores above 0.9."""
    page_h, page_w = 64, 352
    ncol = page_w // 16
    scores = (0.999 - 0.003 * ((np.arange(ncol) * 7) % ncol)).astype(F32)      # distinct, 0.93 .. 0.999
    y1, y2 = F32(20.25), F32(43.5)
    page_boxes = np.array([[16 * c, y1, 16 * c + 15, y2] for c in range(ncol)], F32)
    origins = [0, 64, 128, 192, 256]
    cap = 16
    rois = np.zeros((len(origins), cap, 5), F32)
    counts = np.zeros(len(origins), np.int32)
    for t, ox in enumerate(origins):
        cols = [c for c in range(ncol) if ox <= 16 * c < ox + TILE_W]
        order = sorted(cols, key=lambda c: -scores[c])      # a tile's rois come in descending score
        for r, c in enumerate(order):
            rois[t, r] = (scores[c], 16 * c - ox, y1, 16 * c - ox + 15, y2)
        counts[t] = len(order)
    return (page_h, page_w), rois, counts, page_boxes, scores


def pitched(page, extra, shift):
    """the page inside a larger byte buffer: rows 3 w + extra bytes apart, the first pixel `shift` bytes into it -> (buffer, view)"""
    h, w, _ = page.shape
    pitch = 3 * w + extra
    buf = np.full(shift + (h - 1) * pitch + 3 * w, 0xEE, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[shift:], shape=(h, w, 3), strides=(pitch, 3, 1))
    view[...] = page
    return buf, view
