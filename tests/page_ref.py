"""numpy restatement of the page path's host-checkable parts -- the plan, the cut, the merge and greedy NMS -- written from the definitions in
include/ctpn_hip.h ("pages in tiles"), not from the C++: what tests/test_page_plan.py and tests/test_gpu_page.py hold the library to."""
import numpy as np

FILL = np.array([103, 116, 123], np.uint8)      # round(PIXEL_MEANS), BGR
F32 = np.float32


def plan_ok(page_h, page_w, tile_h, tile_w, overlap):
    return (16 <= page_h <= 16384 and 16 <= page_w <= 16384 and tile_h >= 16 and tile_w >= 16 and tile_h % 16 == 0 and tile_w % 16 == 0
            and overlap >= 0 and overlap % 32 == 0 and overlap <= min(tile_h, tile_w) // 2)


def axis(L, T, V):
    """[(origin, valid, own0, own1)] of the tiles along one axis of length L, tile T, overlap V"""
    if L <= T:
        return [(0, L, 0, L)]
    S = T - V
    k = -(-(L - T) // S) + 1
    origins = [j * S for j in range(k)]
    out = []
    for j, o in enumerate(origins):
        own0 = 0 if j == 0 else o + V // 2
        own1 = L if j == k - 1 else origins[j + 1] + V // 2
        out.append((o, min(T, L - o), own0, own1))
    return out


def plan(page_h, page_w, tile_h, tile_w, overlap):
    """-> (tiles (k, 8) int32 {oy, ox, valid_h, valid_w, own_y0, own_y1, own_x0, own_x1}, row-major; (rows, columns))"""
    assert plan_ok(page_h, page_w, tile_h, tile_w, overlap)
    ys, xs = axis(page_h, tile_h, overlap), axis(page_w, tile_w, overlap)
    tiles = [(oy, ox, vh, vw, y0, y1, x0, x1) for oy, vh, y0, y1 in ys for ox, vw, x0, x1 in xs]
    return np.array(tiles, np.int32).reshape(-1, 8), (len(ys), len(xs))


def cut(page, tiles, tile_h, tile_w):
    """the tiles of `tiles` (any rows of a plan) as (n, tile_h, tile_w, 3) uint8: the page's bytes inside it, FILL outside"""
    out = np.empty((len(tiles), tile_h, tile_w, 3), np.uint8)
    out[...] = FILL
    for t, (oy, ox, vh, vw) in enumerate(np.asarray(tiles)[:, :4]):
        out[t, :vh, :vw] = page[oy:oy + vh, ox:ox + vw]
    return out


def merge(tiles, rois, roi_counts, page_h, page_w, min_size):
    """rois (n_tiles, capacity, 5) [score, x1, y1, x2, y2], fp32 -> boxes (m, 4), scores (m,), src (m,) in tile order, then roi order"""
    rois = np.asarray(rois, F32)
    cap = rois.shape[1]
    boxes, scores, src = [], [], []
    half, one, ms = F32(0.5), F32(1.0), F32(min_size)
    for t, (oy, ox, vh, vw, y0, y1, x0, x1) in enumerate(np.asarray(tiles).tolist()):
        for r in range(int(roi_counts[t])):
            s, bx1, by1, bx2, by2 = (F32(v) for v in rois[t, r])
            col = 16 * (int(bx1) >> 4) + ox
            if not (x0 <= col < x1):
                continue
            cy = F32(F32(by1 + by2) * half)
            if not (F32(y0 - oy) <= cy < F32(y1 - oy)):
                continue
            X1, Y1 = F32(bx1 + F32(ox)), F32(by1 + F32(oy))
            X2, Y2 = min(F32(bx2 + F32(ox)), F32(page_w - 1)), min(F32(by2 + F32(oy)), F32(page_h - 1))
            if F32(F32(X2 - X1) + one) < ms or F32(F32(Y2 - Y1) + one) < ms:
                continue
            boxes.append((X1, Y1, X2, Y2))
            scores.append(s)
            src.append(t * cap + r)
    return np.array(boxes, F32).reshape(-1, 4), np.array(scores, F32), np.array(src, np.int32)


def nms(boxes, thresh):
    """greedy NMS over score-sorted rows [x1, y1, x2, y2, ...]: keep positions, ascending. fp32 in devIoU's order: "+1" areas,
    inter / (sa + sb - inter) > thresh."""
    b = np.asarray(boxes, F32)
    n = b.shape[0]
    thr, one, zero = F32(thresh), F32(1.0), F32(0.0)
    area = ((b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)).astype(F32)
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        j = np.arange(i + 1, n)
        if j.size == 0:
            break
        w = np.maximum((np.minimum(b[i, 2], b[j, 2]) - np.maximum(b[i, 0], b[j, 0]) + one).astype(F32), zero)
        h = np.maximum((np.minimum(b[i, 3], b[j, 3]) - np.maximum(b[i, 1], b[j, 1]) + one).astype(F32), zero)
        inter = (w * h).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = (inter / ((area[i] + area[j]).astype(F32) - inter).astype(F32)).astype(F32)
        dead[j[iou > thr]] = True
    return np.array(keep, np.int32)
