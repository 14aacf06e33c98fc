"""Generated inputs for the text-line tail (lines_prep_kernel -> connector NMS 0.2 -> connect_kernel / connect_lines): text lines laid on the
16-px anchor grid, as rois [score, x1, y1, x2, y2] at network resolution in descending score order, at most 1000 per image -- what the
proposal layer hands to the tail. Pure numpy, seeded (of the oracle, make_scene takes nothing; the oracle_* helpers below call it); the committed CASES are what tests/test_lines_scenes.py (CPU: the conditions the
list must meet, and the mutants it must catch) and tests/test_gpu_text_line_tail.py (the device against the oracle) run on.

A scene is built to reach what whole-network runs with random weights do not:
  * scores: nine in ten from 15 fixed fp32 levels in (0.72, 1.0] (ties inside a column and along a chain are the rule), the rest at or below
    0.7 -- the value 0.7f itself among them -- so the `score > 0.7` prefix ends inside the list;
  * geometry: a start and end column, a centre height, a slope of either sign, quarter-pixel jitter per column, one or two proposals per
    column and a few missing columns; the second proposal of a column sits around the 0.2 IoU of the connector's NMS (both sides of it) or
    well inside it;
  * some columns fork into two boxes with one score that both meet their neighbours: the successor search's tie rule decides the chain;
  * some columns shrink to about 0.7 of the line's height and slide to about 0.7 vertical overlap: the two thresholds of meet_v_iou;
  * "mixed" scenes carry one line for each reason filter_boxes drops a line: 3 columns of tall boxes (width / height <= 0.5), 2 columns
    (width <= 32) and a long line of scores below 0.9.
"""
import collections

import numpy as np

from oracle import postproc as P

LEVELS = np.linspace(0.73, 1.0, 15).astype(np.float32)          # the fixed score levels: 0.73, 0.749.., .. 0.98.., 1.0
LOW = np.array([0.7, 0.7, 0.69, 0.55, 0.31], np.float32)        # at or below TEXT_PROPOSALS_MIN_SCORE (0.7f itself: `>` against `>=`)

Scene = collections.namedtuple("Scene", "name rois h w scale")
Case = collections.namedtuple("Case", "name seed h w scale lines kind")

# name, seed, h, w, scale, lines, kind. "mixed": the recipe above; "full": no low scores, cut at exactly 1000 rois; "long": every line spans the
# whole width with one proposal in every column; "low": nothing above 0.7; "empty": no rois at all; "deep": `lines` disjoint boxes 2 px apart in
# ONE column with strictly descending scores (all kept), and a lower-scored near-duplicate (IoU 0.875 with its original, disjoint from every
# other box) of four in five of them, in shuffled score order: each is suppressed by one kept box alone, at every depth of the kept list.
CASES = [
    Case("g0", 1, 600, 900, 1.0, 12, "mixed"),                  # g0 .. g5: one geometry, the batch tests take them together
    Case("g1", 2, 600, 900, 1.25, 20, "mixed"),
    Case("g2", 3, 600, 900, 1.8018018, 14, "mixed"),
    Case("g3", 4, 600, 900, 1.0, 16, "mixed"),
    Case("g4", 5, 600, 900, 2.0, 18, "mixed"),
    Case("g5", 6, 600, 900, 1.0, 9, "mixed"),
    Case("wide", 7, 608, 1216, 1.0, 36, "mixed"),               # more than 512 kept proposals
    Case("full", 8, 608, 1216, 1.0, 80, "full"),                # exactly 1000 rois, all above 0.7
    Case("zoom", 9, 352, 1000, 1.8018018, 10, "mixed"),
    Case("strip", 10, 256, 4096, 1.0, 3, "long"),               # chains longer than 128 on the widest image the column NMS takes
    Case("beyond", 11, 128, 4400, 1.0, 2, "long"),              # chains longer than 256; 275 columns: past the column NMS's 256
    Case("big_scale", 12, 352, 1000, 4.5, 10, "mixed"),         # scale above 4: the generic NMS kernel
    Case("low", 13, 600, 900, 1.0, 4, "low"),
    Case("empty", 14, 600, 900, 1.0, 0, "empty"),
    Case("deep", 15, 608, 64, 1.0, 300, "deep"),                # one column that keeps 300 boxes: the column NMS's kept list past its LDS capacity
]
BATCH_NAMES = ["g0", "g1", "g2", "g3", "g4", "g5"]
# not in CASES (the oracle, like the reference, raises IndexError on it): g0's rois with a scale below 1, boxes / scale beyond the image
OUTSIDE = Case("outside", 1, 600, 900, 0.5, 12, "mixed")


def _line(rng, rows, c0, c1, cy, hh, slope, levels, second=0.5, missing=0.06, wobble=True):
    """one text line: columns c0 .. c1 (inclusive), centre height cy at c0, box height hh, slope in px per column"""
    for c in range(c0, c1 + 1):
        if c not in (c0, c1) and rng.random() < missing:
            continue
        yc = cy + slope * (c - c0) + rng.integers(-6, 7) * 0.25
        h = hh
        if wobble and c not in (c0, c1) and rng.random() < 0.06:
            # a fork: two boxes of 0.72 of the line's height, one over its upper and one over its lower edge, with ONE score. Both survive
            # the NMS (IoU 0.12) and both meet their neighbours (0.8 of their height overlaps): a tied maximum inside a column
            h, sc = np.floor(hh * 0.72) + 0.5, rng.choice(levels)
            for y1 in (yc - hh / 2.0 - 0.2 * h, yc + hh / 2.0 - 0.8 * h):
                rows.append([sc, 16.0 * c, y1, 16.0 * c + 15.0, y1 + h - 1.0])
            continue
        if wobble and rng.random() < 0.15:
            # around MIN_SIZE_SIM: 0.7 of the line's height, half a pixel either way; and slid to around MIN_V_OVERLAPS of the smaller box
            h = np.floor(hh * 0.7) + rng.integers(-1, 2) * 0.5
            yc += rng.choice([-1.0, 1.0]) * ((hh - h) / 2.0 + 0.3 * h + rng.integers(-1, 2) * 0.5)
        y1 = yc - h / 2.0
        rows.append([rng.choice(levels), 16.0 * c, y1, 16.0 * c + 15.0, y1 + h - 1.0])
        if rng.random() < second:
            if rng.random() < 0.5:
                dy = np.round(2.0 / 3.0 * h) + rng.integers(-2, 3) * 0.5      # IoU (h - dy) / (h + dy) around 0.2
            else:
                dy = float(rng.integers(0, 4))                                # far above it: one of the two goes
            rows.append([rng.choice(levels), 16.0 * c, y1 + dy, 16.0 * c + 15.0, y1 + dy + h - 1.0])


def make_scene(case):
    """-> Scene: rois (R, 5) float32 [score, x1, y1, x2, y2], R <= 1000, descending score (ties in the order a stable sort leaves them)"""
    name, seed, h, w, scale, lines, kind = case
    rng = np.random.default_rng(seed)
    ncol = w // 16
    rows = []
    top, mid = LEVELS[-5:], LEVELS[:9]                           # line means above / below LINE_MIN_SCORE (0.9)
    if kind in ("mixed", "full", "low"):
        hh_max = 34 if h >= 500 else 22
        band_h = hh_max + 26
        nbands = max(1, (h - 20) // band_h)
        gap = int(np.ceil(51.0 * scale / 16.0)) + 1             # columns that put two lines of a band more than MAX_HORIZONTAL_GAP apart
        cursor = [int(rng.integers(0, 4)) for _ in range(nbands)]
        specials = ["tall", "short", "dim"] if kind == "mixed" else []
        for li in range(lines):
            band = li % nbands
            c0 = cursor[band]
            if c0 + 4 >= ncol:
                band = int(np.argmin(cursor)); c0 = cursor[band]
                if c0 + 4 >= ncol:
                    break
            what = specials.pop(0) if specials and li >= 2 else "plain"
            length = int(rng.integers(5, max(6, ncol // 2)))
            hh = float(rng.integers(12, hh_max + 1))
            levels = top
            slope = float(rng.choice([-1.0, 1.0]) * rng.choice([0.0, 0.1, 0.25, 0.4]))
            if what == "tall":
                length, hh, slope = 3, 2.0 * band_h + 24.0 * scale, 0.0
            elif what == "short":
                length = 2
            elif what == "dim":
                levels = mid
            elif rng.random() < 0.2:
                levels = LEVELS[6:]                                # means near 0.9
            c1 = min(ncol - 1, c0 + length - 1)
            reach = abs(slope) * (c1 - c0)
            cy = 14 + band * band_h + band_h / 2.0 + (reach / 2.0 if slope < 0 else -reach / 2.0)
            cy = min(max(cy, hh / 2.0 + 4), h - hh / 2.0 - 5)
            _line(rng, rows, c0, c1, cy, hh, slope, levels, second=0.95 if kind == "full" else 0.5, wobble=what == "plain")
            cursor[band] = c1 + gap + int(rng.integers(0, 3))
    elif kind == "long":
        band_h = h // max(lines, 1)
        for li in range(lines):
            hh = float(rng.integers(12, min(28, band_h - 14)))
            slope = float(rng.choice([-1.0, 1.0]) * rng.choice([0.01, 0.02, 0.03]))
            cy = band_h * li + band_h / 2.0 - slope * ncol / 2.0
            _line(rng, rows, 0, ncol - 1, cy, hh, slope, LEVELS[-6:], second=0.3 if li == 0 else 0.0, missing=0.02 if li % 2 else 0.0, wobble=False)
    elif kind == "deep":
        ys = 2.0 * np.arange(lines)
        rows += [[sc, 32.0, y, 47.0, y + 1.0] for sc, y in zip(np.linspace(0.99, 0.80, lines), ys)]
        dup = rng.permutation(ys[np.arange(lines) % 5 != 0])
        rows += [[sc, 32.0, y, 47.0, y + 0.75] for sc, y in zip(np.linspace(0.79, 0.71, dup.size), dup)]
    r = np.array(rows, np.float32).reshape(-1, 5)
    n = r.shape[0]
    if kind == "low":
        r[:, 0] = rng.choice(LOW, n)
    elif kind not in ("full", "deep") and n:
        low = rng.random(n) < (0.03 if kind == "long" else 0.1)       # (a long line must not lose three columns in a row)
        r[low, 0] = rng.choice(LOW, int(low.sum()))
    r[:, 2] = np.maximum(r[:, 2], 0)
    r[:, 4] = np.minimum(r[:, 4], h - 1)
    r = r[rng.permutation(n)]                                     # ties then fall in an order unrelated to the geometry
    r = r[np.argsort(-r[:, 0], kind="stable")][:1000]            # (a sort of its own: the oracle's ordering is what the scenes test)
    return Scene(name, np.ascontiguousarray(r, np.float32), h, w, float(scale))


def scenes():
    return [make_scene(c) for c in CASES]


def divide(boxes, scale):
    """boxes / im_scale as lib/fast_rcnn/test.py:57 does it: an fp32 division (a mutant of tests/test_lines_scenes.py replaces this)"""
    return boxes / np.float32(scale)


def prefix_dets(scene):
    """the connector NMS's input: rows [x1, y1, x2, y2, score] of the score > 0.7 prefix, boxes / scale in fp32"""
    s = scene.rois[:, 0]
    m = int(np.count_nonzero(s > np.float32(P.Cfg.TEXT_PROPOSALS_MIN_SCORE)))
    return np.hstack([divide(scene.rois[:m, 1:5], scene.scale), s[:m, None]]).astype(np.float32)


def oracle_keep(scene):
    d = prefix_dets(scene)
    return P.nms(d, P.Cfg.TEXT_PROPOSALS_NMS_THRESH) if d.shape[0] else []


def sole_suppressor_depths(dets, keep, thresh, col_scale=1.0):
    """dets: rows [x1, y1, x2, y2, score] in descending score order, keep: the oracle's greedy NMS of them. For every dropped row that exactly
    ONE kept row before it overlaps above the threshold (the oracle's fp32 IoU): that kept row's position among the kept rows of its own 16-px
    column -- how deep into a column's kept list a column NMS has to look to drop it. -> sorted list"""
    d = np.asarray(dets, np.float32)
    keep = np.asarray(keep, np.int64)
    area = (d[:, 2] - d[:, 0] + 1) * (d[:, 3] - d[:, 1] + 1)
    col = (d[:, 0] * np.float32(col_scale) + np.float32(0.5)).astype(np.int64) >> 4
    depth = {int(k): int(np.count_nonzero(col[keep[:i]] == col[k])) for i, k in enumerate(keep)}
    out = []
    for r in np.setdiff1d(np.arange(d.shape[0]), keep):
        k = keep[keep < r]
        w = np.maximum(np.float32(0), np.minimum(d[r, 2], d[k, 2]) - np.maximum(d[r, 0], d[k, 0]) + 1)
        h = np.maximum(np.float32(0), np.minimum(d[r, 3], d[k, 3]) - np.maximum(d[r, 1], d[k, 1]) + 1)
        over = k[w * h / (area[r] + area[k] - w * h) > np.float32(thresh)]
        if over.size == 1:
            out.append(depth[int(over[0])])
    return sorted(out)


def deep_heads(hf=20, wf=4, kept=150, dups=50, seed=16):
    """network heads for ONE image of hf x wf cells whose column 0 decodes to `kept` boxes of 8 px stepping 2 px (IoU 7 / 11 < 0.7: all
    survive, strictly descending scores) and `dups` lower-scored boxes of 7.5 px on top of the LAST `dups` of them (IoU 0.94 with that one,
    at most 0.67 with its neighbours), assigned to the column's hf x 10 anchors in shuffled order; the other columns decode below min_size.
    -> cls_prob (1, hf, wf, 20), bbox_pred (1, hf, wf, 40), im_info (3,): the proposal layer's inputs"""
    assert kept + dups == hf * 10 and 2 * kept + 8 < 16 * hf
    anc = P.anchors().astype(np.float64)
    cls = np.zeros((1, hf, wf, 10, 2), np.float32)
    box = np.zeros((1, hf, wf, 10, 4), np.float32)
    t = np.arange(kept - dups, kept)
    y1 = np.concatenate([2.0 * np.arange(kept), 2.0 * t])
    ph = np.concatenate([np.full(kept, 8.0), np.full(dups, 7.5)])
    score = np.concatenate([np.linspace(0.99, 0.6, kept), np.linspace(0.5, 0.3, dups)])
    for j, cell in enumerate(np.random.default_rng(seed).permutation(hf * 10)):
        y, a = divmod(int(cell), 10)
        h = anc[a, 3] - anc[a, 1] + 1.0
        box[0, y, 0, a] = [0.0, (y1[j] + ph[j] / 2.0 - (16 * y + anc[a, 1] + 0.5 * h)) / h, 0.0, np.log(ph[j] / h)]
        cls[0, y, 0, a] = [1.0 - score[j], score[j]]
    box[0, :, 1:, :, 3] = np.log(2.0 / (anc[:, 3] - anc[:, 1] + 1.0))
    cls[0, :, 1:] = [0.9, 0.1]
    return cls.reshape(1, hf, wf, 20), box.reshape(1, hf, wf, 40), np.array([16.0 * hf, 16.0 * wf, 1.0], np.float32)


def oracle_lines(scene, mode):
    """TextDetector.detect of the oracle on the scene, fed as test_ctpn + the demo feed it: boxes / scale, scores, the network size"""
    return P.text_detect(divide(scene.rois[:, 1:5], scene.scale), scene.rois[:, 0], (scene.h, scene.w), mode)
