"""Small generated proposal sets for the tests of the detection tail's run-time parameters (tests/test_tail_params.py on the host connector,
tests/test_gpu_tail_params.py on the device), in the style of tests/lines_scenes.py and built from its helpers: 192 x 320 images (a 12 x 20
feature map), at most 300 rois each, laid out so that boxes straddle every EDITED threshold of CONFIGS below, not only the defaults:

  band 0  two lines 80 px apart (columns 0-6 and 11-19): one line under MAX_HORIZONTAL_GAP 90, two under 50
  band 1  one line with every third column missing (32 px steps): it falls apart under MAX_HORIZONTAL_GAP 20
  band 2  a line of scores 0.81 .. 0.88 (kept under LINE_MIN_SCORE 0.8 only), a 3-column and a 4-column line (48 and 64 px wide: both go
          under a minimum width of 64)
  band 3  3 columns of 34-px boxes (width / height 1.4: gone under MIN_RATIO 1.5), then a line whose columns carry a second box at IoU
          0.25 .. 0.37 with the first (suppressed under TEXT_PROPOSALS_NMS_THRESH 0.2, kept under 0.4)
  band 4  a line with one column slid to 0.6 vertical overlap and one shrunk to 0.6 of the height (linked under MIN_V_OVERLAPS /
          MIN_SIZE_SIM 0.5 only), and a stretch of scores 0.55 .. 0.69 in its middle (proposals under TEXT_PROPOSALS_MIN_SCORE 0.5 only)
plus lines_scenes' own jitter, forks and near-threshold wobble. tests/test_tail_params.py asserts, on the oracle alone, that every
configuration changes the line set of every scene in both modes."""
import contextlib

import numpy as np

import lines_scenes as S
from oracle import postproc as P

H, W = 192, 320
SEEDS = (1, 2, 3, 4, 5)

# TextLineCfg attribute -> value; "MIN_LINE_WIDTH" stands for TEXT_PROPOSALS_WIDTH * MIN_NUM_PROPOSALS (the reference only uses the product)
CONFIGS = {
    "min_score_0.5": {"TEXT_PROPOSALS_MIN_SCORE": 0.5},
    "nms_0.4": {"TEXT_PROPOSALS_NMS_THRESH": 0.4},
    "gap_20": {"MAX_HORIZONTAL_GAP": 20},
    "gap_90": {"MAX_HORIZONTAL_GAP": 90},
    "v_overlaps_0.5": {"MIN_V_OVERLAPS": 0.5},
    "size_sim_0.5": {"MIN_SIZE_SIM": 0.5},
    "ratio_1.5": {"MIN_RATIO": 1.5},
    "line_score_0.8": {"LINE_MIN_SCORE": 0.8},
    "width_64": {"MIN_LINE_WIDTH": 64},
    "all": {"TEXT_PROPOSALS_MIN_SCORE": 0.5, "TEXT_PROPOSALS_NMS_THRESH": 0.4, "MAX_HORIZONTAL_GAP": 90, "MIN_V_OVERLAPS": 0.5,
            "MIN_SIZE_SIM": 0.5, "MIN_RATIO": 1.5, "LINE_MIN_SCORE": 0.8, "MIN_LINE_WIDTH": 64},
}
# ctpn_connector_constants' order
CFG8_NAMES = ("MIN_LINE_WIDTH", "MIN_RATIO", "LINE_MIN_SCORE", "MAX_HORIZONTAL_GAP", "TEXT_PROPOSALS_MIN_SCORE", "TEXT_PROPOSALS_NMS_THRESH",
              "MIN_V_OVERLAPS", "MIN_SIZE_SIM")
DEFAULTS = {"MIN_LINE_WIDTH": 32, "MIN_RATIO": 0.5, "LINE_MIN_SCORE": 0.9, "MAX_HORIZONTAL_GAP": 50, "TEXT_PROPOSALS_MIN_SCORE": 0.7,
            "TEXT_PROPOSALS_NMS_THRESH": 0.2, "MIN_V_OVERLAPS": 0.7, "MIN_SIZE_SIM": 0.7}


def cfg8(config):
    return np.array([float(dict(DEFAULTS, **config)[n]) for n in CFG8_NAMES], np.float64)


def as_text_line_cfg(config):
    """the configuration as TextLineCfg attributes (the width as TEXT_PROPOSALS_WIDTH with MIN_NUM_PROPOSALS 2)"""
    out = {k: v for k, v in config.items() if k != "MIN_LINE_WIDTH"}
    if "MIN_LINE_WIDTH" in config:
        out["TEXT_PROPOSALS_WIDTH"] = config["MIN_LINE_WIDTH"] // 2
        out["MIN_NUM_PROPOSALS"] = 2
    return out


@contextlib.contextmanager
def patched(cfg_class, config):
    """cfg_class (oracle.postproc.Cfg, or the reference's TextLineCfg) with `config` applied, restored afterwards"""
    edits = as_text_line_cfg(config)
    saved = {k: getattr(cfg_class, k) for k in edits}
    try:
        for k, v in edits.items():
            setattr(cfg_class, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(cfg_class, k, v)


def _box(rows, score, c, yc, h):
    rows.append([score, 16.0 * c, yc - h / 2.0, 16.0 * c + 15.0, yc - h / 2.0 + h - 1.0])


def make_scene(seed):
    rng = np.random.default_rng(1000 + seed)
    top, dim = S.LEVELS[-5:], S.LEVELS[4:9]
    rows = []
    cy = [20.0, 56.0, 92.0, 128.0, 164.0]
    # band 0: two lines 80 px apart
    S._line(rng, rows, 0, 6, cy[0], 16.0, 0.1, top, missing=0.0)
    S._line(rng, rows, 11, 19, cy[0] + 0.6, 16.0, -0.1, top, missing=0.0)
    # band 1: every third column missing
    for c in range(20):
        if c % 3 != 2:
            _box(rows, rng.choice(top), c, cy[1] + rng.integers(-2, 3) * 0.25, 18.0)
    # band 2: a dim line, a 3-column and a 4-column line
    S._line(rng, rows, 0, 6, cy[2], 14.0, 0.0, dim, second=0.0, missing=0.0, wobble=False)
    S._line(rng, rows, 10, 12, cy[2], 14.0, 0.0, top, second=0.0, missing=0.0, wobble=False)
    S._line(rng, rows, 16, 19, cy[2], 14.0, 0.0, top, second=0.0, missing=0.0, wobble=False)
    # band 3: a squat line, then second boxes between IoU 0.2 and 0.4
    for c in range(3):
        _box(rows, rng.choice(top), c, cy[3], 34.0)
    for c in range(8, 20):
        h = 18.0
        _box(rows, rng.choice(top), c, cy[3] + rng.integers(-1, 2) * 0.25, h)
        if c % 2 == 0:
            dy = float(rng.choice([8.5, 9.0, 10.0, 10.5]))          # IoU (h - dy) / (h + dy) = 0.36 .. 0.26
            _box(rows, rng.choice(top[:2]), c, cy[3] + dy, h)
    # band 4: one column slid, one shrunk, a stretch of low scores
    h = 20.0
    for c in range(20):
        sc = rng.choice(top)
        if c == 4:
            _box(rows, sc, c, cy[4] + 0.4 * h, h)                   # overlap 0.6 h
        elif c == 9:
            _box(rows, sc, c, cy[4], 0.6 * h)                       # size similarity 0.6
        elif 13 <= c <= 15:
            _box(rows, np.float32(rng.choice([0.55, 0.62, 0.69])), c, cy[4], h)
        else:
            _box(rows, sc, c, cy[4] + rng.integers(-1, 2) * 0.25, h)
    r = np.array(rows, np.float32).reshape(-1, 5)
    n = r.shape[0]
    r[:, 2] = np.maximum(r[:, 2], 0)
    r[:, 4] = np.minimum(r[:, 4], H - 1)
    r = r[rng.permutation(n)]
    r = r[np.argsort(-r[:, 0], kind="stable")]
    assert n <= 300
    return S.Scene("t%d" % seed, np.ascontiguousarray(r, np.float32), H, W, 1.0)


def scenes():
    return [make_scene(s) for s in SEEDS]


def oracle_lines(scene, mode, config=None):
    with patched(P.Cfg, config or {}):
        return S.oracle_lines(scene, mode)
