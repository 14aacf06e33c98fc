"""The proposal layer's kernels one at a time: the cells of its launch decisions, the data recipes, the numpy restatement of every stage, the
checks and the numpy models (with one defect each) that tests/test_proposal_cells.py (CPU) and tests/test_gpu_proposal_kernels.py (device) share.
No device needed.

The stage is decode_kernel -> radix_sort_kernel<false | true> + merge_rank_kernel -> gather_kernel -> nms_kernel / nms_columns_kernel<16, 12288, 128> /
nms_column_groups_kernel (csrc/decode.hip, sort_keys.hip, nms.hip). A CELL is everything that changes what a workgroup of it does, as one string

    sort / tail / nms / prefix / kept / batch / valid        e.g. "seg/odd/groups/falls/k256/n2-4/some"

  sort   one | seg     one workgroup per image, or eight segments + merge_rank_kernel
  tail   one: idle (per_img <= 960: some of the 16 waves have no keys) | full;  seg: eq (the last segment is as long as the others) | short (shorter, a
         multiple of MG_SP = 4) | odd (not a multiple of 4: a partial splitter group)
  nms    generic | one_wg | groups
  prefix p0 (no prefix pass planned) | none (planned, the image has no more valid candidates than the prefix looks at) | answers | falls (back to a
         full pass); of the image of the batch that goes furthest: falls > answers > none
  kept   the longest kept list of one column in the pass that answers, against the kernels' LDS capacities (128 one_wg, 256 groups):
         k128 (<= 128) | k256 (129 .. 256) | kbig (> 256);  "-" for the generic kernel
  batch  n1 | n2-4 (im_info in decode_kernel's arguments) | n5+ (the device copy)
  valid  all (every key of every image valid) | some | zero1 (an image without one valid key beside others) | none

sort, tail, nms, batch and whether a prefix pass is planned come from the library's plan (ctpn_debug_proposal_plan: the function enqueue_proposals
follows), the prefix outcome, kept and valid from model() below on the case's data. census() is the set of plan halves the grid reaches and REQUIRED_DATA the data classes every NMS form must meet;
proposal_cell_cases.CASES is the committed table (regenerate from the repository root: PYTHONPATH=. python tests/proposal_cells.py >
tests/proposal_cell_cases.py)."""
import collections
import functools

import numpy as np

from ctpn_amd import _binding as B
from oracle import cnms

KEY_INVALID = np.uint64(B.KEY_INVALID)
PREFIX_RANKS = 4096
KCAP = {"one_wg": 128, "groups": 256}
A_Y1 = np.array([2, 0, -4, -9, -16, -26, -41, -62, -91, -134], np.int64)
A_Y2 = np.array([13, 15, 19, 24, 31, 41, 56, 77, 106, 149], np.int64)
f32 = np.float32

# name, batch, map, top-N, threshold, min_size, options, recipes of the scores, of (dy, dh) and of im_info
Case = collections.namedtuple("Case", "name n hf wf pre post thresh min_size cols prefix scores deltas info")

GRID_N = (1, 2, 4, 5, 8, 32)
GRID_HF, GRID_WF = 110, 260
GRID_PRE = (300, 4096, 4097, 7000, 12000)
MUTANTS = ("merge_ties_strict", "splitter_group_dropped", "valid_counts_full_topn", "key_index_in_batch", "order_bits_negative", "min_size_no_scale",
           "im_info_second_for_third", "column_of_clipped_box", "prefix_never_falls_back", "kept_beyond_cap_ignored", "mask_not_cleared_after_again")


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def case_plan(c):
    info = case_inputs(c)[2]
    return B.proposal_plan(c.n, c.hf, c.wf, pre=c.pre, post=c.post, thresh=c.thresh, nms_columns=c.cols, nms_prefix=c.prefix, im_widths=info[:, 1])


# ---------------------------------------------------------------------------------------------------------------
# the plan half of a cell, and the census of it
# ---------------------------------------------------------------------------------------------------------------
def tail_class(sort_seg, per_img, seg_len, last_seg):
    if not sort_seg:
        seg = ((per_img + 15) // 16 + 63) & ~63            # radix_sort_kernel: a wave's share of the keys
        return "idle" if 15 * seg >= per_img else "full"
    return "eq" if last_seg == seg_len else ("short" if last_seg % 4 == 0 else "odd")


def batch_class(n):
    return "n1" if n == 1 else ("n2-4" if n <= 4 else "n5+")


def plan_half(n, per_img, raw):
    """raw: the nine ints of ctpn_debug_proposal_plan -> (sort, tail, nms, planned prefix launches, batch)"""
    seg = int(raw[2]) == 1
    return ("seg" if seg else "one", tail_class(seg, per_img, int(raw[3]), int(raw[4])), B.PROPOSAL_NMS_FORMS[int(raw[6])], int(raw[8]), batch_class(n))


@functools.lru_cache(maxsize=None)
def census():
    """{plan half: smallest (n * per_img, n, hf, wf, pre, nms_columns, nms_prefix)} over the grid"""
    found = {}
    hf = np.arange(1, GRID_HF + 1)[:, None]
    wf = np.arange(1, GRID_WF + 1)[None, :]
    per = hf * wf * 10
    for n in GRID_N:
        for cols in (0, 1, 2, 3):
            for prefix in (0, 1):
                for pre in GRID_PRE:
                    raw = B.proposal_plan_sweep(n, 1, GRID_HF, 1, GRID_WF, pre=pre, post=1000, thresh=0.7, nms_columns=cols, nms_prefix=prefix)
                    seg = raw[..., 2] == 1
                    sh = ((per + 15) // 16 + 63) & ~63
                    tail = np.where(seg, np.where(raw[..., 4] == raw[..., 3], 2, np.where(raw[..., 4] % 4 == 0, 3, 4)), np.where(15 * sh >= per, 0, 1))
                    code = tail * 100 + raw[..., 6] * 10 + raw[..., 8]
                    for cd in np.unique(code):
                        m = code == cd
                        k = np.argmin(np.where(m, per, 1 << 40))
                        a, b = divmod(int(k), GRID_WF)
                        key = plan_half(n, int(per[a, b]), raw[a, b])
                        # the smallest map; among equals the default options, more than one column and more than one row
                        cand = (n * int(per[a, b]), cols != 1, prefix != 1, n, a + 1, b + 1, pre)
                        if key not in found or cand < found[key][0]:
                            found[key] = (cand, (n, a + 1, b + 1, pre, cols, prefix))
    return {k: v[1] for k, v in found.items()}


# every NMS form that has the notion meets these classes of the data (cell words `prefix`, `kept`), and the layer these of `valid`
REQUIRED_DATA = [("one_wg", "prefix", w) for w in ("none", "answers", "falls")] + [("groups", "prefix", w) for w in ("none", "answers", "falls")] + \
                [(f, "kept", w) for f in ("one_wg", "groups") for w in ("k128", "k256", "kbig")] + [(None, "valid", w) for w in ("all", "some", "zero1", "none")]


# ---------------------------------------------------------------------------------------------------------------
# data recipes (seeded; nothing is read from outside the repository)
# ---------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    """(cls_prob (n, hf, wf, 20), bbox_pred (n, hf, wf, 40), im_info (n, 3)) of a case, float32"""
    rng = np.random.default_rng((c.n * 1000003 + c.hf * 1009 + c.wf) * 64 + len(c.scores + c.deltas + c.info))
    shape = (c.n, c.hf, c.wf, 10)
    if c.scores == "uniform":
        s = rng.random(shape, np.float32)
    elif c.scores == "saturated":                      # 60 % exactly 1.0: long runs of one score byte pattern, ties broken by the index alone
        s = np.where(rng.random(shape) < 0.6, f32(1.0), rng.random(shape, np.float32)).astype(np.float32)
    elif c.scores == "equal":
        s = np.full(shape, 0.5, np.float32)
    elif c.scores == "tiny":                           # 1e-13 .. 1.0: every exponent byte of the key's high word
        s = (10.0 ** rng.uniform(-13, 0, shape)).astype(np.float32)
    elif c.scores == "edge":                           # what only the host-heads seam can hand in (-0.0 apart: the key-order test pins it)
        s = rng.random(shape, np.float32)
        r = rng.random(shape)
        s = np.where(r < 0.1, f32(0.0), np.where(r < 0.3, -s, np.where(r < 0.4, f32(np.nan), np.where(r < 0.45, f32(np.inf), s)))).astype(np.float32)
    elif c.scores == "nan":
        s = np.full(shape, np.nan, np.float32)
    else:
        raise ValueError(c.scores)
    cls = np.zeros(shape + (2,), np.float32)
    cls[..., 1] = s
    cls[..., 0] = rng.random(shape, np.float32)
    d = (rng.standard_normal(shape + (4,)) * 0.3).astype(np.float32)
    if c.deltas == "normal":
        d[..., 3] = (rng.standard_normal(shape) * 0.5).astype(np.float32)
    elif c.deltas == "wide":                           # sigma(dh) 0.4 .. 0.6 by column and dy over a few anchors' heights: long kept lists at threshold 0.9
        d[..., 3] = (rng.standard_normal(shape) * np.linspace(0.4, 0.6, c.wf)[None, None, :, None]).astype(np.float32)
        d[..., 1] = (rng.standard_normal(shape) * 0.6).astype(np.float32)
    elif c.deltas == "tall":                           # dh = 3: every box is the image's height after the clip, one survivor per column
        d[..., 3] = 3.0
    else:
        raise ValueError(c.deltas)
    info = np.tile(np.array([c.hf * 16, c.wf * 16, 1.0], np.float32), (c.n, 1))
    if c.info in ("differ", "narrow", "zero"):         # different per image in h, w and scale
        for i in range(c.n):
            info[i] = [c.hf * 16 + (0, 9, -5, 4)[i % 4], c.wf * 16 + 7 * (i % 3), (1.0, 1.5, 0.75, 2.0)[i % 4]]
    if c.info == "narrow":                             # one image narrower than the map: its last columns' boxes are clipped onto one pixel column
        info[c.n - 1, 1] = max(c.wf * 16 - 40, 10)
    if c.info == "zero":                               # min_size x scale above every box
        info[c.n // 2, 2] = 1000.0
    return _frozen(cls.reshape(c.n, c.hf, c.wf, 20), d.reshape(c.n, c.hf, c.wf, 40), info)


# ---------------------------------------------------------------------------------------------------------------
# the stages restated
# ---------------------------------------------------------------------------------------------------------------
def order_bits(s):
    u = np.ascontiguousarray(s, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def score_from_order_bits(o):
    o = np.asarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7fffffff), ~o).astype(np.uint32).view(np.float32)


EXP_ULPS = 1            # |expf(dh) - float32(exp(float64(dh)))| of decode_kernel in ulps, the most measured (profiles/proposal_kernel_cells.txt)
EXP_ULPS_SEEN = 4       # ... and how far the measurement looks


def decode_ref(bbox, info_row, hf, wf):
    """One image: boxes (per_img, 4) float32 with exp taken in float64 and rounded once; the bound on y1 / y2 (float64, per anchor); and ys
    (2 EXP_ULPS_SEEN + 1, per_img, 2): y1 / y2 with exp k = -EXP_ULPS_SEEN .. EXP_ULPS_SEEN floats away from that rounding.
    decode.hip claims "the last ulp of exp()". E = exp(dh) off by EXP_ULPS ulps moves E x height by EXP_ULPS ulp(E) x height -- up to two ulps of
    pred_h, not one: the product's mantissa may be just above 1 where E's is just below 2 -- and pred_h's two roundings (the device's, the
    reference's) by ulp(pred_h) more; half of that reaches y = ctr -+ pred_h / 2, whose two roundings add ulp(y):
        0.5 (EXP_ULPS ulp(E) height + ulp(pred_h)) + ulp(y), y before the clip (the clip moves nothing apart)."""
    d = np.asarray(bbox, np.float32).reshape(hf, wf, 10, 4)
    y, x = np.meshgrid(np.arange(hf), np.arange(wf), indexing="ij")
    ax1 = (x * 16).astype(np.float32)[..., None] + np.zeros(10, np.float32)
    ax2 = (x * 16 + 15).astype(np.float32)[..., None] + np.zeros(10, np.float32)
    ay1 = (y[..., None] * 16 + A_Y1).astype(np.float32)
    ay2 = (y[..., None] * 16 + A_Y2).astype(np.float32)
    widths = ax2 - ax1 + f32(1.0)
    heights = ay2 - ay1 + f32(1.0)
    ctr_x = ax1 + f32(0.5) * widths
    ctr_y = ay1 + f32(0.5) * heights
    pcy = d[..., 1] * heights + ctr_y
    e0 = np.exp(d[..., 3].astype(np.float64)).astype(np.float32)
    imh, imw = f32(info_row[0]), f32(info_row[1])
    wl, hl = imw - f32(1.0), imh - f32(1.0)
    clip = lambda v, l: np.maximum(np.minimum(v, l), f32(0.0))
    ys = []
    for k in range(-EXP_ULPS_SEEN, EXP_ULPS_SEEN + 1):
        e = e0
        for _ in range(abs(k)):
            e = np.nextafter(e, f32(np.inf if k > 0 else 0.0))
        ph = e * heights
        ys.append(np.stack([clip(pcy - f32(0.5) * ph, hl), clip(pcy + f32(0.5) * ph, hl)], axis=-1).reshape(-1, 2))
        if k == 0:
            raw = [ctr_x - f32(0.5) * widths, pcy - f32(0.5) * ph, ctr_x + f32(0.5) * widths, pcy + f32(0.5) * ph]
            tol = 0.5 * (EXP_ULPS * np.spacing(e).astype(np.float64) * heights + np.spacing(ph)) + \
                np.maximum(np.spacing(np.abs(raw[1])), np.spacing(np.abs(raw[3]))).astype(np.float64)
    boxes = np.stack([clip(v, l) for v, l in zip(raw, [wl, hl] * 2)], axis=-1).astype(np.float32)
    return boxes.reshape(-1, 4), tol.reshape(-1), np.stack(ys).astype(np.float32)


def exp_ulps_of(b4, ys):
    """per anchor, the fewest floats exp must be away from its correct rounding for the restatement to give the device's y1 / y2 bit for bit
    (EXP_ULPS_SEEN + 1: none of those looked at does)"""
    hit = np.all(ys.view(np.uint32) == np.asarray(b4, np.float32)[None, :, 1::2].view(np.uint32), axis=2)
    dist = np.abs(np.arange(-EXP_ULPS_SEEN, EXP_ULPS_SEEN + 1))[:, None]
    return np.where(hit, dist, EXP_ULPS_SEEN + 1).min(axis=0)


def keys_ref(boxes4, scores, info_row, min_size, mutant=None, img=0):
    """decode_kernel's keep flag and key of one image from ITS boxes (per_img, 4) and the input scores"""
    b = np.asarray(boxes4, np.float32)
    s = np.asarray(scores, np.float32).reshape(-1)
    ms = f32(min_size) * (f32(1.0) if mutant == "min_size_no_scale" else f32(info_row[2]))
    keep = (b[:, 2] - b[:, 0] + f32(1.0) >= ms) & (b[:, 3] - b[:, 1] + f32(1.0) >= ms) & (s == s)
    ob = order_bits(s)
    if mutant == "order_bits_negative":
        ob = s.view(np.uint32) | np.uint32(0x80000000)
    idx = np.arange(s.size, dtype=np.uint64) + np.uint64(img * s.size if mutant == "key_index_in_batch" else 0)
    return np.where(keep, ((~ob).astype(np.uint64) << np.uint64(32)) | idx, KEY_INVALID)


def sort_ref(keys, npad):
    out = np.full(npad, KEY_INVALID, np.uint64)
    out[: keys.size] = np.sort(keys)
    return out


def merge_model(keys, npad, seg_len, mutant):
    """merge_rank_kernel with one defect, on the sorted segments of one image: rank = place in the own segment + keys before it in every other one"""
    n = keys.size
    out = np.zeros(npad, np.uint64)                  # a slot nobody writes keeps what it held: here a key that reads as valid
    out[n:] = KEY_INVALID
    segs = [np.sort(keys[a: a + seg_len]) for a in range(0, n, seg_len)]
    for s, ks in enumerate(segs):
        rank = np.arange(ks.size)
        for g, kg in enumerate(segs):
            if g == s:
                continue
            if mutant == "splitter_group_dropped":
                kg = kg[: kg.size // 4 * 4]
            side = "left" if (mutant == "merge_ties_strict" or g > s) else "right"
            rank = rank + np.searchsorted(kg, ks, side=side)
        out[rank] = ks
    return out


def nms_col_of(x1, ncols):
    return np.clip((np.asarray(x1, np.float32) + f32(0.5)).astype(np.int32) >> 4, 0, ncols - 1)


def gather_ref(skeys, boxes4, pre, wf):
    """One image: (sorted_boxes, sorted_scores as uint32 bits, sorted_anchor, colid) of the valid prefix of the first `pre` keys, and its length"""
    k = skeys[:pre]
    inv = np.nonzero(k == KEY_INVALID)[0]
    v = int(inv[0]) if inv.size else k.size
    idx = (k[:v] & np.uint64(0xffffffff)).astype(np.int64)
    sb = np.asarray(boxes4, np.float32)[np.minimum(idx, len(boxes4) - 1)]      # (an index beyond the image is a defect the key check names first)
    sc = score_from_order_bits((~(k[:v] >> np.uint64(32))).astype(np.uint32))
    return sb, sc.view(np.uint32), idx.astype(np.int32), nms_col_of(sb[:, 0], wf).astype(np.uint8), v


def nms_ref(sorted_boxes, thresh, limit=None):
    """oracle.postproc.nms's predicate (its C restatement) on boxes already in score order: kept ranks, ascending"""
    b = np.asarray(sorted_boxes, np.float32)
    if b.shape[0] == 0:
        return np.zeros(0, np.int32)
    dets = np.hstack([b, -np.arange(b.shape[0], dtype=np.float32)[:, None]])       # 12000 ranks are exact in float32
    k = np.asarray(cnms.nms(dets, thresh), np.int32)
    return k if limit is None else k[:limit]


def column_nms_model(boxes, cols, thresh, kcap):
    """greedy NMS per column whose candidates see the first kcap kept boxes of their column only (kcap None: all): kept ranks, ascending"""
    b = np.asarray(boxes, np.float32)
    area = (b[:, 2] - b[:, 0] + f32(1.0)) * (b[:, 3] - b[:, 1] + f32(1.0))
    thr = f32(thresh)
    keep = []
    for c in np.unique(cols):
        ranks = np.nonzero(cols == c)[0]
        if kcap is None:
            keep.extend(ranks[nms_ref(b[ranks], thresh)].tolist())
            continue
        kept = []
        for r in ranks:
            ks = np.array(kept[:kcap], np.int64)
            if ks.size:
                w = np.maximum(np.minimum(b[r, 2], b[ks, 2]) - np.maximum(b[r, 0], b[ks, 0]) + f32(1.0), f32(0.0))
                h = np.maximum(np.minimum(b[r, 3], b[ks, 3]) - np.maximum(b[r, 1], b[ks, 1]) + f32(1.0), f32(0.0))
                inter = w * h
                if np.any(inter / (area[ks] + area[r] - inter) > thr):
                    continue
            kept.append(int(r))
        keep.extend(kept)
    return np.sort(np.array(keep, np.int32))


# ---------------------------------------------------------------------------------------------------------------
# the whole stage as a model (mutant None: what the device must return), and its data classes
# ---------------------------------------------------------------------------------------------------------------
def model(c, mutant=None):
    """Every intermediate of ctpn_debug_proposal_fetch, the rois and anchors of one call, keyed as the fetch names them, + "stats" per image."""
    cls, bbox, info = case_inputs(c)
    plan = case_plan(c)
    per_img, npad = c.hf * c.wf * 10, next_pow2(c.hf * c.wf * 10)
    out = {k: [] for k in ("boxes4", "sorted_keys", "sorted_boxes", "sorted_scores", "sorted_anchor", "valid_counts", "colid", "keep", "rois", "anchors")}
    stats = []
    scratch = np.zeros((c.n, 2048), np.uint8)
    for i in range(c.n):
        row = info[1 if (mutant == "im_info_second_for_third" and i == 2) else i]
        boxes4 = decode_ref(bbox[i], row, c.hf, c.wf)[0]
        scores = cls[i].reshape(-1, 2)[:, 1]
        keys = keys_ref(boxes4, scores, row, c.min_size, mutant, i)
        if plan.sort == "segmented" and mutant in ("merge_ties_strict", "splitter_group_dropped"):
            skeys = merge_model(keys, npad, plan.seg_len, mutant)
        else:
            skeys = sort_ref(keys, npad)
        sb, sc, sa, colid, v = gather_ref(skeys, boxes4, c.pre, c.wf)
        vc = v - 1 if (mutant == "valid_counts_full_topn" and v == c.pre) else v
        cols = nms_col_of(sb[:vc, 0], c.wf)
        # the pass that answers: the prefix's ranks where they hold `post` survivors, else all
        full = nms_ref(sb[:vc], c.thresh)
        outcome = "p0" if plan.prefix == "none" else "none"
        keep = full
        if plan.prefix != "none" and vc > PREFIX_RANKS:
            pk = full[full < PREFIX_RANKS]
            outcome = "answers" if pk.size >= c.post else "falls"
            if outcome == "answers" or mutant == "prefix_never_falls_back":
                keep = pk
            if outcome == "falls" and mutant == "mask_not_cleared_after_again" and plan.nms == "groups":
                np.bitwise_or.at(scratch[i], pk >> 3, (1 << (pk & 7)).astype(np.uint8))
        if plan.nms != "generic":
            if mutant == "column_of_clipped_box":
                keep = column_nms_model(sb[:vc], (sa[:vc] // 10) % c.wf, c.thresh, None)        # the anchor's column, not the clipped x1's
            kept_max = int(np.bincount(cols[keep], minlength=1).max()) if keep.size else 0
            kept = "k128" if kept_max <= 128 else ("k256" if kept_max <= 256 else "kbig")
            if mutant == "kept_beyond_cap_ignored" and kept_max > KCAP[plan.nms]:
                keep = column_nms_model(sb[:vc], cols, c.thresh, KCAP[plan.nms])
        else:
            kept_max, kept = 0, "-"
        keep = keep[: c.post]
        stats.append(dict(valid=int(np.count_nonzero(keys != KEY_INVALID)), outcome=outcome, kept=kept, kept_max=kept_max,
                          cand_max=int(np.bincount(cols, minlength=1).max()) if vc else 0))
        for k, val in (("boxes4", boxes4), ("sorted_keys", skeys), ("sorted_boxes", sb), ("sorted_scores", sc), ("sorted_anchor", sa), ("valid_counts", vc),
                       ("colid", colid), ("keep", keep.astype(np.int32)), ("rois", np.hstack([sc.view(np.float32)[keep][:, None], sb[keep]]).astype(np.float32)),
                       ("anchors", sa[keep])):
            out[k].append(val)
    out["mw_scratch"] = scratch
    out["stats"] = stats
    return out


def data_half(c, stats=None):
    """(prefix, kept, valid) words of a case's cell"""
    st = model(c)["stats"] if stats is None else stats
    per_img = c.hf * c.wf * 10
    order = ("p0", "none", "answers", "falls")
    prefix = max((s["outcome"] for s in st), key=order.index)
    kept = max((s["kept"] for s in st), key=("-", "k128", "k256", "kbig").index)
    v = [s["valid"] for s in st]
    valid = "all" if min(v) == per_img else ("none" if max(v) == 0 else ("zero1" if min(v) == 0 else "some"))
    return prefix, kept, valid


def case_cell(c):
    p = case_plan(c)
    raw = B.proposal_plan_sweep(c.n, c.hf, 1, c.wf, 1, pre=c.pre, post=c.post, thresh=c.thresh, nms_columns=c.cols, nms_prefix=c.prefix,
                                im_widths=case_inputs(c)[2][:, 1])[0, 0]
    sort, tail, nms, _, batch = plan_half(c.n, c.hf * c.wf * 10, raw)
    assert nms == p.nms
    prefix, kept, valid = data_half(c)
    return "/".join((sort, tail, nms, prefix, kept, batch, valid))


def cell_plan_half(cell, c):
    """the census key a committed (cell, case) stands for"""
    sort, tail, nms, prefix, _, batch, _ = cell.split("/")
    launches = 0 if prefix == "p0" else (2 if nms == "groups" else 1)
    return (sort, tail, nms, launches, batch)


# ---------------------------------------------------------------------------------------------------------------
# the checks: every stage against the oracle operation on the PREVIOUS tensor of `got` (the device's, or a mutant model's)
# ---------------------------------------------------------------------------------------------------------------
def check_stages(c, got, report=None):
    """got: model()'s keys, per image (arrays of the fetch's shapes are fine: rows behind the counts are ignored). Raises AssertionError.
    report (a list): gets (case, image, max |dy| / bound, the most floats exp is off, anchors where it is off at all) for the measured table."""
    cls, bbox, info = case_inputs(c)
    plan = case_plan(c)
    per_img, npad = c.hf * c.wf * 10, next_pow2(c.hf * c.wf * 10)
    for i in range(c.n):
        tag = "%s image %d: " % (c.name, i)
        # decode
        ref, tol, ys = decode_ref(bbox[i], info[i], c.hf, c.wf)
        b4 = np.asarray(got["boxes4"][i], np.float32)
        assert np.array_equal(b4[:, 0::2].view(np.uint32), ref[:, 0::2].view(np.uint32)), tag + "decode x1 / x2"
        dy = np.abs(b4[:, 1::2].astype(np.float64) - ref[:, 1::2].astype(np.float64)).max(axis=1)
        ulps = exp_ulps_of(b4, ys)
        if report is not None:
            report.append((c.name, i, float((dy / tol).max()), int(ulps.max()), int(np.count_nonzero(ulps))))
        # y1 / y2 are the float32 restatement's bits for an exp within EXP_ULPS floats of the correctly rounded one, and so inside the bound
        assert ulps.max() <= EXP_ULPS, tag + "decode y1 / y2 of %d anchors need exp %d floats off" % (np.count_nonzero(ulps > EXP_ULPS), ulps.max())
        assert np.all(dy <= tol), tag + "decode y off by %.3g x its bound" % (dy / tol).max()
        # keys and sort
        keys = keys_ref(b4, cls[i].reshape(-1, 2)[:, 1], info[i], c.min_size)
        skeys = np.asarray(got["sorted_keys"][i], np.uint64)
        assert skeys.shape == (npad,) and np.array_equal(skeys, sort_ref(keys, npad)), tag + "sorted keys"
        # gather
        sb, sc, sa, colid, v = gather_ref(skeys, b4, c.pre, c.wf)
        assert int(got["valid_counts"][i]) == v, tag + "valid_counts %d, not %d" % (int(got["valid_counts"][i]), v)
        gb = np.asarray(got["sorted_boxes"][i], np.float32)[:v]
        assert np.array_equal(gb.view(np.uint32), sb.view(np.uint32)), tag + "sorted_boxes"
        assert np.array_equal(np.asarray(got["sorted_scores"][i]).view(np.uint32)[:v], sc), tag + "sorted_scores"
        assert np.array_equal(np.asarray(got["sorted_anchor"][i])[:v], sa), tag + "sorted_anchor"
        if plan.nms == "groups":
            assert np.array_equal(np.asarray(got["colid"][i])[:v], colid), tag + "colid"
        # NMS, on the device's sorted boxes
        keep = nms_ref(gb, c.thresh, c.post)
        gk = np.asarray(got["keep"][i], np.int32)
        assert gk.size == keep.size and np.array_equal(gk, keep), tag + "keep list (%d kept, oracle %d)" % (gk.size, keep.size)
        rois = np.hstack([sc.view(np.float32)[keep][:, None], gb[keep]]).astype(np.float32)
        assert np.array_equal(np.asarray(got["rois"][i], np.float32).view(np.uint32), rois.view(np.uint32)), tag + "rois"
        assert np.array_equal(np.asarray(got["anchors"][i]), sa[keep]), tag + "anchors"
    assert not np.any(got["mw_scratch"]), c.name + ": the multi-workgroup NMS's scratch is not zero after the call"


def caught(c, mutant):
    """do the checks reject the model with this defect on this case?"""
    try:
        check_stages(c, model(c, mutant))
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------
# the table's source: the census's smallest cases on plain data + the cases that reach the data classes and the switch points
# ---------------------------------------------------------------------------------------------------------------
def _case(name, n, hf, wf, pre=12000, post=1000, thresh=0.7, min_size=8.0, cols=1, prefix=1, scores="uniform", deltas="normal", info="same"):
    return Case(name, n, hf, wf, pre, post, thresh, min_size, cols, prefix, scores, deltas, info)


def extra_cases():
    E = [
        # sort: the switch points of the segmented form, idle waves, equal segments
        _case("sort_1x1", 1, 1, 1), _case("sort_3x5_differ", 3, 3, 5, info="differ"), _case("sort_4080", 1, 102, 4, scores="saturated"),
        _case("sort_4100_edge", 2, 41, 10, scores="edge", info="differ"), _case("sort_4130_odd", 1, 59, 7, scores="tiny", min_size=14.0),
        _case("sort_4130_all_valid", 2, 59, 7, scores="tiny", deltas="tall"),
        _case("sort_2x256_eq", 1, 2, 256, scores="equal"), _case("sort_32760", 1, 52, 63, scores="saturated"), _case("sort_32770", 1, 29, 113),
        _case("sort_n4_seg", 4, 41, 10, info="differ"), _case("sort_n5_one", 5, 41, 10, info="differ"),
        # NMS: column counts, candidates per column, kept lists against the LDS capacities
        _case("nms_wf1", 2, 30, 1), _case("nms_wf3", 1, 20, 3), _case("nms_wf5", 1, 20, 5, cols=3), _case("nms_wf17", 1, 6, 17), _case("nms_wf256", 1, 1, 256),
        _case("nms_wf257_generic", 1, 1, 257), _case("nms_1020", 1, 102, 4), _case("nms_1030", 1, 103, 4),
        _case("kept_60x3_groups", 1, 60, 3, thresh=0.9, deltas="wide"), _case("kept_100x2_groups", 1, 100, 2, thresh=0.9, deltas="wide"),
        _case("kept_60x3_one_wg", 1, 60, 3, thresh=0.9, deltas="wide", cols=2), _case("kept_100x2_one_wg", 1, 100, 2, thresh=0.9, deltas="wide", cols=2),
        _case("kept_mid_groups", 1, 25, 3, thresh=0.9, deltas="wide"), _case("kept_mid_one_wg", 2, 25, 3, thresh=0.9, deltas="wide", cols=2),
        # prefix: answers / falls back / none in both column forms, pre on both sides of 4096, colid pitch 7008
        _case("tall_groups_12000", 1, 50, 12, deltas="tall"), _case("tall_one_wg_12000", 1, 50, 12, deltas="tall", cols=2),
        _case("tall_groups_4097", 1, 50, 12, pre=4097, deltas="tall"), _case("tall_groups_4096", 1, 50, 12, pre=4096, deltas="tall"),
        _case("pre_300", 2, 20, 8, pre=300, post=100), _case("pre_7000", 2, 72, 10, pre=7000, post=50), _case("pre_7000_one_wg", 2, 72, 10, pre=7000, post=50, cols=2),
        _case("post_below", 1, 20, 8, post=30), _case("post_above", 1, 20, 8, post=1000, cols=0),
        _case("anchor_37x56", 1, 37, 56, pre=12000),
        # scores and im_info
        _case("scores_edge_one", 1, 12, 9, scores="edge", cols=2), _case("scores_nan", 2, 5, 4, scores="nan"), _case("scores_equal_5", 5, 9, 5, scores="equal"),
        _case("info_narrow", 3, 20, 9, min_size=1.0, info="narrow"), _case("info_zero", 3, 41, 10, info="zero"), _case("info_zero_8", 8, 6, 5, info="zero"),
        _case("batch_8", 8, 7, 9, info="differ"), _case("batch_32", 32, 3, 5, info="differ"), _case("batch_32_groups", 32, 3, 5, cols=3, info="differ"),
    ]
    return E


def build_table():
    rows = []
    for key, (n, hf, wf, pre, cols, prefix) in sorted(census().items()):
        c = _case("census_%s_%s_%s_p%d_%s" % key, n, hf, wf, pre=pre, cols=cols, prefix=prefix, info="differ" if n > 1 else "same")
        rows.append((case_cell(c), c))
    for c in extra_cases():
        rows.append((case_cell(c), c))
    return rows


if __name__ == "__main__":
    print('"""The committed table of tests/proposal_cells.py: (cell, case) rows. Generated: PYTHONPATH=. python tests/proposal_cells.py > tests/proposal_cell_cases.py"""')
    print("from proposal_cells import Case")
    print()
    print("CASES = [")
    for cell, c in build_table():
        print("    (%r, %r)," % (cell, c))
    print("]")
