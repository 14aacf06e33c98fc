"""decode_kernel's PRODUCTION branch (csrc/decode.hip, heads != nullptr) on chosen heads: the cases, their seeded recipes, the expected values,
the checks and a numpy model of the branch (with one defect each) that tests/test_decode_heads_cells.py (CPU) and
tests/test_gpu_decode_heads.py (device, through ctpn_debug_proposals_from_heads) share. No device needed.

The branch reads the heads GEMM's fp32 rows of 64 floats -- a float4 of deltas at column 4 a, the (bg, fg) logit pair at 40 + 2 a, columns
60 .. 63 unused -- takes the pair softmax in the kernel (fmaxf, two expf, a sum, two divides), stores rpn_cls_prob_reshape and rpn_bbox_pred,
drops the cells below an image of a ragged batch (valid_rows) and, for up to four images, takes im_info from its arguments through selects
and publishes it to the device copy. proposal_cells.py starts behind all of that (ctpn_proposals_from_host).

CASES are the smallest shapes that reach each situation (test_decode_heads_cells.py asserts the seams):
  1,1,1   10 anchors: fewer than a wave          4,2,3   240 anchors: all four select arms in one 256-thread block
  5,2,3   the device copy of im_info, one block seam              3,5,7   1050 anchors: image seams in mid-block, five blocks
  3,6,4 with valid_rows (6, 3, 1): the ragged filter              2,6,4 with valid_rows (6, 6): the filter present but idle
  2,2,3 at min_size 0.5: the non-finite deltas whose key STAYS VALID (below)
Every image of a case has its own [h, w, scale] row: widths three pixels apart below the map's (the last column's x2 clips differently for every
image), heights and scales that differ; swapped_row_shows() asserts that any other image's row changes a box or a keep flag.

LOGITS of an anchor, by recipe (KINDS), and what the kernel's five operations give (mx = fmaxf(s0, s1); e = expf(s - mx); p = e / (e0 + e1)):
  normal   sigma 2                        p inside the interval of softmax_interval() -- an exponential at most EXP_ULPS floats off
  tie      s0 == s1                       e0 = e1 = 1: p = 0.5, 0.5 as bits; the sort's ascending-anchor rule decides among them
  d20      s1 = s0 +- 20                  the small exponential is a normal float
  d88      +- 88                          ... a subnormal (exp(-88) = 6.1e-39)
  d104     +- 104                         ... zero: exp(-104) = 6.8e-46 is below half the smallest subnormal. p = 1.0 and 0.0 as bits
  d200     +- 200                         ... zero. Without the max subtraction exp(200) = inf and p = NaN
  big      both +-1e30, one float apart   the difference is 7.6e22: p = 1.0 and 0.0 as bits. Only valid WITH the max subtraction
  neg_inf  -inf in one logit              e = expf(-inf) = 0: p = 1.0 and 0.0 as bits; the fg score 0.0 is a valid key
  pos_inf  +inf in one logit              mx = inf, inf - inf = NaN: p = NaN, NaN, and the key is KEY_INVALID. (The limit is 1 and 0; the float64
                                          pair softmax of oracle.network and numpy say NaN as well.)
  nan      NaN in one logit               fmaxf drops the NaN, expf(NaN) is NaN, the sum is NaN: p = NaN, NaN; KEY_INVALID, as decode.hip documents
Columns 60 .. 63 of every row hold NaN bit patterns; no output may depend on them.

DELTAS: proposal_cells' recipe (sigma 0.3; dh sigma 0.5), and a few anchors with one non-finite component. The kernel clips with
fmaxf(fminf(v, lim), 0), the reference with numpy's maximum(minimum(v, lim), 0); fminf / fmaxf return the OTHER operand for a NaN, numpy keeps it:
  dh +100   expf = inf: y1 = -inf, y2 = +inf -> 0 and h - 1. The whole height. numpy agrees. The key is valid.
  dh -100   expf = 3.8e-44 (or zero): y1 = y2 = the centre. numpy agrees. One pixel high: dropped at min_size 8, kept at 0.5.
  dy +inf   y1 = y2 = +inf -> h - 1, h - 1. numpy agrees. One pixel high.       dy -inf   -> 0, 0. numpy agrees.
  dh NaN    y1 = y2 = NaN -> fminf(NaN, h - 1) = h - 1, then fmaxf(h - 1, 0): the kernel stores y1 = y2 = h - 1, a one-pixel box on the image's
            last row. numpy stores NaN, and NaN >= min_size is false: the reference drops the box at ANY min_size.
FINDING (reported, not hidden): at min_size x scale <= 1 the kernel keeps a box of an anchor whose dh is NaN -- [x1, h - 1, x2, h - 1] with a valid
key -- where the reference drops it. The shipped min_size is 8, where both drop it (the box is one pixel high); case min_size_half pins the
kernel's behaviour. A NaN dy behaves the same way through pred_ctr_y; it is not in the table. nonfinite_expected() writes all of this down."""
import collections
import functools

import numpy as np

import proposal_cells as C

f32 = np.float32
KEY_INVALID = C.KEY_INVALID
PRE, POST, THRESH = 12000, 1000, 0.7
EXP_ULPS = 1            # |expf(s - mx) - float32(exp(float64(s - mx)))| of decode_kernel's softmax in floats, the most allowed (as for the height decode)
EXP_ULPS_SEEN = 4       # ... and how far the measurement looks

Case = collections.namedtuple("Case", "name n hf wf valid_rows min_size")
CASES = [
    Case("one_cell", 1, 1, 1, None, 8.0),
    Case("four_selects", 4, 2, 3, None, 8.0),
    Case("five_device_rows", 5, 2, 3, None, 8.0),
    Case("seams_3x5x7", 3, 5, 7, None, 8.0),
    Case("ragged_6_3_1", 3, 6, 4, (6, 3, 1), 8.0),
    Case("ragged_idle", 2, 6, 4, (6, 6), 8.0),
    Case("min_size_half", 2, 2, 3, None, 0.5),
]
BY_NAME = {c.name: c for c in CASES}

KINDS = ("normal", "tie", "d20+", "d20-", "d88+", "d88-", "d104+", "d104-", "d200+", "d200-", "big+", "big-", "pos_inf0", "pos_inf1", "neg_inf0",
         "neg_inf1", "nan0", "nan1")
DELTA_KINDS = ("finite", "dh+100", "dh-100", "dh_nan", "dy+inf", "dy-inf")
DEFECTS = ("select_image2_gets_row1", "select_image3_gets_row2", "head_ld_60", "pair_of_next_anchor", "fg_bg_swapped_in_store", "no_max_subtraction",
           "valid_rows_le", "valid_rows_of_previous_image", "dy_dh_from_x_z", "nan_score_kept")


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def info_rows(c):
    """a different [h, w, scale] per image; ragged cases: a height inside the image's last valid feature row"""
    info = np.zeros((c.n, 3), np.float32)
    for i in range(c.n):
        h = c.hf * 16 + (0, 9, -5, 4, -11)[i] if c.valid_rows is None else c.valid_rows[i] * 16 + (0, 9, 5)[i]
        info[i] = [h, c.wf * 16 - 3 * i, (1.0, 1.5, 0.75, 2.0, 1.25)[i]]
    return info


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    """(heads (n, hf, wf, 64) float32, im_info (n, 3), valid_rows int32 (n,) or None, kind (n, hf, wf, 10) index into KINDS, delta kind likewise)"""
    rng = np.random.default_rng(c.n * 1000003 + c.hf * 1009 + c.wf * 31 + len(c.name))
    shape = (c.n, c.hf, c.wf, 10)
    total = int(np.prod(shape))
    order = rng.permutation(total)
    kind = np.zeros(total, np.int64)
    n_special = total // 2
    kind[order[:n_special]] = 1 + np.arange(n_special) % (len(KINDS) - 1)
    dkind = np.zeros(total, np.int64)
    n_delta = 2 if total < 60 else max(5, total // 40)
    dkind[order[n_special: n_special + n_delta]] = 1 + np.arange(n_delta) % (len(DELTA_KINDS) - 1)
    s = (rng.standard_normal((total, 2)) * 2.0).astype(np.float32)
    for k, name in enumerate(KINDS):
        at = np.nonzero(kind == k)[0]
        if name == "tie":
            s[at, 1] = s[at, 0]
        elif name[0] == "d":
            s[at, 1] = s[at, 0] + f32(float(name[1:-1]) * (1 if name[-1] == "+" else -1))
        elif name.startswith("big"):
            s[at, 0] = f32(1e30 if name[-1] == "+" else -1e30)
            up = np.arange(at.size) % 2 == 0
            s[at, 1] = np.where(up, np.nextafter(s[at, 0], f32(np.inf)), np.nextafter(s[at, 0], f32(-np.inf)))
        elif name.startswith("pos_inf"):
            s[at, int(name[-1])] = np.inf
        elif name.startswith("neg_inf"):
            s[at, int(name[-1])] = -np.inf
        elif name.startswith("nan"):
            s[at, int(name[-1])] = np.nan
    d = (rng.standard_normal((total, 4)) * 0.3).astype(np.float32)
    d[:, 3] = (rng.standard_normal(total) * 0.5).astype(np.float32)
    for k, (col, v) in enumerate([(3, 100.0), (3, -100.0), (3, np.nan), (1, np.inf), (1, -np.inf)], 1):
        d[dkind == k, col] = v
    heads = np.zeros((c.n * c.hf * c.wf, 64), np.float32)
    heads[:, :40] = d.reshape(-1, 40)
    heads[:, 40:60] = s.reshape(-1, 20)
    heads[:, 60:].view(np.uint32)[:] = np.array([0x7fc00000, 0xffc00001, 0x7f800001, 0xffffffff], np.uint32)      # quiet and signalling NaN
    vr = None if c.valid_rows is None else np.array(c.valid_rows, np.int32)
    return _frozen(heads.reshape(c.n, c.hf, c.wf, 64), info_rows(c), vr, kind.reshape(shape), dkind.reshape(shape))


# ---------------------------------------------------------------------------------------------------------------
# the pair softmax: the float64 reference, the float32 restatement of the kernel's five operations, the interval
# ---------------------------------------------------------------------------------------------------------------
def softmax64(s):
    """the float64 pair softmax (oracle.network.pair_softmax's operations) of logits (..., 2)"""
    s = np.asarray(s, np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(s - s.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


def _moved(e, k):
    for _ in range(abs(k)):
        e = np.nextafter(e, f32(np.inf if k > 0 else 0.0))
    return e


def softmax_restated(s, k0=0, k1=0, max_subtraction=True):
    """decode_kernel's softmax in float32, each exponential k floats away from the correctly rounded one -> (..., 2) float32"""
    s = np.asarray(s, np.float32)
    with np.errstate(all="ignore"):
        mx = np.fmax(s[..., 0], s[..., 1]) if max_subtraction else f32(0.0)        # fmaxf: the other operand for a NaN
        e0 = _moved(np.exp((s[..., 0] - mx).astype(np.float64)).astype(np.float32), k0)
        e1 = _moved(np.exp((s[..., 1] - mx).astype(np.float64)).astype(np.float32), k1)
        total = e0 + e1
        return np.stack([e0 / total, e1 / total], axis=-1).astype(np.float32)


def softmax_expected(s):
    """per pair: `nan` (both NaN expected), `exact` (the bits are known) with the bits in `p`, the rest measured"""
    s = np.asarray(s, np.float32)
    p = softmax_restated(s)
    with np.errstate(all="ignore"):
        d = (s - np.fmax(s[..., 0], s[..., 1])[..., None]).astype(np.float64)
        e = np.exp(d).astype(np.float32)
    nan = np.isnan(p[..., 0])
    tie = s[..., 0] == s[..., 1]
    zero = ~nan & ((e[..., 0] == 0) | (e[..., 1] == 0))            # the other exponential is zero: 1.0 and 0.0
    return nan, (tie | zero) & ~nan, p


def softmax_interval(s):
    """(lo, hi) float64 (..., 2): the restatement with each exponential up to EXP_ULPS floats either way"""
    ps = np.stack([softmax_restated(s, a, b).astype(np.float64) for a in range(-EXP_ULPS, EXP_ULPS + 1) for b in range(-EXP_ULPS, EXP_ULPS + 1)])
    return ps.min(axis=0), ps.max(axis=0)


def softmax_exp_floats(s, got):
    """per pair, the fewest floats the two exponentials must be off for the restatement to give `got`'s bits (EXP_ULPS_SEEN + 1: not found)"""
    got = np.asarray(got, np.float32).view(np.uint32)
    best = np.full(got.shape[:-1], EXP_ULPS_SEEN + 1, np.int64)
    r = range(-EXP_ULPS_SEEN, EXP_ULPS_SEEN + 1)
    for a in r:
        for b in r:
            hit = np.all(softmax_restated(s, a, b).view(np.uint32) == got, axis=-1)
            best = np.where(hit, np.minimum(best, max(abs(a), abs(b))), best)
    return best


# ---------------------------------------------------------------------------------------------------------------
# the decode: proposal_cells' for the finite anchors, the kernel's operations written out for the others
# ---------------------------------------------------------------------------------------------------------------
def decode_restated(d4, info_row, hf, wf, numpy_clip=False):
    """decode_kernel's box arithmetic in float32 on deltas (hf * wf * 10, 4) -> boxes (per_img, 4); exp correctly rounded. numpy_clip: the
    reference's maximum(minimum()) instead of fmaxf(fminf())"""
    d = np.asarray(d4, np.float32).reshape(hf, wf, 10, 4)
    y, x = np.meshgrid(np.arange(hf), np.arange(wf), indexing="ij")
    zero = np.zeros(10, np.float32)
    ax1 = (x * 16).astype(np.float32)[..., None] + zero
    ax2 = (x * 16 + 15).astype(np.float32)[..., None] + zero
    ay1 = (y[..., None] * 16 + C.A_Y1).astype(np.float32)
    ay2 = (y[..., None] * 16 + C.A_Y2).astype(np.float32)
    widths = ax2 - ax1 + f32(1.0)
    heights = ay2 - ay1 + f32(1.0)
    ctr_x = ax1 + f32(0.5) * widths
    ctr_y = ay1 + f32(0.5) * heights
    with np.errstate(all="ignore"):
        pcy = d[..., 1] * heights + ctr_y
        ph = np.exp(d[..., 3].astype(np.float64)).astype(np.float32) * heights
        raw = [ctr_x - f32(0.5) * widths, pcy - f32(0.5) * ph, ctr_x + f32(0.5) * widths, pcy + f32(0.5) * ph]
        wl, hl = f32(info_row[1]) - f32(1.0), f32(info_row[0]) - f32(1.0)
        lo, hi = (np.minimum, np.maximum) if numpy_clip else (np.fmin, np.fmax)
        return np.stack([hi(lo(v, l), f32(0.0)) for v, l in zip(raw, [wl, hl] * 2)], axis=-1).astype(np.float32).reshape(-1, 4)


def keep_restated(boxes4, info_row, min_size):
    b = np.asarray(boxes4, np.float32)
    ms = f32(min_size) * f32(info_row[2])
    with np.errstate(all="ignore"):
        return (b[:, 2] - b[:, 0] + f32(1.0) >= ms) & (b[:, 3] - b[:, 1] + f32(1.0) >= ms)


def nonfinite_expected(c):
    """rows (image, anchor, delta kind, the kernel's box, numpy's box, clips agree, the kernel's keep flag, numpy's) of the non-finite deltas"""
    heads, info, _, _, dkind = case_inputs(c)
    rows = []
    for i in range(c.n):
        d4 = heads[i, :, :, :40].reshape(-1, 4)
        kb, nb = decode_restated(d4, info[i], c.hf, c.wf), decode_restated(d4, info[i], c.hf, c.wf, numpy_clip=True)
        kk, nk = keep_restated(kb, info[i], c.min_size), keep_restated(nb, info[i], c.min_size)
        for a in np.nonzero(dkind[i].reshape(-1))[0]:
            rows.append((i, int(a), DELTA_KINDS[dkind[i].reshape(-1)[a]], kb[a], nb[a], bool(np.array_equal(kb[a].view(np.uint32), nb[a].view(np.uint32))),
                         bool(kk[a]), bool(nk[a])))
    return rows


def swapped_row_shows(c):
    """for every image, every OTHER image's im_info row changes a box or a keep flag of it"""
    heads, info, _, _, _ = case_inputs(c)
    for i in range(c.n):
        d4 = heads[i, :, :, :40].reshape(-1, 4)
        own = decode_restated(d4, info[i], c.hf, c.wf)
        for j in range(c.n):
            if j == i:
                continue
            other = decode_restated(d4, info[j], c.hf, c.wf)
            if own.tobytes() == other.tobytes() and np.array_equal(keep_restated(own, info[i], c.min_size), keep_restated(other, info[j], c.min_size)):
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------
# the branch as a model (defect None: what the device must return)
# ---------------------------------------------------------------------------------------------------------------
def model(c, defect=None):
    """cls_prob (n, hf, wf, 20), bbox_pred (n, hf, wf, 40), boxes4 (n, per_img, 4), sorted_keys (n, npad), im_info (n, 3) of one call"""
    heads, info, vr, _, _ = case_inputs(c)
    cells, per_img = c.hf * c.wf, c.hf * c.wf * 10
    npad = C.next_pow2(per_img)
    flat = heads.reshape(-1)
    ld = 60 if defect == "head_ld_60" else 64
    base = (np.arange(c.n * cells) * ld)[:, None]
    a = np.arange(10)[None, :]
    rd = lambda off: flat[base + off]
    d = np.stack([rd(a * 4 + k) for k in range(4)], axis=-1)                       # (M, 10, 4)
    po = 40 + 2 * a + (2 if defect == "pair_of_next_anchor" else 0)
    s = np.stack([rd(po), rd(po + 1)], axis=-1)
    p = softmax_restated(s, max_subtraction=defect != "no_max_subtraction")
    stored = p[..., ::-1] if defect == "fg_bg_swapped_in_store" else p
    used = d[..., [0, 0, 2, 2]] if defect == "dy_dh_from_x_z" else d
    out = dict(cls_prob=stored.reshape(c.n, c.hf, c.wf, 20).copy(), bbox_pred=d.reshape(c.n, c.hf, c.wf, 40).copy(), boxes4=[], sorted_keys=[], im_info=info.copy())
    ycell = np.repeat(np.arange(c.hf), c.wf * 10)
    for i in range(c.n):
        row = info[i]
        if c.n <= 4 and defect == "select_image2_gets_row1" and i == 2:
            row = info[1]
        if c.n <= 4 and defect == "select_image3_gets_row2" and i == 3:
            row = info[2]
        b4 = decode_restated(used[i * cells: (i + 1) * cells].reshape(-1, 4), row, c.hf, c.wf)
        score = p[i * cells: (i + 1) * cells, :, 1].reshape(-1)
        keep = keep_restated(b4, row, c.min_size)
        if vr is not None:
            v = vr[i - 1] if defect == "valid_rows_of_previous_image" else vr[i]
            keep &= (ycell <= v) if defect == "valid_rows_le" else (ycell < v)
        if defect != "nan_score_kept":
            keep &= score == score
        key = ((~C.order_bits(score)).astype(np.uint64) << np.uint64(32)) | np.arange(per_img, dtype=np.uint64)
        out["boxes4"].append(b4)
        out["sorted_keys"].append(C.sort_ref(np.where(keep, key, KEY_INVALID), npad))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the checks, on the device's tensors or a model's
# ---------------------------------------------------------------------------------------------------------------
def check(c, got, report=None):
    """Raises AssertionError. report (a list): gets (case, pairs measured, the most floats an exponential is off, pairs where one is off at all,
    the worst |p - float64 softmax| as a fraction of the interval's half width, and in ulps of p)."""
    heads, info, vr, kind, dkind = case_inputs(c)
    per_img, npad = c.hf * c.wf * 10, C.next_pow2(c.hf * c.wf * 10)
    tag = c.name + ": "
    # rpn_bbox_pred: the rows' first 40 columns, bit for bit
    bbox = np.asarray(got["bbox_pred"], np.float32).reshape(c.n, c.hf, c.wf, 40)
    assert np.array_equal(bbox.view(np.uint32), heads[..., :40].view(np.uint32)), tag + "bbox_pred is not heads[:, :40]"
    # rpn_cls_prob_reshape
    s = heads[..., 40:60].reshape(-1, 2)
    p = np.asarray(got["cls_prob"], np.float32).reshape(-1, 2)
    nan, exact, want = softmax_expected(s)
    assert np.array_equal(np.isnan(p), np.stack([nan, nan], axis=-1)), tag + "cls_prob: NaN on %d values, expected on %d pairs" % (np.isnan(p).sum(), nan.sum())
    assert np.array_equal(p[exact].view(np.uint32), want[exact].view(np.uint32)), tag + "cls_prob: a tie is not 0.5 / 0.5 or a saturated pair not 1.0 / 0.0, as bits"
    rest = ~nan & ~exact
    ref = softmax64(s[rest])
    floats = softmax_exp_floats(s[rest], p[rest])
    lo, hi = softmax_interval(s[rest])
    p64 = p[rest].astype(np.float64)
    half = np.maximum(hi - ref, ref - lo)
    frac = float((np.abs(p64 - ref)[half > 0] / half[half > 0]).max()) if np.any(half > 0) else 0.0
    ulps = float((np.abs(p64 - ref) / np.spacing(p[rest]).astype(np.float64)).max()) if p64.size else 0.0
    if report is not None:
        report.append((c.name, int(rest.sum()), int(floats.max()) if floats.size else 0, int(np.count_nonzero(floats)), frac, ulps))
    assert floats.size == 0 or floats.max() <= EXP_ULPS, tag + "cls_prob of %d pairs needs an exponential %d floats off" % (np.count_nonzero(floats > EXP_ULPS), floats.max())
    assert np.all((p64 >= lo) & (p64 <= hi)), tag + "cls_prob outside the interval of an exponential %d float off" % EXP_ULPS
    # im_info on the device, for the kernels behind decode_kernel
    assert np.array_equal(np.asarray(got["im_info"], np.float32).view(np.uint32), info.view(np.uint32)), tag + "im_info on the device"
    ycell = np.repeat(np.arange(c.hf), c.wf * 10)
    for i in range(c.n):
        tag = "%s image %d: " % (c.name, i)
        # boxes: proposal_cells' decode (and its bound) on the image's OWN row over the finite anchors; the others as the kernel's operations give them
        fin = dkind[i].reshape(-1) == 0
        d4 = heads[i, :, :, :40].reshape(-1, 4)
        twin = np.where(fin[:, None], d4, f32(0.0))
        ref4, tol, ys = C.decode_ref(twin.reshape(-1), info[i], c.hf, c.wf)
        b4 = np.asarray(got["boxes4"][i], np.float32)
        assert np.array_equal(b4[:, 0::2].view(np.uint32), ref4[:, 0::2].view(np.uint32)), tag + "decode x1 / x2"
        ulps = C.exp_ulps_of(b4, ys)[fin]
        with np.errstate(all="ignore"):
            dy = np.abs(b4[:, 1::2].astype(np.float64) - ref4[:, 1::2].astype(np.float64)).max(axis=1)[fin]
        assert ulps.max() <= C.EXP_ULPS, tag + "decode y1 / y2 of %d anchors need exp %d floats off" % (np.count_nonzero(ulps > C.EXP_ULPS), ulps.max())
        assert np.all(dy <= tol[fin]), tag + "decode y off by %.3g x its bound" % (dy / tol[fin]).max()
        kern = decode_restated(d4, info[i], c.hf, c.wf)
        assert np.array_equal(b4[~fin].view(np.uint32), kern[~fin].view(np.uint32)), tag + "decode of a non-finite delta is not fmaxf(fminf(v, lim), 0)"
        # keys: the keep flag and key from the device's own boxes and fg probabilities; a NaN score and a cell below the image are KEY_INVALID
        score = p.reshape(c.n, per_img, 2)[i, :, 1]
        keys = C.keys_ref(b4, score, info[i], c.min_size)
        if vr is not None:
            keys = np.where(ycell < vr[i], keys, KEY_INVALID)
        assert np.all(keys[np.isnan(score)] == KEY_INVALID)
        skeys = np.asarray(got["sorted_keys"][i], np.uint64)
        assert skeys.shape == (npad,) and np.array_equal(skeys, C.sort_ref(keys, npad)), tag + "sorted keys"


def caught(c, defect):
    try:
        check(c, model(c, defect))
    except AssertionError:
        return True
    return False
