"""The first layer's kernels alone (ctpn_debug_conv1, ctpn_debug_conv1_fused): the cell table, the recipes, the float64 references and the judge
functions of tests/test_gpu_first_kernels.py (-m gpu). tests/test_first_cells.py (CPU) keeps the table true and applies the judges to numpy
models of the likely defects.

Forms: valu = conv_first_kernel, mfma = conv_first_mfma_kernel, q = image_to_q_kernel + conv_first_p_kernel, fused = image_to_q_kernel + the
conv1_1 producer inside conv3x3_wr_kernel<FUSE> (csrc/conv_first.hip, conv_first_q.hip, conv3x3_wr.h).

A cell is (n, h, w, byte offsets of the uint8 image pointer). Every form runs every cell; the float feed has no byte offset. What the shapes are for:
  w * 3 % 4        0, 3, 2, 1 at w = 16, 17, 18, 19: the alignment of every image row but the first
  w % 4            the four-pixel groups of conv_first_kernel and image_to_q_kernel end with 4, 1, 2, 3 live pixels (16, 17, 18, 19)
  the 64-pixel tile seam (conv_first_*: 64 x 4 tiles; conv_first_p: 64 pixels per wave)     63, 64, 65, 67, and again 128, 129
  the 1024-pixel row segment of image_to_q_kernel      1023, 1024, 1025, 1027; 2051 = three segments (h = 16, n = 1 only)
  h % 4            the 4-row tiles end with 4, 1, 2, 3 live rows (16, 17, 18, 19)
  n = 3            image i starts i * h * w * 3 bytes behind the pointer: h * w * 3 % 4 = 1, 2, 3 puts images 1 and 2 at other alignments
  byte offset      0 .. 3 of the pointer itself
"""
import functools

import numpy as np

from oracle.rounding import bf16_round, fp16_round

FORMS = ("valu", "mfma", "q", "fused")
FORM_ID = {"valu": 0, "mfma": 1, "q": 2}
PRECS = {"valu": ("fp32", "bf16", "fp16"), "mfma": ("bf16", "fp16", "split"), "q": ("bf16", "fp16"), "fused": ("bf16", "fp16")}
FLOAT_FEED = ("valu", "mfma")                 # the forms that also take the mean-subtracted blob

ALL4 = (0, 1, 2, 3)
CELLS = {
    # name: (n, h, w, byte offsets)                       w * 3 % 4, h * w * 3 % 4
    "1x16x16": (1, 16, 16, ALL4),                       # 0, 0: one tile, whole four-pixel groups
    "1x17x17": (1, 17, 17, ALL4),                       # 3, 3
    "1x18x18": (1, 18, 18, (0,)),                       # 2, 0
    "1x19x19": (1, 19, 19, ALL4),                       # 1, 3
    "1x16x19": (1, 16, 19, (0,)),
    "3x16x16": (3, 16, 16, (0,)),                       # 0, 0: every image aligned
    "3x17x19": (3, 17, 19, ALL4),                       # 1, 1: images at +1, +2
    "3x17x18": (3, 17, 18, (0,)),                       # 2, 2: images at +2, +0
    "3x19x17": (3, 19, 17, (0, 3)),                     # 3, 1: images at +1, +2
    "3x17x17": (3, 17, 17, (0, 2)),                     # 3, 3: images at +3, +2
    "1x16x63": (1, 16, 63, (0, 1)),
    "1x17x64": (1, 17, 64, (0,)),
    "1x18x65": (1, 18, 65, ALL4),
    "1x19x67": (1, 19, 67, (0, 2)),
    "3x17x65": (3, 17, 65, (0, 3)),                     # 3, 3
    "1x16x128": (1, 16, 128, (0,)),
    "1x17x129": (1, 17, 129, (0, 1)),
    "3x19x129": (3, 19, 129, (0,)),                     # 3, 1
    "1x16x1023": (1, 16, 1023, (0, 3)),
    "1x16x1024": (1, 16, 1024, (0, 1)),
    "1x16x1025": (1, 16, 1025, ALL4),
    "1x16x1027": (1, 16, 1027, (0, 2)),
    "1x16x2051": (1, 16, 2051, (0, 1)),
}
WIDTHS_SMALL = (16, 17, 18, 19, 63, 64, 65, 67, 128, 129)
WIDTHS_WIDE = (1023, 1024, 1025, 1027, 2051)
HEIGHTS = (16, 17, 18, 19)

# the project's per-mode bounds (tests/tail_cells.py::BOUND, tests/test_gpu_conv_forms.py): max |diff| over the map's max |value|, no element beyond 4 x
BOUND = {"fp32": 5e-6, "split": 2e-5, "fp16": 1.5e-3, "bf16": 8e-3}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}      # one rounding step of the output type at the map's maximum (tests/test_gpu_fuse.py)
SPEC_SHARE = 2e-3                                   # share of values that may differ from oracle/conv1_q.py's form by that step (tests/test_gpu_fuse.py)
FILL16 = 0xC3C3                                     # the hooks' fill byte 0xC3, as a 16-bit value
POISON = 0x47                                       # the hooks' poison byte around the image
MEANS_INT = np.array([103.0, 116.0, 123.0])         # round(PIXEL_MEANS), BGR
ONE_BITS = {"bf16": 0x3F80, "fp16": 0x3C00}


def thawed(*arrays):
    """writable copies of frozen arrays, for torch (oracle/network.py)"""
    return tuple(np.array(a) for a in arrays)


def cells_of(form):
    """[(name, n, h, w, offsets)] of one form, small shapes first"""
    return [(k,) + v for k, v in sorted(CELLS.items(), key=lambda kv: (kv[1][0] * kv[1][1] * kv[1][2], kv[0]))]


def _seed(n, h, w, salt):
    return ((salt * 64 + n) * 8192 + h) * 8192 + w


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------
def bits16(prec, a):
    """float values -> the bits of the type's round-to-nearest-even (split precision: the hi half)"""
    a = np.asarray(a, np.float32)
    if prec == "fp16":
        return a.astype(np.float16).view(np.uint16)
    return (bf16_round(a).view(np.uint32) >> 16).astype(np.uint16)


def from_bits16(prec, b):
    b = np.asarray(b, np.uint16)
    if prec == "fp16":
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def store_bits(prec, ref, mode="rne"):
    """float64 results that are exact in fp32 -> the stored 16-bit values: (n, h, w, 64), split precision (n, h, w, [hi | lo]).
    mode half_up: to nearest, ties toward +infinity (the defect model of tests/test_first_cells.py)"""
    ref = np.asarray(ref, np.float64)
    f32 = ref.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), ref)
    hi = bits16(prec, f32)
    if mode == "half_up":
        down = from_bits16(prec, hi).astype(np.float64)
        nxt = from_bits16(prec, (hi + 1).astype(np.uint16)).astype(np.float64)      # positive values: the next value up is the next bit pattern
        tie = (ref > 0) & (down < ref) & (ref - down == nxt - ref)
        hi = np.where(tie, hi + 1, hi).astype(np.uint16)
    if prec != "split":
        return hi
    lo = bits16("bf16", (ref - from_bits16("bf16", hi).astype(np.float64)).astype(np.float32))
    return np.concatenate([hi, lo], axis=-1)


def tie_share(prec, ref):
    """share of the positive results that lie exactly between two neighbouring values of the type"""
    ref = np.asarray(ref, np.float64)
    pos = ref[ref > 0]
    hi = bits16(prec, pos.astype(np.float32))
    near = from_bits16(prec, hi).astype(np.float64)
    other = from_bits16(prec, np.where(near < pos, hi + 1, hi - 1).astype(np.uint16)).astype(np.float64)
    return float(((near != pos) & (np.abs(near - pos) == np.abs(other - pos))).mean())


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def conv_ref64(x_nhwc, w_hwio, bias, relu=True):
    """3x3 'SAME' cross-correlation + bias (+ ReLU) in float64: the layer of oracle/network.py::conv3x3_relu"""
    x = np.asarray(x_nhwc, np.float64)
    w = np.asarray(w_hwio, np.float64)
    n, h, wd, _ = x.shape
    xp = np.zeros((n, h + 2, wd + 2, x.shape[3]), np.float64)
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((n, h, wd, w.shape[3]), np.float64) + np.asarray(bias, np.float64)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky: ky + h, kx: kx + wd] @ w[ky, kx]
    return np.maximum(out, 0.0) if relu else out


def q_model(images_u8, prec, defect=None):
    """The q-image as ctpn_debug_conv1 returns it: (n, Hq, Wq, 4) uint16, image pixel (y, x) at (y + 2, x + 2) = (p - round(mean), 1.0) in the
    type's bits, everything else the hook's fill. defect: frame_written | one_bf16_in_fp16"""
    im = np.asarray(images_u8)
    n, h, w, _ = im.shape
    hq, wq = (h + 7) // 8 * 8 + 4, (w + 63) // 64 * 64 + 8
    q = np.full((n, hq, wq, 4), FILL16, np.uint16)
    q[:, 2: 2 + h, 2: 2 + w, :3] = bits16(prec, (im.astype(np.float64) - MEANS_INT).astype(np.float32))
    q[:, 2: 2 + h, 2: 2 + w, 3] = ONE_BITS["bf16" if defect == "one_bf16_in_fp16" else prec]
    if defect == "frame_written":
        q[n - 1, 2 + h - 1, 2 + w] = 0            # the pixel right of the last image pixel, as the fourth pixel of a full 16-byte store would
    return q


# ---------------------------------------------------------------------------------------------------------------
# recipes
# ---------------------------------------------------------------------------------------------------------------
EXACT_WMAX = {"fp32": 3, "bf16": 3, "split": 3, "fp16": 8}      # fp16 needs sums beyond 2048 to have ties


@functools.lru_cache(maxsize=None)
def exact_problem(prec, n, h, w):
    """(blob (n, h, w, 3) fp32, weights (3, 3, 3, 64), bias (64,), float64 conv1_1): integers -- the blob in [-123, 152] like p - round(mean),
    weights in [-wmax, wmax], a bias in [-40, 40] -- so that every product and every partial sum is an integer below 2^24 (exact in fp32 in
    any order; below 2^16 for wmax 3, which makes hi + lo of split precision exact as well) and every operand's bf16 lo half is 0. The only
    rounding left is the output store."""
    rng = np.random.default_rng(_seed(n, h, w, 3 if prec == "fp16" else 2))
    wmax = EXACT_WMAX[prec]
    blob = rng.integers(-123, 153, size=(n, h, w, 3)).astype(np.float32)
    wts = rng.integers(-wmax, wmax + 1, size=(3, 3, 3, 64)).astype(np.float32)
    bias = rng.integers(-40, 41, size=(64,)).astype(np.float32)
    return _frozen(blob, wts, bias, conv_ref64(blob, wts, bias))


def exact_abs_bound(prec):
    """the largest |partial sum| the exact recipe can reach"""
    return 152 * 27 * EXACT_WMAX[prec] + 40


@functools.lru_cache(maxsize=None)
def normal_weights():
    """conv1_1 and conv1_2 at the benchmark arena's scale (ctpn_amd.weights.make_synthetic_arena: He-scaled truncated normals, conv1_1 times
    1 / 64), with non-zero biases"""
    rng = np.random.default_rng(11)
    w1 = (np.clip(rng.standard_normal((3, 3, 3, 64)), -2, 2) * np.sqrt(2.0 / 27.0) / 64.0).astype(np.float32)
    b1 = rng.uniform(-0.3, 0.3, 64).astype(np.float32)
    w2 = (np.clip(rng.standard_normal((3, 3, 64, 64)), -2, 2) * np.sqrt(2.0 / 576.0)).astype(np.float32)
    b2 = rng.uniform(-0.1, 0.1, 64).astype(np.float32)
    return _frozen(w1, b1, w2, b2)


@functools.lru_cache(maxsize=None)
def normal_images(n, h, w):
    import ctpn_amd
    return _frozen(ctpn_amd.weights.synthetic_images(n, h, w, 100 + (h * 31 + w) % 997))[0]


# ---------------------------------------------------------------------------------------------------------------
# judges: what tests/test_gpu_first_kernels.py asserts. Each returns the figure it prints.
# ---------------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def judge_q(what, q_got, images_u8, prec):
    """the q-image, bit for bit: the image's pixels, and nothing else written. Returns the number of 16-bit values compared."""
    want = q_model(images_u8, prec)
    assert q_got.shape == want.shape and q_got.dtype == np.uint16, (what, q_got.shape, want.shape)
    bad = np.argwhere(q_got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [hex(int(q_got[tuple(i)])) for i in bad[:4]], [hex(int(want[tuple(i)])) for i in bad[:4]])
    return want.size


def judge_same_bytes(what, a, b):
    """two runs that must store the same bytes. Returns the number of values compared."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    av, bv = a.view(np.uint8), b.view(np.uint8)
    bad = np.argwhere((av != bv).reshape(a.shape + (-1,)).any(axis=-1))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())
    return a.size


def judge_exact(what, prec, got, bits, ref):
    """the exact recipe: the stored values are the type's round-to-nearest-even of the float64 result, bit for bit (fp32: the result itself;
    split precision: hi + lo is the result and lo the residual). Returns the number of values compared."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if prec == "fp32":
        bad = np.argwhere(got.astype(np.float64) != ref)
    else:
        want = store_bits(prec, ref)
        assert bits.shape == want.shape, (what, bits.shape, want.shape)
        bad = np.argwhere(bits != want)
        if prec == "split" and bad.size == 0:
            bad = np.argwhere(got.astype(np.float64) != ref)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [float(got[tuple(i[:3]) + (int(i[3]) % 64,)]) for i in bad[:4]],
                           [float(ref[tuple(i[:3]) + (int(i[3]) % 64,)]) for i in bad[:4]])
    return ref.size


def judge_bound(what, got, ref, tol):
    """tests/test_gpu_tail_kernels.py::_judge: the whole map within tol of the map's max |value|, no element beyond 4 x tol"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    e = rel_err(got, ref)
    assert e < tol, (what, e, tol)
    assert not (np.abs(got - ref) > 4 * tol * float(np.abs(ref).max())).any(), what
    return e


def judge_ulp(what, got, want, prec):
    """tests/test_gpu_fuse.py: within one rounding step of the output type at the map's maximum. Returns the worst difference in steps."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ulp = float(np.abs(want).max()) * ULP[prec]
    e = float(np.abs(got.astype(np.float64) - want).max())
    assert e <= ulp, (what, e / ulp)
    return e / ulp


def judge_spec(what, got, want, prec):
    """tests/test_gpu_fuse.py: equal to oracle/conv1_q.py's form value for value, except on rounding boundaries. Returns the share that differs."""
    share = float((got != want).mean())
    assert share <= SPEC_SHARE, (what, share)
    judge_ulp(what, got, want, prec)
    return share
