"""CPU: the cell table and the recipes of the first layer's kernel tests (tests/first_cells.py, run on the device by
tests/test_gpu_first_kernels.py), the float64 references against the oracle, the hooks' argument domain, and MUTANTS: numpy models of the
kernels with one defect each, to which the device tests' own judge functions are applied. Each must fail:
  * what moves a pixel, a column or an image (a one-byte shift, a dropped or doubled last column, a neighbour image's pixel, a poison byte)
    must fail the byte comparison it would meet on the device AND exceed the loosest per-mode bound of the normal recipe;
  * what writes the q-image wrongly (a frame pixel, a 1.0 in the other type's bits) must fail the q-image's bit comparison;
  * a wrong rounding of the store moves a value by one step, which no tolerance sees: it must fail the exact recipe's bit comparison."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
from oracle import conv1_q as Q
from oracle import network as N
import first_cells as C


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", C.FORMS)
def test_every_axis_value_is_covered_by_every_form(form):
    cells = C.cells_of(form)
    assert len(cells) == len(C.CELLS) == 23
    assert {w for _, n, h, w, _ in cells} == set(C.WIDTHS_SMALL + C.WIDTHS_WIDE)
    assert {h for _, n, h, w, _ in cells} == set(C.HEIGHTS) and {n for _, n, h, w, _ in cells} == {1, 3}
    for name, n, h, w, offs in cells:
        assert name == "%dx%dx%d" % (n, h, w) and offs[0] == 0 and set(offs) <= {0, 1, 2, 3}
        assert h >= 16 and w >= 16                                     # the product's domain
        if w in C.WIDTHS_WIDE:
            assert (n, h) == (1, 16), name                             # the segment seam needs no second row tile or image
    assert {o for c in cells for o in c[4]} == {0, 1, 2, 3}
    assert {w * 3 % 4 for _, n, h, w, _ in cells if w < 20} == {0, 1, 2, 3} and [w * 3 % 4 for w in (16, 19, 18, 17)] == [0, 1, 2, 3]
    assert {w % 4 for _, n, h, w, _ in cells} == {0, 1, 2, 3} == {h % 4 for _, n, h, w, _ in cells}
    # a batch whose images 1 and 2 start at every alignment but the pointer's own, and one whose images are all aligned
    assert {h * w * 3 % 4 for _, n, h, w, _ in cells if n == 3} == {0, 1, 2, 3}
    # every byte offset together with: each w * 3 % 4, a tile seam, a segment seam, a batch
    for sel in (lambda n, h, w: w * 3 % 4 == 0, lambda n, h, w: w * 3 % 4 == 1, lambda n, h, w: w * 3 % 4 == 3, lambda n, h, w: 64 < w < 128,
                lambda n, h, w: w > 1024, lambda n, h, w: n == 3):
        assert {o for _, n, h, w, offs in cells if sel(n, h, w) for o in offs} == {0, 1, 2, 3}
    assert {w // 1024 + (w % 1024 > 0) for _, n, h, w, _ in cells} == {1, 2, 3}      # row segments of image_to_q_kernel


def test_every_width_of_the_table_fuses():
    """launch_conv3x3 refuses the fused form where the layer's plan has a strip; conv1_2's pooled launch (Ci = Co = 64, no full map) never has one"""
    for prec in C.PRECS["fused"]:
        for _, n, h, w, _ in C.cells_of("fused"):
            p = B.conv3x3_plan(prec, n, h, w, 64, 64, True, keep_full=False, cu_count=256)
            assert (p.main, p.strip) == ("wr", "none"), (prec, n, h, w, p)


def test_hook_argument_domain():
    w1, b1, w2, b2 = C.normal_weights()
    u8 = np.zeros((1, 16, 16, 3), np.uint8)
    f32 = np.zeros((1, 16, 16, 3), np.float32)
    bad = [dict(images=u8, precision="split", form=0), dict(images=u8, precision="fp32", form=1), dict(images=u8, precision="fp32", form=2),
           dict(images=u8, precision="split", form=2), dict(images=f32, precision="bf16", form=2), dict(images=u8, precision="bf16", form=3),
           dict(images=u8, precision="bf16", form=0, byte_offset=4), dict(images=u8, precision="bf16", form=0, byte_offset=-1),
           dict(images=f32, precision="bf16", form=0, byte_offset=1), dict(images=np.zeros((1, 15, 16, 3), np.uint8), precision="bf16", form=0),
           dict(images=np.zeros((1, 16, 15, 3), np.uint8), precision="bf16", form=1), dict(images=u8, precision="bf16", form=0, want_q=True)]
    for kw in bad:
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.debug_conv1(w_hwio=w1, bias=b1, **kw)
        assert e.value.code == -1, kw
    for kw in (dict(precision="fp32"), dict(precision="split"), dict(precision="bf16", byte_offset=4)):
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.debug_conv1_fused(u8, w1, b1, w2, b2, **kw)
        assert e.value.code == -1, kw
    if B.device_count() == 0:       # the launches need a device
        for fn in (lambda: B.debug_conv1(u8, w1, b1, "bf16", 0), lambda: B.debug_conv1_fused(u8, w1, b1, w2, b2, "bf16")):
            with pytest.raises(ctpn_amd.CtpnError) as e:
                fn()
            assert e.value.code == -5
    assert B.conv1_q_shape(16, 16) == (20, 72) and B.conv1_q_shape(17, 65) == (28, 136)


# ---------------------------------------------------------------------------------------------------------------
# the recipes do what they are for
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16", "split"])
def test_exact_recipe_is_exact_in_any_order_and_full_of_ties(prec):
    blob, w, b, ref = C.exact_problem(prec, 1, 19, 67)
    assert C.exact_abs_bound(prec) < (2 ** 16 if prec == "split" else 2 ** 24)
    assert np.abs(blob).max() <= 152 and blob.min() >= -123 and np.abs(w).max() <= C.EXACT_WMAX[prec] and np.abs(b).max() <= 40
    assert np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() <= C.exact_abs_bound(prec)
    for a in (blob, w, b):                                             # every operand is its own bf16 hi half: lo = 0
        assert np.array_equal(C.from_bits16("bf16", C.bits16("bf16", a)), a)
    if prec == "fp16":
        assert np.abs(ref).max() < 65504
    # an fp32 accumulation in another order gives the same bits
    order = np.random.default_rng(0).permutation(27)
    xp = np.zeros((21, 69, 3), np.float32)
    xp[1:-1, 1:-1] = blob[0]
    acc = np.tile(b, (19, 67, 1)).astype(np.float32)
    for k in order:
        ky, kx, c = k // 9, k // 3 % 3, k % 3
        acc = (acc + xp[ky: ky + 19, kx: kx + 67, c: c + 1] * w[ky, kx, c]).astype(np.float32)
    assert np.array_equal(np.maximum(acc, 0).astype(np.float64), ref[0])
    if prec in ("bf16", "fp16"):
        share = C.tie_share(prec, ref)
        print("%s: %.1f %% of the positive outputs are exact ties, max %g" % (prec, 100 * share, ref.max()))
        assert share >= (0.10 if prec == "bf16" else 0.02)
    if prec == "split":                                                # hi + lo is the result, bit for bit
        s = C.store_bits("split", ref)
        assert np.array_equal(C.from_bits16("bf16", s[..., :64]).astype(np.float64) + C.from_bits16("bf16", s[..., 64:]), ref)


def test_references_agree_with_the_oracle():
    w1, b1, w2, b2 = C.normal_weights()
    images = C.normal_images(2, 17, 19)
    blob = N.image_blob(images)
    want = N.conv3x3_relu(blob, *C.thawed(w1, b1))
    assert C.rel_err(C.conv_ref64(blob, w1, b1), want.astype(np.float64)) < 2e-6
    assert float(want.max()) > 1.0 and (want == 0).mean() > 0.2                    # the scale of the arena's conv1_1, ReLU at work
    x2 = np.random.default_rng(1).standard_normal((1, 6, 7, 64)).astype(np.float32)
    assert C.rel_err(C.conv_ref64(x2, w2, b2), N.conv3x3_relu(x2, *C.thawed(w2, b2)).astype(np.float64)) < 2e-6
    for prec in ("bf16", "fp16"):
        q = C.q_model(images, prec)
        inner = q[:, 2: 2 + 17, 2: 2 + 19]
        assert np.array_equal(C.from_bits16(prec, inner), Q.q_image(images)[:, 2:-2, 2:-2])
        frame = np.ones(q.shape[:3], bool)
        frame[:, 2: 2 + 17, 2: 2 + 19] = False
        assert (q[frame] == C.FILL16).all() and q.shape[1:] == B.conv1_q_shape(17, 19) + (4,)
        C.judge_q(prec, q, images, prec)
        # the two oracle forms the device's q form is held to agree with each other within the judges' own criteria
        C.judge_ulp(prec, Q.conv1_1_from_q(images, w1, b1, prec), Q.reference_on_rounded_weights(images, w1, b1, prec), prec)


def test_store_bits_is_the_types_rounding():
    v = np.array([[[[257.0, 258.0, 259.0, 2049.0, 2051.0, 4098.0, 4102.0, 3.0]]]])
    assert C.from_bits16("bf16", C.store_bits("bf16", v)).ravel().tolist() == [256.0, 258.0, 260.0, 2048.0, 2048.0, 4096.0, 4096.0, 3.0]
    assert C.from_bits16("fp16", C.store_bits("fp16", v)).ravel().tolist() == [257.0, 258.0, 259.0, 2048.0, 2052.0, 4096.0, 4104.0, 3.0]
    assert C.from_bits16("bf16", C.store_bits("bf16", v, "half_up")).ravel().tolist()[:3] == [258.0, 258.0, 260.0]
    assert C.tie_share("bf16", v) == 2 / 8 and C.tie_share("fp16", v) == 4 / 8


# ---------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------
def _fails(judge, *args):
    with pytest.raises(AssertionError):
        judge(*args)


def _conv1(images_u8):
    w1, b1, _, _ = C.normal_weights()
    return C.conv_ref64(N.image_blob(images_u8), w1, b1).astype(np.float32)


def _moved_pixels_fail(what, images, mutant_images):
    """a defect that is a changed input image: the q-image's bit comparison, the byte comparison with the unshifted run and the normal
    recipe's loosest bound (bf16's) must each fail"""
    good, bad = _conv1(images), _conv1(mutant_images)
    C.judge_same_bytes(what, good, _conv1(images))
    C.judge_bound(what, C.from_bits16("bf16", C.bits16("bf16", good)), good.astype(np.float64), C.BOUND["bf16"])
    _fails(C.judge_same_bytes, what, bad, good)
    _fails(C.judge_same_bytes, what, C.bits16("bf16", bad), C.bits16("bf16", good))
    _fails(C.judge_bound, what, bad, good.astype(np.float64), C.BOUND["bf16"])
    for prec in ("bf16", "fp16"):
        _fails(C.judge_q, what, C.q_model(mutant_images, prec), images, prec)


def test_mutant_one_byte_shift_at_offset_1():
    images = C.normal_images(1, 17, 17)
    flat = np.concatenate([[C.POISON], images.ravel()[:-1]]).astype(np.uint8)      # every byte read one byte early: the poison byte in front comes in
    _moved_pixels_fail("shift", images, flat.reshape(images.shape))


def test_mutant_poison_byte_used_as_a_pixel():
    images = C.normal_images(1, 16, 19).copy()
    images[0, -1, -1, 2] = 250                                                      # the image's last byte, then the poison byte behind it in its place
    mutant = images.copy()
    mutant[0, -1, -1, 2] = C.POISON
    _moved_pixels_fail("poison", images, mutant)


def test_mutant_neighbour_images_pixel_at_a_batch_seam():
    images = C.normal_images(3, 17, 19).copy()
    images[1, 0, 0] = (250, 5, 250)
    images[0, -1, -1] = (5, 250, 5)
    mutant = images.copy()
    mutant[0, -1, -1] = images[1, 0, 0]                                             # image 0's last pixel read from image 1's first
    _moved_pixels_fail("seam", images, mutant)
    # ... which is what "image i of a batch against the image alone" compares
    _fails(C.judge_same_bytes, "seam", _conv1(mutant)[0:1], _conv1(images[0:1]))


@pytest.mark.parametrize("defect", ["dropped", "doubled"])
def test_mutant_last_live_column_of_a_tile(defect):
    for w in (65, 67):
        images = C.normal_images(1, 18 if w == 65 else 19, w)
        good = _conv1(images)
        bad = good.copy()
        bad[:, :, w - 1] = 0 if defect == "dropped" else good[:, :, w - 2]
        _fails(C.judge_bound, defect, bad, good.astype(np.float64), C.BOUND["bf16"])
        _fails(C.judge_ulp, defect, bad, good.astype(np.float64), "bf16")
        _fails(C.judge_same_bytes, defect, bad, good)
    blob, wts, b, ref = C.exact_problem("bf16", 1, 18, 65)
    bad = ref.copy()
    bad[:, :, 64] = 0 if defect == "dropped" else ref[:, :, 63]
    _fails(C.judge_exact, defect, "bf16", bad.astype(np.float32), C.store_bits("bf16", bad), ref)
    _fails(C.judge_exact, defect, "fp32", bad.astype(np.float32), None, ref)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_mutant_q_image_frame_pixel_written(prec):
    images = C.normal_images(1, 17, 17)
    C.judge_q(prec, C.q_model(images, prec), images, prec)
    _fails(C.judge_q, prec, C.q_model(images, prec, "frame_written"), images, prec)


def test_mutant_one_in_bf16_bits_in_the_fp16_q_image():
    images = C.normal_images(1, 16, 16)
    _fails(C.judge_q, "one", C.q_model(images, "fp16", "one_bf16_in_fp16"), images, "fp16")
    # what the conv would make of it: P = 1.875 instead of 1.0 scales the bias and mean terms only -- small against the pixels, so the
    # bit comparison of the q-image is the check that sees it for certain
    assert C.from_bits16("fp16", np.uint16(0x3F80)) == 1.875


@pytest.mark.parametrize("prec", ["bf16", "fp16", "split"])
def test_mutant_round_half_up_breaks_the_exact_recipe(prec):
    blob, w, b, ref = C.exact_problem(prec, 1, 19, 67)
    good = C.store_bits(prec, ref)
    C.judge_exact(prec, prec, ref.astype(np.float32), good, ref)
    bad = C.store_bits(prec, ref, "half_up")
    differ = float((bad != good).mean())
    print("%s: round-half-up changes %.1f %% of the stored values" % (prec, 100 * differ))
    assert differ >= (0.01 if prec == "fp16" else 0.03)
    _fails(C.judge_exact, prec, prec, ref.astype(np.float32), bad, ref)
    if prec != "split":      # ... by one step of the type: what the normal recipe's bound does not see
        v = C.from_bits16(prec, bad).astype(np.float64)
        assert C.rel_err(v, ref) < C.BOUND[prec]
