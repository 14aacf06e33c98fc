"""GPU (-m gpu): the first layer's kernels, each alone on caller data through its test hook -- conv_first_kernel (form valu),
conv_first_mfma_kernel (mfma), image_to_q_kernel + conv_first_p_kernel (q) through ctpn_debug_conv1, and image_to_q_kernel + the conv1_1
producer inside conv3x3_wr_kernel<FUSE> (fused) through ctpn_debug_conv1_fused. tests/first_cells.py holds the cells, the recipes, the float64
references and the judges; tests/test_first_cells.py (CPU) keeps the table true and shows that a defective kernel would not pass the judges.

The hooks put the image at byte 64 + offset of a block of poison bytes, fill the bordered output map and the q-image with 0xC3 and fail
themselves (CTPN_ERR_STATE) when a border pixel, a guard row or a frame pixel of the q-image changed. On top of that, per cell:
  q-image        every 16-bit value of the whole q-image: (p - round(mean), 1.0) in the type's bits at the image's pixels, the fill elsewhere
  alignment      the image at byte offsets 1, 2, 3 stores the bytes of offset 0; image i of a batch stores the bytes of that image run alone
  feeds          valu and mfma: the uint8 feed stores the bytes of the float feed of fp32(p - mean), in every precision
  exact recipe   valu and mfma on integer data: the stored values are the round-to-nearest-even of the float64 result, bit for bit
  normal recipe  valu and mfma within the project's per-mode bound of oracle/network.py; q within one output rounding step of
                 oracle/conv1_q.py::reference_on_rounded_weights and equal to conv1_1_from_q except on at most 2e-3 of the values
  fused          pool1 of the fused chain is, byte for byte, ctpn_debug_conv3x3's pool of form q's conv1_1, and within the bound of the oracle
  repeat         a second run stores the same bytes

Every test prints one line per cell: FIRST <kernel> <cell> <shape> <measured> <bound>. Measured on an MI355X: profiles/first_kernel_cells.txt
(798 lines). No byte comparison of any cell differs by a bit: the q-image at every byte offset, every offset against offset 0, every image of a
batch against the image alone, the uint8 feed against the float feed (valu and mfma, bf16 and fp16 included), the exact recipe (13 - 15 % of the
positive outputs exact fp16 ties, 21 - 22 % bf16 ties), the fused pool against the stored form, and every second run. Worst on the normal
recipe, against the bound:
    valu fp32 2.0e-7 of 5e-6, bf16 3.1e-3 of 8e-3, fp16 4.1e-4 of 1.5e-3; mfma bf16 3.1e-3, fp16 4.1e-4, split 7.5e-6 of 2e-5;
    q against the reference on rounded weights: bf16 0.63 and fp16 0.96 of one output rounding step; against the specification 1.4e-5 (bf16)
    and 9.4e-5 (fp16) of the values differ, of 2e-3;
    fused pool1 against the oracle: bf16 3.4e-3 of 8e-3, fp16 4.1e-4 of 1.5e-3.
The new tests exposed no kernel defect."""
import numpy as np
import pytest

from ctpn_amd import _binding as B
from oracle import conv1_q as Q
from oracle import network as N
import first_cells as C

pytestmark = pytest.mark.gpu

CONV1_CASES = [(f, p) for f in ("valu", "mfma", "q") for p in C.PRECS[f]]
ALL_CASES = CONV1_CASES + [("fused", p) for p in C.PRECS["fused"]]
FLOAT_CASES = [(f, p) for f in C.FLOAT_FEED for p in C.PRECS[f]]
_ids = lambda cases: ["%s-%s" % c for c in cases]


def _run(form, prec, images, weights, off=0):
    """one hook call -> the arrays whose bytes the kernels stored: (fp32 view, stored 16-bit values or None, q-image or None)"""
    w1, b1, w2, b2 = weights
    if form == "fused":
        out, bits = B.debug_conv1_fused(images, w1, b1, w2, b2, prec, byte_offset=off)
        return out, bits, None
    return B.debug_conv1(images, w1, b1, prec, C.FORM_ID[form], byte_offset=off, want_bits=prec != "fp32", want_q=form == "q")


def _same(what, a, b):
    cnt = 0
    for x, y in zip(a, b):
        assert (x is None) == (y is None), what
        if x is not None:
            cnt += C.judge_same_bytes(what, x, y)
    return cnt


def _line(kernel, cell, shape, measured, bound):
    print("FIRST %-12s %-10s %-12s %s  %s" % (kernel, cell, shape, measured, bound))


def _shape(n, h, w, off=None):
    return "%dx%dx%d" % (n, h, w) + ("" if off is None else "+%d" % off)


@pytest.mark.parametrize("prec", C.PRECS["q"])
def test_q_image_is_the_images_pixels_and_nothing_else(prec):
    for name, n, h, w, offs in C.cells_of("q"):
        images = C.normal_images(n, h, w)
        for off in offs:
            q = _run("q", prec, images, C.normal_weights(), off)[2]
            cnt = C.judge_q((prec, name, off), q, images, prec)
            _line("q_image/" + prec, name, _shape(n, h, w, off), "0 of %d values differ" % cnt, "exact")


@pytest.mark.parametrize("form,prec", ALL_CASES, ids=_ids(ALL_CASES))
def test_alignment_of_the_image_pointer_and_of_an_image_in_a_batch_changes_no_byte(form, prec):
    wts = C.normal_weights()
    for name, n, h, w, offs in C.cells_of(form):
        images = C.normal_images(n, h, w)
        base = _run(form, prec, images, wts, 0)
        cnt = 0
        for off in offs[1:]:
            cnt += _same((form, prec, name, "offset", off), _run(form, prec, images, wts, off), base)
        for i in range(n if n > 1 else 0):
            alone = _run(form, prec, images[i: i + 1], wts, 0)
            cnt += _same((form, prec, name, "image", i), alone, tuple(None if a is None else a[i: i + 1] for a in base))
        if cnt:
            _line("%s/%s" % (form, prec), name, _shape(n, h, w), "offsets %s, %d images alone: 0 of %d values differ" % (",".join(map(str, offs)), n if n > 1 else 0, cnt), "exact")


@pytest.mark.parametrize("form,prec", FLOAT_CASES, ids=_ids(FLOAT_CASES))
def test_uint8_feed_stores_the_bytes_of_the_float_feed(form, prec):
    wts = C.normal_weights()
    for name, n, h, w, _offs in C.cells_of(form):
        images = C.normal_images(n, h, w)
        cnt = _same((form, prec, name), _run(form, prec, images, wts), _run(form, prec, N.image_blob(images), wts))
        _line("%s/%s" % (form, prec), name, _shape(n, h, w), "uint8 against float feed: 0 of %d values differ" % cnt, "exact")


@pytest.mark.parametrize("form,prec", FLOAT_CASES, ids=_ids(FLOAT_CASES))
def test_exact_recipe_is_stored_round_to_nearest_even_bit_for_bit(form, prec):
    for name, n, h, w, _offs in C.cells_of(form):
        blob, w1, b1, ref = C.exact_problem(prec, n, h, w)
        wts = (w1, b1, None, None)
        got = _run(form, prec, blob, wts)
        cnt = C.judge_exact((form, prec, name), prec, got[0], got[1], ref)
        _same((form, prec, name, "again"), _run(form, prec, blob, wts), got)
        ties = "" if prec in ("fp32", "split") else " (%.0f %% ties)" % (100 * C.tie_share(prec, ref))
        _line("%s/%s" % (form, prec), name, _shape(n, h, w), "exact recipe: 0 of %d values differ%s" % (cnt, ties), "exact")


@pytest.mark.parametrize("form,prec", CONV1_CASES, ids=_ids(CONV1_CASES))
def test_normal_recipe_is_within_the_projects_bounds(form, prec):
    w1, b1, _w2, _b2 = wts = C.normal_weights()
    for name, n, h, w, _offs in C.cells_of(form):
        images = C.normal_images(n, h, w)
        got = _run(form, prec, images, wts)
        if form == "q":
            steps = C.judge_ulp((form, prec, name), got[0], Q.reference_on_rounded_weights(images, w1, b1, prec), prec)
            share = C.judge_spec((form, prec, name), got[0], Q.conv1_1_from_q(images, w1, b1, prec), prec)
            _same((form, prec, name, "again"), _run(form, prec, images, wts), got)
            _line("q/" + prec, name, _shape(n, h, w), "%.3f steps of the reference, %.2e differ from the specification" % (steps, share), "1 step, %.0e" % C.SPEC_SHARE)
        else:
            e = C.judge_bound((form, prec, name), got[0], N.conv3x3_relu(N.image_blob(images), *C.thawed(w1, b1)), C.BOUND[prec])
            _line("%s/%s" % (form, prec), name, _shape(n, h, w), "%.3e" % e, "%.1e" % C.BOUND[prec])


@pytest.mark.parametrize("prec", C.PRECS["fused"])
def test_fused_pool1_is_the_stored_forms_bytes_and_within_the_bound(prec):
    w1, b1, w2, b2 = wts = C.normal_weights()
    for name, n, h, w, _offs in C.cells_of("fused"):
        images = C.normal_images(n, h, w)
        pool, bits, _ = got = _run("fused", prec, images, wts)
        c11 = _run("q", prec, images, wts)[0]
        # c11 is representable in the type: the hook's rounding of its input is the identity
        stored = B.debug_conv3x3(c11, w2, b2, prec, impl=1, fuse_pool=True, want_full=False)[1]
        cnt = C.judge_same_bytes((prec, name, "stored form"), bits, C.bits16(prec, stored))
        assert np.array_equal(C.from_bits16(prec, bits), pool), (prec, name)
        e = C.judge_bound((prec, name), pool, N.maxpool2x2(N.conv3x3_relu(c11, *C.thawed(w2, b2))), C.BOUND[prec])
        _same((prec, name, "again"), _run("fused", prec, images, wts), got)
        _line("fused/" + prec, name, _shape(n, h, w), "0 of %d values differ from the stored form; oracle %.3e" % (cnt, e), "exact; %.1e" % C.BOUND[prec])
