"""GPU (-m gpu): the network with non-zero biases and with saturated LSTM gates / pair softmax.

Every other GPU test that runs the whole network loads the benchmark arena (ctpn_amd.make_synthetic_arena(0)): all 19 bias vectors exactly
zero, conv1_1 scaled by 1/64 so that no gate leaves sigmoid(+-1.6). This file runs the same kernels on the two stress recipes of
tests/util.py (stress_arena; their conditions and the mutants that give "biased" its teeth are CPU tests in tests/test_oracle.py):

  "biased"     the benchmark arena's scale, every bias non-zero: conv epilogue biases, the three conv1_1 bias forms (accumulator init of
               conv_first_kernel, weight row x constant-1 slot of the MFMA hi+lo kernel, the (hi, lo) V pair of the q-image form), the LSTM
               bias through the gate-column permutation (LDS and global-memory forms of lstm_pre, igemm's epilogue), b_fc, b_h as 40 | 20 and
               the folded bias b' = b_fc W_h + b_h;
  "fullscale"  image_gain 1.0: lstm_pre in [-90, 100] (exp overflows: fast_sigmoid = rcp(1 + exp(-x)), fast_tanh = 1 - 2 rcp(exp(2x) + 1),
               the library forms, the fp16 lstm_pre of the 16-bit modes), cls_prob from 1e-13 to exactly 1.0f with many exact ties.

Every comparison is a device tensor against oracle/network.py, oracle/conv1_q.py or oracle/postproc.py applied to the DEVICE's previous
tensor, so each check isolates one launch. Nothing here reads anything outside the repository.

Bounds: the ones the suite already applies to the same tensor in the same mode (TOL / REC_TOL below). What the device measured on an
MI355X (max over the shapes of the named test; conv, lstm_pre, lstm_o, heads: max |diff| over the map's max; recurrence: max |diff|):

  tensor, form                                         mode   arena      measured  bound    worst shape  bound from
  bbox_pred, end to end                                fp32   fullscale  3.24e-05  0.001    1x600x900    north star (1e-3)
  cls_prob, end to end                                 fp32   fullscale  8.95e-05  0.001    1x600x900    issue / north star
  cls_prob, end to end                                 split  biased     3.68e-05  0.0002   1x600x900    issue / north star
  conv (worst of 14)                                   fp32   biased     2.49e-06  5e-06    2x70x100     existing (layer walks)
  conv (worst of 14)                                   fp32   fullscale  2.92e-06  5e-06    2x70x100     existing (layer walks)
  conv (worst of 14)                                   split  biased     1.08e-05  1.2e-05  1x600x900    existing (layer walks)
  conv (worst of 14)                                   split  fullscale  9.35e-06  1.2e-05  2x70x100     existing (layer walks)
  conv (worst of 14)                                   bf16   biased     0.00414   0.008    1x600x900    existing (layer walks)
  conv (worst of 14)                                   bf16   fullscale  0.00413   0.008    2x70x100     existing (layer walks)
  conv (worst of 14)                                   fp16   biased     0.000535  0.0015   2x70x100     existing (layer walks)
  conv (worst of 14)                                   fp16   fullscale  0.000519  0.0015   2x70x100     existing (layer walks)
  conv1_1, MFMA hi+lo, share != direct kernel (f32)    bf16   biased     0.00156   0.002    1x37x53      existing (test_gpu_parity)
  conv1_1, MFMA hi+lo, share != direct kernel (f32)    bf16   fullscale  0.00158   0.002    2x72x104     existing (test_gpu_parity)
  conv1_1, MFMA hi+lo, share != direct kernel (u8)     bf16   biased     0.00156   0.002    1x37x53      existing (test_gpu_parity)
  conv1_1, MFMA hi+lo, share != direct kernel (u8)     bf16   fullscale  0.00158   0.002    2x72x104     existing (test_gpu_parity)
  conv1_1, conv_first_kernel                           fp32   biased     1.67e-07  5e-06    1x16x19      existing (fp32 walk)
  conv1_1, conv_first_kernel                           fp32   fullscale  1.27e-07  5e-06    2x72x104     existing (fp32 walk)
  conv1_1, q-image, in output ulps                     bf16   biased     0.682     1        1x16x19      existing (test_gpu_fuse)
  conv1_1, q-image, in output ulps                     bf16   fullscale  0.674     1        1x16x19      existing (test_gpu_fuse)
  conv1_1, q-image, in output ulps                     fp16   biased     0.659     1        1x16x19      existing (test_gpu_fuse)
  conv1_1, q-image, in output ulps                     fp16   fullscale  0.672     1        1x16x19      existing (test_gpu_fuse)
  conv1_1, q-image, share != specification             bf16   biased     5.14e-05  0.002    1x16x19      existing (test_gpu_fuse)
  conv1_1, q-image, share != specification             bf16   fullscale  5.14e-05  0.002    1x16x19      existing (test_gpu_fuse)
  conv1_1, q-image, share != specification             fp16   biased     0.000103  0.002    1x16x19      existing (test_gpu_fuse)
  conv1_1, q-image, share != specification             fp16   fullscale  0.000136  0.002    2x72x104     existing (test_gpu_fuse)
  heads (bbox 40, cls 20)                              fp32   biased     9.31e-07  5e-06    2x70x100     existing (lstm_o's)
  heads (bbox 40, cls 20)                              fp32   fullscale  8.22e-07  5e-06    2x70x100     existing (lstm_o's)
  heads (bbox 40, cls 20)                              split  biased     1.25e-06  5e-06    1x600x900    existing (lstm_o's)
  heads (bbox 40, cls 20)                              split  fullscale  7.65e-07  5e-06    2x70x100     existing (lstm_o's)
  heads, folded against two GEMMs                      bf16   biased     9.98e-07  2e-05    2x150x230    existing
  heads, folded against two GEMMs                      bf16   fullscale  1.29e-06  2e-05    2x150x230    existing
  heads, folded against two GEMMs                      fp16   biased     9.38e-07  2e-05    2x150x230    existing
  heads, folded against two GEMMs                      fp16   fullscale  8.3e-07   2e-05    2x150x230    existing
  heads, folded, against the oracle                    bf16   biased     8.8e-07   1e-05    2x150x230    issue (1e-5 x scale)
  heads, folded, against the oracle                    bf16   fullscale  5.55e-07  1e-05    2x150x230    issue (1e-5 x scale)
  heads, folded, against the oracle                    fp16   biased     7.91e-07  1e-05    2x150x230    issue (1e-5 x scale)
  heads, folded, against the oracle                    fp16   fullscale  4.61e-07  1e-05    2x150x230    issue (1e-5 x scale)
  heads, two GEMMs, against the oracle                 bf16   biased     9.98e-07  1e-05    2x150x230    issue (1e-5 x scale)
  heads, two GEMMs, against the oracle                 bf16   fullscale  1.11e-06  1e-05    2x150x230    issue (1e-5 x scale)
  heads, two GEMMs, against the oracle                 fp16   biased     1.17e-06  1e-05    2x150x230    issue (1e-5 x scale)
  heads, two GEMMs, against the oracle                 fp16   fullscale  1.11e-06  1e-05    2x150x230    issue (1e-5 x scale)
  lstm_o                                               fp32   biased     4.8e-07   5e-06    2x70x100     existing (fp32 walk)
  lstm_o                                               fp32   fullscale  2.56e-07  5e-06    2x70x100     existing (fp32 walk)
  lstm_o                                               split  biased     6.4e-07   5e-06    1x600x900    existing (fp32 walk)
  lstm_o                                               split  fullscale  2.27e-07  5e-06    2x70x100     existing (fp32 walk)
  lstm_out, end to end                                 split  biased     5.98e-05  0.0001   1x600x900    issue (1e-4)
  lstm_out, exact                                      fp32   biased     4.77e-07  5e-06    1x600x900    existing
  lstm_out, exact                                      fp32   fullscale  2.32e-06  5e-06    9x240x512    existing
  lstm_out, exact_fast_gates                           bf16   biased     5.07e-07  2e-05    1x600x900    existing
  lstm_out, exact_fast_gates                           bf16   fullscale  2.18e-06  2e-05    9x240x512    existing
  lstm_out, split_16                                   split  biased     5.42e-06  3e-05    9x240x512    existing (recurrence)
  lstm_out, split_16                                   split  fullscale  4.04e-06  3e-05    9x240x512    existing (recurrence)
  lstm_out, split_16                                   bf16   biased     5.62e-06  3e-05    9x240x512    existing (recurrence)
  lstm_out, split_16                                   bf16   fullscale  3.61e-06  3e-05    9x240x512    existing (recurrence)
  lstm_out, split_16                                   fp16   biased     5.2e-06   3e-05    9x240x512    existing (recurrence)
  lstm_out, split_16                                   fp16   fullscale  3.41e-06  3e-05    9x240x512    existing (recurrence)
  lstm_out, split_few                                  split  biased     6.65e-06  3e-05    1x600x900    existing (recurrence)
  lstm_out, split_few                                  split  fullscale  3.46e-06  3e-05    1x600x900    existing (recurrence)
  lstm_out, split_few                                  bf16   biased     7.44e-06  3e-05    1x600x900    existing (recurrence)
  lstm_out, split_few                                  bf16   fullscale  3.73e-06  3e-05    1x600x900    existing (recurrence)
  lstm_out, split_few                                  fp16   biased     6.74e-06  3e-05    1x600x900    existing (recurrence)
  lstm_out, split_few                                  fp16   fullscale  5.6e-06   3e-05    1x600x900    existing (recurrence)
  lstm_pre, igemm                                      fp32   biased     6.13e-07  5e-06    2x96x1000    existing (layer walks)
  lstm_pre, igemm                                      fp32   fullscale  9.2e-07   5e-06    2x70x100     existing (layer walks)
  lstm_pre, igemm                                      split  biased     4.17e-06  1.2e-05  1x600x900    existing (layer walks)
  lstm_pre, igemm                                      split  fullscale  5.91e-06  1.2e-05  1x600x900    existing (layer walks)
  lstm_pre, lds                                        bf16   biased     0.0012    0.008    9x240x512    existing (layer walks)
  lstm_pre, lds                                        bf16   fullscale  0.00171   0.008    9x240x512    existing (layer walks)
  lstm_pre, lds                                        fp16   biased     0.000406  0.0015   9x240x512    existing (layer walks)
  lstm_pre, lds                                        fp16   fullscale  0.000451  0.0015   9x240x512    existing (layer walks)
  lstm_pre, small                                      bf16   biased     0.00124   0.008    1x600x900    existing (layer walks)
  lstm_pre, small                                      bf16   fullscale  0.00176   0.008    2x96x1000    existing (layer walks)
  lstm_pre, small                                      fp16   biased     0.000409  0.0015   2x96x1000    existing (layer walks)
  lstm_pre, small                                      fp16   fullscale  0.000498  0.0015   3x17x33      existing (layer walks)
"""
import os
import re

import numpy as np
import pytest

import ctpn_amd
from oracle import conv1_q as Q
from oracle import network as N
from oracle import postproc as P
from oracle.rounding import bf16_round, fp16_round
from util import match_lines, stress_arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["biased", "fullscale"]
SMALL = (2, 70, 100)

# conv and lstm_pre against the oracle op on the device's input, max |diff| over the map's max: test_fp32_every_layer_matches_oracle (5e-6),
# test_every_layer_matches_oracle (split 1.2e-5, fp16 1.5e-3), _layerwise_bf16 (8e-3)
TOL = {"fp32": 5e-6, "split": 1.2e-5, "fp16": 1.5e-3, "bf16": 8e-3}
# the recurrence on the device's own lstm_pre, max |diff| of outputs bounded by 1 (test_recurrent_kernels_on_device_pre_activations_at_
# benchmark_geometry): exact-fp32 MFMA with library gates 5e-6, with v_exp / v_rcp gates 2e-5, split-bf16 product with those gates 3e-5
REC_TOL = {"exact": 5e-6, "fast": 2e-5, "split": 3e-5}
# the FC GEMMs (fp32 operands in every mode) against N.dense of the device's input: test_fp32_every_layer_matches_oracle's lstm_o bound
FC_TOL = 5e-6
# launch_bilstm (csrc/bilstm.hip): the split-bf16 recurrence takes its four-rows-per-workgroup form up to this many rows (n x hf)
FEW_ROWS_MAX = 128


def lstm_pre_form(prec, cells):
    """Which kernel computes lstm_pre: fp32 and split precision the im2col GEMM (bias in its epilogue); the 16-bit modes launch_lstm_pre
    (csrc/lstm_pre.hip), whose one-wave form reads the bias from global memory and whose resident-slice form reads it from LDS."""
    if prec in ("fp32", "split"):
        return "igemm"
    from ctpn_amd import _binding as B
    return B.lstm_pre_plan(cells, cu_count=0).form      # the plan launch_lstm_pre follows, on this device


def recurrent_form(prec, lstm_split, rows):
    """Which kernel launch_bilstm picks, and the bound of REC_TOL that goes with it."""
    if prec == "fp32" or not lstm_split:
        return ("exact", "exact") if prec in ("fp32", "split") else ("exact_fast_gates", "fast")
    return ("split_few" if rows <= FEW_ROWS_MAX else "split_16", "split")


@pytest.fixture(autouse=True)
def _options_come_from_the_tests_only(monkeypatch):
    from ctpn_amd import _binding as B
    for var in B.OPTION_ENV.values():                      # the binding maps these onto every Context; other modules set some of them
        monkeypatch.delenv(var, raising=False)


@pytest.fixture(scope="module")
def arenas():
    out = {}
    for kind in KINDS:
        a = stress_arena(kind)
        out[kind] = (a, ctpn_amd.arena_views(a))
    return out


_forward_cache = {}


def oracle_forward(arenas, kind, shape, seed):
    key = (kind, shape, seed)
    if key not in _forward_cache:
        _forward_cache[key] = N.forward(ctpn_amd.weights.synthetic_images(*shape, seed), arenas[kind][1], keep={"lstm_out"})
    return _forward_cache[key]


def fig(what, mode, kind, shape, measured, bound):
    """One line per figure, printed BEFORE the assertion that uses it (pytest -s shows them; the table above was collected from them)."""
    print("FIG | %s | %s | %s | %s | %.3g | %.3g" % (what, mode, kind, "x".join(map(str, shape)), measured, bound))
    return measured


def rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(float(np.abs(want).max()), 1e-30))


def ctx_for(arena, shape, prec, **options):
    n, h, w = shape
    ctx = ctpn_amd.Context(0, n, h, w, prec, options=options)
    ctx.load_weights(arena)
    return ctx


# ---------------------------------------------------------------------------------------------------------------
# a. layer walk
# ---------------------------------------------------------------------------------------------------------------
def walk(ctx, imgs, w, prec, kind):
    shape = imgs.shape[:3]
    tol = TOL[prec]
    ctx.forward(imgs)
    prev = N.image_blob(imgs)
    worst = 0.0
    for name in N.CONVS:
        dev = ctx.get_tensor(name)
        iso = N.conv3x3_relu(prev, w[name + "/weights"], w[name + "/biases"])
        scale = max(float(np.abs(iso).max()), 1e-30)
        diff = np.abs(dev - iso)
        worst = max(worst, float(diff.max()) / scale)
        assert np.isfinite(dev).all(), name
        assert float(diff.max()) / scale < tol, (name, float(diff.max()) / scale)
        # a wrong pixel row / tile is a LOCAL error: no pixel off by more than 4 x tol of the map's range
        bad = diff.max(axis=-1) > 4 * tol * scale
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        prev = dev
        del iso, diff
        if name in N.POOL_AFTER:
            p = ctx.get_tensor(N.POOL_AFTER[name])
            assert np.array_equal(p, N.maxpool2x2(dev)), N.POOL_AFTER[name]
            prev = p
    fig("conv (worst of 14)", prec, kind, shape, worst, tol)
    pre = ctx.get_tensor("lstm_pre")
    assert fig("lstm_pre, " + lstm_pre_form(prec, pre.size // 1024), prec, kind, shape, rel(pre, N.lstm_pre(prev, w)), tol) < tol
    lo = ctx.get_tensor("lstm_out")
    form, cls = recurrent_form(prec, ctx.get_option("lstm_split"), shape[0] * (shape[1] // 16))
    assert np.isfinite(lo).all() and np.abs(lo).max() <= 1.0
    assert fig("lstm_out, " + form, prec, kind, shape, float(np.abs(lo - N.bilstm_from_pre(pre, w)).max()), REC_TOL[cls]) < REC_TOL[cls]
    if prec in ("fp32", "split"):
        fc = ctx.get_tensor("lstm_o")
        assert fig("lstm_o", prec, kind, shape, rel(fc, N.dense(lo, w["lstm_o/weights"], w["lstm_o/biases"])), FC_TOL) < FC_TOL
        heads = ctx.get_tensor("heads")
        want = np.concatenate([N.dense(fc, w["rpn_bbox_pred/weights"], w["rpn_bbox_pred/biases"]),
                               N.dense(fc, w["rpn_cls_score/weights"], w["rpn_cls_score/biases"])], axis=-1)
        e_box, e_cls = rel(heads[..., :40], want[..., :40]), rel(heads[..., 40:], want[..., 40:])
        fig("heads (bbox 40, cls 20)", prec, kind, shape, max(e_box, e_cls), FC_TOL)
        assert e_box < FC_TOL and e_cls < FC_TOL, (e_box, e_cls)
    return lo


PRODUCTION_TENSORS = ("pool1", "pool2", "pool3", "pool4", "conv5_3", "rpn_conv/3x3", "lstm_out")


def production_equals_keep_acts(arena, imgs, prec, kept):
    """Without keep_acts (fused pools, conv1_1 inside conv1_2, folded heads in the 16-bit modes): the same bytes up to lstm_out."""
    with ctx_for(arena, imgs.shape[:3], prec) as ctx:
        ctx.forward(imgs)
        for k in PRODUCTION_TENSORS:
            assert np.array_equal(ctx.get_tensor(k), kept[k]), k
        heads = ctx.get_tensor("heads")
    assert np.abs(heads - kept["heads"]).max() < 2e-5 * max(1.0, float(np.abs(kept["heads"]).max()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("prec", ["fp32", "split", "bf16", "fp16"])
def test_every_layer_with_biases_and_at_full_scale(arenas, prec, kind):
    arena, w = arenas[kind]
    imgs = ctpn_amd.weights.synthetic_images(*SMALL, 101)
    with ctx_for(arena, SMALL, prec, keep_acts=1) as ctx:
        walk(ctx, imgs, w, prec, kind)
        kept = {k: ctx.get_tensor(k) for k in PRODUCTION_TENSORS + ("heads",)}
    production_equals_keep_acts(arena, imgs, prec, kept)


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_every_layer_with_biases_at_600x900(arenas, prec):
    """The benchmark geometry (persistent conv kernels, ragged edge columns, 37 x 56 feature map) on "biased". split precision: also one
    fixed END-TO-END bound against the fp32 oracle forward with the default lstm_split = 1 -- cls_prob < 2e-4 (the figure the mode delivers
    on the benchmark arena, test_config5_geometry_end_to_end_against_the_oracle) and lstm_out < 1e-4."""
    shape = (1, 600, 900)
    arena, w = arenas["biased"]
    imgs = ctpn_amd.weights.synthetic_images(*shape, 101)
    with ctx_for(arena, shape, prec, keep_acts=1) as ctx:
        lo = walk(ctx, imgs, w, prec, "biased")
        kept = {k: ctx.get_tensor(k) for k in PRODUCTION_TENSORS + ("heads",)}
        if prec == "split":
            assert ctx.get_option("lstm_split") == 1
            ctx.proposals(np.array([[600, 900, 1.0]], np.float32))
            cp = ctx.get_tensor("rpn_cls_prob_reshape")
            ref = oracle_forward(arenas, "biased", shape, 101)
            d_lo = fig("lstm_out, end to end", prec, "biased", shape, float(np.abs(lo - ref["lstm_out"]).max()), 1e-4)
            d_cls = fig("cls_prob, end to end", prec, "biased", shape, float(np.abs(cp - ref["rpn_cls_prob_reshape"]).max()), 2e-4)
            assert d_lo < 1e-4 and d_cls < 2e-4, (d_lo, d_cls)
    production_equals_keep_acts(arena, imgs, prec, kept)


# ---------------------------------------------------------------------------------------------------------------
# b. conv1_1 with a bias, every form
# ---------------------------------------------------------------------------------------------------------------
CONV1_SHAPES = [(2, 72, 104), (1, 16, 19), (1, 37, 53)]
shape_id = lambda s: "x".join(map(str, s))      # noqa: E731


def border_of(a):
    m = np.ones(a.shape[1:3], bool)
    m[1:-1, 1:-1] = False
    return m


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CONV1_SHAPES, ids=shape_id)
def test_conv1_1_bias_fp32_direct_kernel_both_feeds(arenas, shape, kind):
    """conv_first_kernel: the accumulator starts from bias[]. uint8 feed and float blob feed, interior and border pixels."""
    arena, w = arenas[kind]
    imgs = ctpn_amd.weights.synthetic_images(*shape, 77)
    want = N.conv3x3_relu(N.image_blob(imgs), w["conv1_1/weights"], w["conv1_1/biases"])
    with ctx_for(arena, shape, "fp32", keep_acts=1) as ctx:
        ctx.forward(imgs)
        a = ctx.get_tensor("conv1_1")
        ctx.forward_blob(N.image_blob(imgs))
        b = ctx.get_tensor("conv1_1")
    assert np.array_equal(a, b)
    scale = float(np.abs(want).max())
    err = np.abs(a - want)
    fig("conv1_1, conv_first_kernel", "fp32", kind, shape, float(err.max()) / scale, TOL["fp32"])
    assert err.max() < TOL["fp32"] * scale
    assert err[:, border_of(err)].max() < TOL["fp32"] * scale


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CONV1_SHAPES, ids=shape_id)
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_conv1_1_bias_q_image_form(arenas, prec, shape, kind):
    """conv1_kernel = 2: V = bias + G[1][1] + ... as a (hi, lo) pair on the centre pixel's P slot. The assertions of
    test_q_image_conv1_1_against_the_oracle_layer (the oracle layer on 16-bit-rounded weights: one rounding of the output type, border
    pixels separately) and of test_device_conv1_1_equals_its_arithmetic_specification (oracle/conv1_q.py, value for value)."""
    arena, w = arenas[kind]
    imgs = ctpn_amd.weights.synthetic_images(*shape, 5)
    with ctx_for(arena, shape, prec, keep_acts=1, conv1_kernel=2) as ctx:
        ctx.forward(imgs)
        got = ctx.get_tensor("conv1_1")
    rnd = bf16_round if prec == "bf16" else fp16_round
    want = N.conv3x3_relu(N.image_blob(imgs), rnd(w["conv1_1/weights"]), w["conv1_1/biases"])
    assert got.shape == want.shape
    ulp = float(np.abs(want).max()) * (2.0 ** -8 if prec == "bf16" else 2.0 ** -11)
    err = np.abs(got - want)
    fig("conv1_1, q-image, in output ulps", prec, kind, shape, float(err.max()) / ulp, 1.0)
    assert err.max() <= ulp, err.max() / ulp
    assert err[:, border_of(err)].max() <= ulp
    spec = Q.conv1_1_from_q(imgs, w["conv1_1/weights"], w["conv1_1/biases"], prec)
    ulp = float(np.abs(spec).max()) * (2.0 ** -8 if prec == "bf16" else 2.0 ** -11)
    fig("conv1_1, q-image, share != specification", prec, kind, shape, float((got != spec).mean()), 2e-3)
    assert (got != spec).mean() < 2e-3, (got != spec).mean()
    assert np.abs(got - spec).max() <= ulp


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CONV1_SHAPES, ids=shape_id)
def test_conv1_1_bias_mfma_hi_lo_form_equals_the_direct_kernel(arenas, shape, kind):
    """conv1_kernel = 1 (the bias is a weight row in slot 9 of ky 0, times a constant-1.0 data slot) against conv1_kernel = 0 (VALU kernel,
    accumulator initialised from the bias) in bf16 mode: the assertions of test_conv1_mfma_split_bf16_equals_fp32_direct_kernel."""
    arena, w = arenas[kind]
    imgs = ctpn_amd.weights.synthetic_images(*shape, 77)
    got = {}
    for kernel in (1, 0):
        with ctx_for(arena, shape, "bf16", keep_acts=1, conv1_kernel=kernel) as ctx:
            ctx.forward(imgs)
            got[kernel, "u8"] = ctx.get_tensor("conv1_1")
            ctx.forward_blob(N.image_blob(imgs))
            got[kernel, "f32"] = ctx.get_tensor("conv1_1")
    exact = N.conv3x3_relu(N.image_blob(imgs), w["conv1_1/weights"], w["conv1_1/biases"])
    for feed in ("u8", "f32"):
        a, b = got[1, feed], got[0, feed]
        assert a.shape == b.shape == exact.shape
        flips = a != b
        fig("conv1_1, MFMA hi+lo, share != direct kernel (%s)" % feed, "bf16", kind, shape, float(flips.mean()), 2e-3)
        assert flips.mean() < 2e-3, (feed, flips.mean())
        assert np.abs(a - b).max() <= np.abs(exact).max() * 2.0 ** -7
        assert np.abs(a - exact).max() <= np.abs(b - exact).max() * 1.02 + 1e-6
        assert rel(b, exact) < TOL["bf16"] and rel(a, exact) < TOL["bf16"]
        bd = border_of(exact)
        assert np.abs(a - exact)[:, bd].max() <= np.abs(exact).max() * 2.0 ** -8
    assert np.array_equal(got[1, "u8"], got[1, "f32"])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("geom", [(2, 600, 900), (3, 101, 203), (1, 16, 16)], ids=shape_id)
def test_fused_conv1_gives_the_stored_forms_bytes_at_full_scale(arenas, prec, geom):
    """test_fused_conv1_gives_the_stored_forms_bytes on "fullscale": conv1_1 computed inside conv1_2's window stage, V pair included."""
    arena = arenas["fullscale"][0]
    imgs = ctpn_amd.weights.synthetic_images(*geom, 7 + geom[1])
    out = {}
    for fuse in (1, 0):
        with ctx_for(arena, geom, prec, conv1_fuse=fuse) as ctx:
            for rep in range(2 if fuse else 1):
                ctx.forward(imgs)
                out[fuse, rep] = {t: ctx.get_tensor(t).copy() for t in ("pool1", "heads")}
    for t in ("pool1", "heads"):
        assert np.isfinite(out[1, 0][t]).all()
        assert np.array_equal(out[1, 0][t], out[1, 1][t]), t + ": the second fused forward differs from the first"
        d = np.flatnonzero(out[1, 0][t].ravel() != out[0, 0][t].ravel())
        assert d.size == 0, "%s: %d of %d values differ between the fused and the stored form" % (t, d.size, out[1, 0][t].size)


# ---------------------------------------------------------------------------------------------------------------
# c. folded heads
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_folded_heads_with_biases(arenas, prec, kind):
    """b' = b_fc W_h + b_h (folded in double at pack time, one fp32 GEMM) against the two fp32 GEMMs of keep_acts = 1, and both against
    the oracle's two dense layers on the device's own lstm_out. On the benchmark arena both forms add zero."""
    shape = (2, 150, 230)
    arena, w = arenas[kind]
    imgs = ctpn_amd.weights.synthetic_images(*shape, 5)
    heads, lo = {}, {}
    for keep in (1, 0):
        with ctx_for(arena, shape, prec, keep_acts=keep) as ctx:
            ctx.forward(imgs)
            heads[keep], lo[keep] = ctx.get_tensor("heads"), ctx.get_tensor("lstm_out")
            if not keep:
                with pytest.raises(ctpn_amd.CtpnError):
                    ctx.get_tensor("lstm_o")
    assert np.array_equal(lo[0], lo[1])
    fc = N.dense(lo[1], w["lstm_o/weights"], w["lstm_o/biases"])
    want = np.concatenate([N.dense(fc, w["rpn_bbox_pred/weights"], w["rpn_bbox_pred/biases"]),
                           N.dense(fc, w["rpn_cls_score/weights"], w["rpn_cls_score/biases"])], axis=-1)
    scale = max(1.0, float(np.abs(want).max()))
    fig("heads, folded against two GEMMs", prec, kind, shape, float(np.abs(heads[1] - heads[0]).max()) / scale, 2e-5)
    assert np.abs(heads[1] - heads[0]).max() < 2e-5 * max(1.0, float(np.abs(heads[1]).max()))
    for keep in (1, 0):
        e = fig("heads, %s, against the oracle" % ("two GEMMs" if keep else "folded"), prec, kind, shape, float(np.abs(heads[keep] - want).max()) / scale, 1e-5)
        assert e < 1e-5, (keep, e)


# ---------------------------------------------------------------------------------------------------------------
# d. recurrence variants at the time-axis and row edges
# ---------------------------------------------------------------------------------------------------------------
# rows = n x (h // 16), T = w // 16: 3 x 2, 12 x 1, 3 x 8, 12 x 62, 37 x 56 -- and 135 x 32: past FEW_ROWS_MAX, the 16-row split form, and
# with 4320 cells past half a round of workgroups on 256 CUs, where launch_lstm_pre leaves its one-wave form for the LDS-bias form
REC_SHAPES = [(3, 17, 33), (1, 200, 31), (1, 48, 130), (2, 96, 1000), (1, 600, 900), (9, 240, 512)]
REC_MODES = [("fp32", 0), ("bf16", 0), ("bf16", 1), ("fp16", 1), ("split", 1)]


def test_recurrence_shapes_reach_every_form():
    src = open(os.path.join(ROOT, "text-detection-ctpn_amd", "csrc", "bilstm.hip")).read()
    assert re.search(r"if \(split_bf16 && rows <= %d\)" % FEW_ROWS_MAX, src), "launch_bilstm's selection rule changed: update FEW_ROWS_MAX"
    forms = {recurrent_form(p, s, sh[0] * (sh[1] // 16))[0] for p, s in REC_MODES for sh in REC_SHAPES}
    assert forms == {"exact", "exact_fast_gates", "split_few", "split_16"}
    for p, s in REC_MODES:
        if s:
            assert {recurrent_form(p, s, sh[0] * (sh[1] // 16))[0] for sh in REC_SHAPES} == {"split_few", "split_16"}, p
    for p in ("bf16", "fp16"):      # (lstm_pre_form asks the library's plan: no copy of launch_lstm_pre's rule here that could drift)
        assert {lstm_pre_form(p, sh[0] * (sh[1] // 16) * (sh[2] // 16)) for sh in REC_SHAPES} == {"small", "lds"}, p


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_both_split_forms_of_the_recurrence_give_one_rows_bits(arenas, prec):
    """bilstm_split_kernel and bilstm_split_few_kernel call one copy of the Wh fragment build, the h reads and the 48 MFMAs (csrc/bilstm.hip):
    every image's lstm_out in a batch of nine (135 rows, T = 4: the 16-row form, last workgroup ragged) equals the bits of that image forwarded
    alone (15 rows: the four-row form, last workgroup ragged), with fp16 pre-activations (bf16) and fp32 ones (split precision). lstm_out of a
    whole forward also needs every layer in front of the recurrence to give a batch the bits of its images alone (the conv dispatch, lstm_pre's
    forms); test_recurrence_on_the_devices_own_pre_activations holds each form of the recurrence to the oracle on the device's own lstm_pre."""
    n, h, wd = shape = (9, 240, 64)
    assert recurrent_form(prec, 1, n * (h // 16))[0] == "split_16" and recurrent_form(prec, 1, h // 16)[0] == "split_few"
    arena = arenas["biased"][0]
    imgs = ctpn_amd.weights.synthetic_images(n, h, wd, 29)
    with ctx_for(arena, shape, prec, keep_acts=1) as ctx:
        assert ctx.get_option("lstm_split") == 1
        ctx.forward(imgs)
        batch = ctx.get_tensor("lstm_out")
    assert batch.shape == (n, h // 16, wd // 16, 256) and np.isfinite(batch).all() and np.abs(batch).max() > 0
    with ctx_for(arena, (1, h, wd), prec, keep_acts=1) as ctx:
        for i in range(n):
            ctx.forward(imgs[i:i + 1])
            assert np.array_equal(ctx.get_tensor("lstm_out")[0], batch[i]), i


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", REC_SHAPES, ids=shape_id)
@pytest.mark.parametrize("prec,lstm_split", REC_MODES)
def test_recurrence_on_the_devices_own_pre_activations(arenas, prec, lstm_split, shape, kind):
    arena, w = arenas[kind]
    n, h, wd = shape
    imgs = ctpn_amd.weights.synthetic_images(n, h, wd, 23)
    with ctx_for(arena, shape, prec, keep_acts=1, lstm_split=lstm_split) as ctx:
        assert ctx.get_option("lstm_split") == lstm_split
        ctx.forward(imgs)
        x, pre, out = ctx.get_tensor("rpn_conv/3x3"), ctx.get_tensor("lstm_pre"), ctx.get_tensor("lstm_out")
    assert pre.shape == (n, h // 16, wd // 16, 1024) and out.shape == (n, h // 16, wd // 16, 256)
    form, cls = recurrent_form(prec, lstm_split, n * (h // 16))
    assert np.isfinite(pre).all()
    e_pre = fig("lstm_pre, " + lstm_pre_form(prec, n * (h // 16) * (wd // 16)), prec, kind, shape, rel(pre, N.lstm_pre(x, w)), TOL[prec])
    assert e_pre < TOL[prec], e_pre
    assert np.isfinite(out).all()
    assert np.abs(out).max() <= 1
    want = N.bilstm_from_pre(pre, w)
    err = fig("lstm_out, " + form, prec, kind, shape, float(np.abs(out - want).max()), REC_TOL[cls])
    print("      max |lstm_pre| %.1f, |lstm_out| > 0.99: %.1f %%" % (float(np.abs(pre).max()), 100.0 * float((np.abs(want) > 0.99).mean())))
    assert err < REC_TOL[cls], (form, err)


# ---------------------------------------------------------------------------------------------------------------
# e. saturated scores through the proposal layer
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [{"nms_prefix": 1}, {"nms_prefix": 0}, {"nms_columns": 0}], ids=["prefix", "full_pass", "generic"])
@pytest.mark.parametrize("prec", ["fp32", "split"])
def test_saturated_scores_through_the_proposal_layer(arenas, prec, options):
    """"fullscale", 1 x 600 x 900: cls_prob holds exact 1.0f (ties by the thousand) and values down to 1e-13 next to KEY_INVALID's order.
    The small-batch column forms with and without the 4096-candidate prefix pass, and the generic kernels (nms_columns = 0)."""
    shape = (1, 600, 900)
    arena, w = arenas["fullscale"]
    imgs = ctpn_amd.weights.synthetic_images(*shape, 101)
    info = np.array([[600, 900, 1.0]], np.float32)
    with ctx_for(arena, shape, prec, **options) as ctx:
        ctx.forward(imgs)
        rois, anchors = ctx.proposals(info, want_anchors=True)
        rois, anchors = rois[0], anchors[0]
        cp, bp = ctx.get_tensor("rpn_cls_prob_reshape"), ctx.get_tensor("rpn_bbox_pred")
        lines = {}
        for mode in "HO":
            lines[mode], r2 = ctx.detect(imgs, mode=mode, want_rois=True)
            assert np.array_equal(r2[0], rois), mode
    assert np.isfinite(cp).all() and np.isfinite(bp).all()
    ones = int((cp == np.float32(1.0)).sum())
    print("      cls_prob == 1.0f: %d of %d, min %.3g, exact zeros %d" % (ones, cp.size, float(cp.min()), int((cp == 0).sum())))
    assert ones > 0
    want = P.proposal_layer(cp, bp, info[0])
    assert rois.shape == want.shape
    assert np.array_equal(rois[:, 0], want[:, 0])
    assert np.abs(rois[:, 1:] - want[:, 1:]).max() < 1e-3
    # the documented tie order: descending score, then ascending anchor index
    assert np.all(np.diff(rois[:, 0]) <= 0)
    tied = np.diff(rois[:, 0]) == 0
    assert tied.any() and np.all(np.diff(anchors)[tied] > 0)
    for mode in "HO":
        assert match_lines(lines[mode][0], P.text_detect(want[:, 1:5], want[:, 0], (600, 900), mode), 1.0, 1e-3), mode
    if prec == "fp32":
        ref = oracle_forward(arenas, "fullscale", shape, 101)
        d_cls = fig("cls_prob, end to end", prec, "fullscale", shape, float(np.abs(cp - ref["rpn_cls_prob_reshape"]).max()), 1e-3)
        d_box = fig("bbox_pred, end to end", prec, "fullscale", shape, float(np.abs(bp - ref["rpn_bbox_pred"]).max()), 1e-3)
        assert d_cls < 1e-3 and d_box < 1e-3


# ---------------------------------------------------------------------------------------------------------------
# f. batch invariance
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_batch_equals_singles_and_is_idempotent_at_full_scale(arenas, prec):
    n = 4
    arena = arenas["fullscale"][0]
    imgs = ctpn_amd.weights.synthetic_images(n, 600, 900, 1)
    with ctx_for(arena, (n, 600, 900), prec) as ctx:
        l1, r1 = ctx.detect(imgs, want_rois=True)
        l2, r2 = ctx.detect(imgs, want_rois=True)
        for i in range(n):
            assert np.array_equal(r1[i], r2[i]) and np.array_equal(l1[i], l2[i]), i
        for i in (0, n - 1):
            ls, rs = ctx.detect(imgs[i:i + 1], want_rois=True)
            assert np.array_equal(rs[0], r1[i]) and np.array_equal(ls[0], l1[i]), i
    for r in r1:
        assert 0 < r.shape[0] <= 1000 and np.isfinite(r).all() and np.all(np.diff(r[:, 0]) <= 0)
