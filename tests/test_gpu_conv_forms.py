"""GPU (-m gpu): every conv3x3 kernel form in every precision at the smallest shape that reaches it, against the float64 oracle.

One case per CELL of tests/conv_form_cases.py (445 of the network, 125 that only the debug entry reaches; tests/conv_forms.py says what a
cell is and how the table is made, tests/test_conv_forms.py keeps it complete). A case runs ctpn_debug_conv3x3 in the cell's precision on
ReLU'd normal input and He-scaled weights with a non-zero bias. Input and weights are rounded to the mode's operand type first (bf16, fp16,
the (hi, lo) bf16 pair of split precision), so what is measured is accumulation and the rounding of the stored output only. The reference
is oracle/network.py's conv (+ the VALID pool) evaluated in float64 on those operands.

Bounds, as max |diff| over the map's max |value| (the project's per-mode bounds of tests/test_gpu_parity.py and tests/test_gpu_precision.py):
    fp32 5e-6   summation order of at most K = 4608 exact-fp32 products
    split 2e-5  2^-16 per operand pair plus the dropped lo x lo term, (hi, lo) rounding of the output (2^-17)
    fp16 1.5e-3 output rounding 2^-11 = 4.9e-4 of a value, up to the map's max
    bf16 8e-3   output rounding 2^-8 = 3.9e-3 of a value
No cell needs a bound of its own. Measured per cell on an MI355X: profiles/conv_form_cells.txt (worst of map, strip
columns and the column to their left: fp32 1.9e-6, split 8.1e-6, fp16 4.3e-4, bf16 3.9e-3 -- the 16-bit modes sit at one output rounding).

The second half walks the whole network layer by layer (the walk of tests/test_gpu_precision.py::test_every_layer_matches_oracle) at the
geometries of conv_forms.WALKS (the four given ones and the census's width for a one-column edge strip at Ci = 256), where the network itself crosses the strips, the forked and deep edge kernels at Ci = 256 / 512, the
non-flat conv5_x / rpn_conv with an edge strip and, in split precision, rpn_conv's [hi | lo | hi] store from the edge kernel."""
import functools

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
from oracle import network as N
from oracle.rounding import bf16_round, fp16_round
import conv_forms as F
from conv_form_cases import CASES, DEBUG_ONLY_CASES

pytestmark = pytest.mark.gpu

BOUND = {"fp32": 5e-6, "split": 2e-5, "fp16": 1.5e-3, "bf16": 8e-3}


def _operand(prec, a):
    """fp32 array -> the values the mode's kernels actually multiply"""
    if prec == "bf16":
        return bf16_round(a)
    if prec == "fp16":
        return fp16_round(a)
    if prec == "split":
        hi = bf16_round(a)
        return hi + bf16_round(a - hi)          # exact in fp32: the pair spans at most 17 mantissa bits
    return a


@functools.lru_cache(maxsize=4)
def _problem(prec, n, h, w, ci, co):
    """(x, weights, bias, float64 reference of the full map, of the pooled map) -- shared by the cells of one shape, never modified"""
    rng = np.random.default_rng(((n * 131 + h) * 2053 + w) * 17 + ci + co)
    x = _operand(prec, np.maximum(rng.standard_normal((n, h, w, ci)).astype(np.float32), 0) * 3.0)
    wt = _operand(prec, (rng.standard_normal((3, 3, ci, co)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32))
    b = (rng.standard_normal(co) * 0.1).astype(np.float32)
    want = N.conv3x3_relu(x.astype(np.float64), wt.astype(np.float64), b.astype(np.float64))
    want_pool = N.maxpool2x2(want) if h >= 2 and w >= 2 else np.zeros((n, h // 2, w // 2, co))      # (a one-row map has no pooled pixel)
    assert want.dtype == np.float64 and want_pool.dtype == np.float64
    for a in (x, wt, b, want, want_pool):
        a.setflags(write=False)
    return x, wt, b, want, want_pool


def _err(got, ref):
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def _judge(cell, what, got, ref, tol, strip_cols):
    """whole map within tol of the map's max, no pixel beyond 4 x tol, and the strip's columns and the column to their left on their own"""
    assert got.shape == ref.shape, (cell, what, got.shape, ref.shape)
    e = _err(got, ref)
    assert e < tol, (cell, what, e)
    bad = np.abs(got - ref).max(axis=-1) > 4 * tol * max(float(np.abs(ref).max()), 1e-30)
    assert not bad.any(), (cell, what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    es = el = 0.0
    if strip_cols:
        w = ref.shape[2]
        es = _err(got[:, :, w - strip_cols:], ref[:, :, w - strip_cols:])
        el = _err(got[:, :, w - strip_cols - 1:w - strip_cols], ref[:, :, w - strip_cols - 1:w - strip_cols])
        assert es < tol and el < tol, (cell, what, "strip columns %g, the column to their left %g" % (es, el))
    return e, es, el


ALL_CASES = sorted({**CASES, **DEBUG_ONLY_CASES}.items(), key=lambda kv: (kv[0].split("/")[0], kv[1][:5], kv[0]))      # neighbours share a problem


@pytest.mark.parametrize("cell,case", ALL_CASES, ids=[c.replace("/", ".") for c, _ in ALL_CASES])
def test_conv_form_cell_matches_float64_oracle(cell, case):
    prec = cell.split("/")[0]
    n, h, w, ci, co, pool, want_full, dup = case
    assert F.case_cell(prec, case, 256) == cell
    here = F.case_cell(prec, case, cu=0)                 # the plan the launch below follows, on this device
    if here != cell:      # same shape, same options: only the CU count differs, and it chooses between exactly two pairs of main forms
        a, b = cell.split("/"), here.split("/")
        assert a[:1] + a[2:] == b[:1] + b[2:] and {a[1], b[1]} in ({"p_flat", "p_flat64"}, {"p_8x32", "p_8x32_half"}), \
            "the plan of %r is %s, the table says %s" % (case, here, cell)
        pytest.skip("%s: its main form is chosen by the CU count (256 in the table); this device takes %s" % (cell, b[1]))
    tol = BOUND[prec]
    x, wt, b, want, want_pool = _problem(prec, n, h, w, ci, co)
    plan = B.conv3x3_plan(prec, n, h, w, ci, co, pool, want_full or not pool, dup, cu_count=0)
    run = functools.partial(B.debug_conv3x3, x, wt, b, precision=prec, impl=1)
    if not pool:
        full, _ = run(fuse_pool=False, dup_hi=bool(dup))
        errs = _judge(cell, "full map", full, want, tol, plan.cols)
        again, _ = run(fuse_pool=False, dup_hi=bool(dup))
        assert np.array_equal(full.view(np.uint32), again.view(np.uint32)), cell
    else:
        pcols = plan.cols // 2 if plan.strip == "edge_pool" else 0
        full, pooled = run(fuse_pool=True, want_full=True)                   # the kept form of this shape
        assert np.array_equal(pooled, N.maxpool2x2(full)), cell              # the fused pool is the max of what the full-resolution store holds
        if want_full:
            errs = _judge(cell, "full map", full, want, tol, plan.cols)
            _judge(cell, "pooled map", pooled, want_pool, tol, pcols)
            again = run(fuse_pool=True, want_full=True)
            assert np.array_equal(full.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(pooled.view(np.uint32), again[1].view(np.uint32)), cell
        else:
            only = run(fuse_pool=True, want_full=False)[1]                   # the cell: nothing but the pooled map is stored
            errs = _judge(cell, "pooled map", only, want_pool, tol, pcols)
            assert np.array_equal(only.view(np.uint32), pooled.view(np.uint32)), cell      # == the pooled output of the kept form
            again = run(fuse_pool=True, want_full=False)[1]
            assert np.array_equal(only.view(np.uint32), again.view(np.uint32)), cell
    print("CELL %-62s %-34s map %.3e  strip %.3e  left %.3e  of %.1e" % (cell, "x".join(str(v) for v in case[:5]), errs[0], errs[1], errs[2], tol))


# ---------------------------------------------------------------------------------------------------------------
# the whole network, layer by layer, where it crosses the forms above by itself
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights(arena):
    return ctpn_amd.arena_views(arena)


@functools.lru_cache(maxsize=None)
def _oracle_heads(n, h, w):
    imgs = ctpn_amd.weights.synthetic_images(n, h, w, 101)
    full = N.forward(imgs, ctpn_amd.arena_views(ctpn_amd.make_synthetic_arena(0)), keep=set())
    return imgs, full["rpn_cls_prob_reshape"]


def rel_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-30))


# conv / lstm_pre tolerances and the cls_prob bound per mode: split and fp16 as tests/test_gpu_precision.py::test_every_layer_matches_oracle,
# fp32 as tests/test_gpu_parity.py::test_fp32_every_layer_matches_oracle, bf16 as test_gpu_parity's _layerwise_bf16 (cls_prob: smoke()'s bound)
WALK_TOL = {"split": (1.2e-5, 1e-5, 1e-4), "fp16": (1.5e-3, 1.5e-3, 1e-2), "fp32": (5e-6, 5e-6, 1e-4), "bf16": (8e-3, 8e-3, 5e-2)}


@pytest.mark.parametrize("prec", F.PRECS)
@pytest.mark.parametrize("n,h,w", F.WALKS, ids=["%dx%dx%d" % g for g in F.WALKS])
def test_every_layer_matches_oracle_where_the_network_crosses_the_strips(arena, weights, prec, n, h, w):
    conv_tol, pre_tol, cls_tol = WALK_TOL[prec]
    imgs, ref_cls = _oracle_heads(n, h, w)
    with ctpn_amd.Context(0, n, h, w, prec, options={"keep_acts": 1}) as ctx:
        ctx.load_weights(arena)
        ctx.forward(imgs)
        prev = N.image_blob(imgs)
        for name in N.CONVS:
            dev = ctx.get_tensor(name)
            iso = N.conv3x3_relu(prev, weights[name + "/weights"], weights[name + "/biases"])
            assert rel_err(dev, iso) < conv_tol, (name, rel_err(dev, iso))
            prev = dev
            if name in N.POOL_AFTER:
                p = ctx.get_tensor(N.POOL_AFTER[name])
                assert np.array_equal(p, N.maxpool2x2(dev)), N.POOL_AFTER[name]
                prev = p
        pre, want_pre = ctx.get_tensor("lstm_pre"), N.lstm_pre(prev, weights)
        assert rel_err(pre, want_pre) < pre_tol
        if w >> 4 > 96:
            # feature columns 96 (and 97): rpn_conv's edge columns -- in split precision the [hi | lo | hi] pixels the edge kernel stores, whose
            # third plane only this projection reads
            assert pre.shape[2] == w >> 4 and rel_err(pre[:, :, 96:], want_pre[:, :, 96:]) < pre_tol, rel_err(pre[:, :, 96:], want_pre[:, :, 96:])
            assert rel_err(pre[:, :, 95:96], want_pre[:, :, 95:96]) < pre_tol
        info = np.array([[h, w, 1.0]] * n, np.float32)
        ctx.proposals(info)
        heads_keep = ctx.get_tensor("rpn_cls_prob_reshape")
        d = float(np.abs(heads_keep - ref_cls).max())
        print("%s %dx%dx%d: cls_prob max |diff| vs the fp32 oracle %.2e" % (prec, n, h, w, d))
        assert d < cls_tol
    # production path (fused pools, nothing kept) == the keep_acts path
    with ctpn_amd.Context(0, n, h, w, prec) as ctx:
        ctx.load_weights(arena)
        ctx.forward(imgs)
        ctx.proposals(info)
        if prec in ("split", "fp32"):
            assert np.array_equal(heads_keep, ctx.get_tensor("rpn_cls_prob_reshape"))
        else:       # the 16-bit modes fold FC x heads without keep_acts: fp32 rounding apart
            assert np.abs(heads_keep - ctx.get_tensor("rpn_cls_prob_reshape")).max() < 2e-5
