"""GPU: ragged batches -- images of one width and different heights in one call (include/ctpn_hip.h, ctpn_forward_ragged) -- through the C ABI.
The result is DEFINED as what the image gives alone, so everything here is an equality of bits: named tensors cropped to an image's valid
rows, rois, roi counts, anchors, lines and line counts, in all four precisions.

Shapes: w = 82 (W mod 16 = 2: the edge-column kernels) with heights 96, 80, 49, 16, 33 in a canvas of 96, and w = 144 with heights 96 and
49, where the pooled conv2_2 takes the 16 x 16-patch form for the canvas and the 8 x 32 form for the 49-row image alone (asserted
below through the library's plan function). Random bytes below every image. Weights: tests/util.py's "biased" arena, on which every one of these images yields
proposals and text lines (asserted)."""
import ctypes as C

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import ragged_ref as R
import util

pytestmark = pytest.mark.gpu

PRECS = ("fp32", "split", "fp16", "bf16")
SETS = {"w82": (82, (96, 80, 49, 16, 33)), "w144": (144, (96, 49))}
MAPS = ("conv1_1", "conv1_2", "pool1", "conv2_1", "conv2_2", "pool2", "conv3_1", "conv3_2", "conv3_3", "pool3", "conv4_1", "conv4_2", "conv4_3",
        "pool4", "conv5_1", "conv5_2", "conv5_3", "rpn_conv/3x3")
LEVEL = {"conv1_1": 0, "conv1_2": 0, "pool1": 1, "conv2_1": 1, "conv2_2": 1, "pool2": 2, "conv3_1": 2, "conv3_2": 2, "conv3_3": 2, "pool3": 3,
         "conv4_1": 3, "conv4_2": 3, "conv4_3": 3, "pool4": 4, "conv5_1": 4, "conv5_2": 4, "conv5_3": 4, "rpn_conv/3x3": 4}
TAIL = ("lstm_pre", "lstm_out", "lstm_o", "heads", "rpn_cls_prob_reshape", "rpn_bbox_pred")


@pytest.fixture(scope="module")
def weights():
    return util.stress_arena("biased")


@pytest.fixture(scope="module")
def batches():
    """name -> (images, canvas, heights): computed once, never modified"""
    out = {}
    for k, (w, hs) in SETS.items():
        ims = R.images(11, w, hs)
        canvas, heights = R.canvas_of(ims, 96)
        canvas.setflags(write=False)
        out[k] = (ims, canvas, heights)
    return out


def _info(heights, w):
    return np.array([[h, w, 1.0] for h in heights], np.float32)


def _tensors(ctx, names, info):
    rois, anchors = ctx.proposals(info, want_anchors=True)
    return {nm: ctx.get_tensor(nm) for nm in names}, rois, anchors


def test_the_two_heights_of_w144_take_different_conv_forms():
    """the library's own plan (ctpn_debug_conv3x3_plan) of the pooled conv2_2 over the 72-wide map, kept and production form, on this device"""
    for prec in PRECS:
        for keep in (False, True):
            canvas = B.conv3x3_plan(prec, 2, 96 >> 1, 144 >> 1, 128, 128, True, keep)
            alone = B.conv3x3_plan(prec, 1, 49 >> 1, 144 >> 1, 128, 128, True, keep)
            assert canvas.main == "p_16x16" and canvas.strip == "none", (prec, keep, canvas)      # the canvas: 16 x 16 patches
            assert alone.main in ("p_8x32", "p_8x32_half") and alone.strip == "none", (prec, keep, alone)      # the 49-row image alone: 8 x 32


@pytest.mark.parametrize("which", sorted(SETS))
@pytest.mark.parametrize("prec", PRECS)
def test_every_tensor_equals_the_lone_image_bit_for_bit(weights, batches, prec, which):
    ims, canvas, heights = batches[which]
    w = canvas.shape[2]
    with ctpn_amd.Context(0, len(ims), 96, w, prec, options={"keep_acts": 1}) as ctx:
        ctx.load_weights(weights)
        ctx.forward_ragged(canvas, heights)
        assert ctx.feat_shape() == (len(ims), 6, w // 16)
        got, rois, anchors = _tensors(ctx, MAPS + TAIL, _info(heights, w))
        for i, im in enumerate(ims):
            ctx.forward(im[None])
            want, lrois, lanch = _tensors(ctx, MAPS + TAIL, _info(heights[i:i + 1], w))
            for nm in MAPS + TAIL:
                v = heights[i] >> LEVEL.get(nm, 4)
                assert got[nm].shape[1:] == (96 >> LEVEL.get(nm, 4),) + want[nm].shape[2:] and want[nm].shape[1] == v, nm
                assert np.array_equal(got[nm][i, :v].view(np.uint32), want[nm][0].view(np.uint32)), (prec, which, i, nm)
                if nm in MAPS:
                    assert not got[nm][i, v:].any(), (prec, which, i, nm)           # conv and pool maps are zero below an image
            assert len(lrois[0]) > 0
            assert np.array_equal(rois[i], lrois[0]) and np.array_equal(anchors[i], lanch[0]), (prec, which, i)


@pytest.mark.parametrize("prec", PRECS)
def test_detect_equals_the_lone_calls(weights, batches, prec):
    """defaults (nothing kept): ctpn_detect_ragged in modes H and O with the host and the device connector, the proposal layer's anchors, and
    the submit / collect form with two ragged batches in flight"""
    with ctpn_amd.Context(0, 5, 96, 144, prec) as ctx:
        ctx.load_weights(weights)
        lone = {}
        n_lines = 0
        for which, (ims, canvas, heights) in batches.items():
            for i, im in enumerate(ims):
                for cd in (0, 1):
                    ctx.set_option("connect_device", cd)
                    for mode in "HO":
                        lone[which, i, cd, mode] = tuple(x[0] for x in ctx.detect(im[None], mode=mode, want_rois=True))
                        n_lines += len(lone[which, i, cd, mode][0])
                ctx.forward(im[None])
                lone[which, i, "prop"] = tuple(x[0] for x in ctx.proposals(_info(heights[i:i + 1], im.shape[1]), want_anchors=True))
                assert len(lone[which, i, "prop"][0]) > 0                              # every image yields proposals ...
        assert n_lines > 0                                                           # ... and lines come out of them
        for which, (ims, canvas, heights) in batches.items():
            for cd in (0, 1):
                ctx.set_option("connect_device", cd)
                for mode in "HO":
                    lines, rois = ctx.detect_ragged(canvas, heights, mode=mode, want_rois=True)
                    for i in range(len(ims)):
                        assert np.array_equal(rois[i], lone[which, i, cd, mode][1]), (which, i, cd, mode)
                        assert np.array_equal(lines[i], lone[which, i, cd, mode][0]), (which, i, cd, mode)
            ctx.forward_ragged(canvas, heights)
            rois, anchors = ctx.proposals(_info(heights, canvas.shape[2]), want_anchors=True)
            for i in range(len(ims)):
                assert np.array_equal(rois[i], lone[which, i, "prop"][0]) and np.array_equal(anchors[i], lone[which, i, "prop"][1]), (which, i)
        # two slots in flight: the batch, and the same images in another order (other heights per slot)
        ims, canvas, heights = batches["w82"]
        ctx.set_option("connect_device", 0)
        order = [3, 0, 4, 2, 1]
        canvas2, heights2 = np.ascontiguousarray(canvas[order]), np.ascontiguousarray(heights[order])
        ctx.detect_submit(canvas, slot=0, heights=heights)
        ctx.detect_submit(canvas2, slot=1, heights=heights2)
        a = ctx.detect_collect(0, mode="H", want_rois=True)
        b = ctx.detect_collect(1, mode="H", want_rois=True)
        for i in range(5):
            for got, j in ((a, i), (b, order.index(i))):
                assert np.array_equal(got[0][j], lone["w82", i, 0, "H"][0]) and np.array_equal(got[1][j], lone["w82", i, 0, "H"][1]), (i, j)


@pytest.mark.parametrize("prec", PRECS)
def test_equal_heights_are_the_uniform_call_and_a_ctx_forgets(weights, batches, prec):
    """A ragged call whose heights all equal the canvas is the uniform call; a uniform forward after a ragged one, and a ragged one after
    a uniform one, on one ctx, give what a fresh ctx gives."""
    ims, canvas, heights = batches["w82"]
    full = np.full(5, 96, np.int32)
    names = ("rpn_conv/3x3", "heads")
    with ctpn_amd.Context(0, 5, 96, 82, prec) as fresh:
        fresh.load_weights(weights)
        fresh.forward(canvas)
        uni = _tensors(fresh, names, _info(full, 82))
        uni_lines = fresh.detect(canvas, want_rois=True)
    with ctpn_amd.Context(0, 5, 96, 82, prec) as fresh:
        fresh.load_weights(weights)
        fresh.forward_ragged(canvas, heights)
        rag = _tensors(fresh, names, _info(heights, 82))

    def same(x, y):
        return all(np.array_equal(x[0][nm].view(np.uint32), y[0][nm].view(np.uint32)) for nm in names) and \
            all(np.array_equal(p, q) for p, q in zip(x[1], y[1])) and all(np.array_equal(p, q) for p, q in zip(x[2], y[2]))
    with ctpn_amd.Context(0, 5, 96, 82, prec) as ctx:
        ctx.load_weights(weights)
        ctx.forward_ragged(canvas, full)
        assert same(_tensors(ctx, names, _info(full, 82)), uni)
        got = ctx.detect_ragged(canvas, full, want_rois=True)
        assert all(np.array_equal(p, q) for k in (0, 1) for p, q in zip(got[k], uni_lines[k]))
        ctx.forward_ragged(canvas, heights)
        assert same(_tensors(ctx, names, _info(heights, 82)), rag)           # ragged after uniform
        ctx.forward(canvas)
        assert same(_tensors(ctx, names, _info(full, 82)), uni)              # uniform after ragged: the valid rows are forgotten
        assert not same(rag, uni)


def test_errors_and_the_callers_canvas(weights, batches):
    import torch
    ims, canvas, heights = batches["w82"]
    lib = B.load_library()
    i32p = C.POINTER(C.c_int)
    with ctpn_amd.Context(0, 5, 96, 82, "bf16") as ctx:
        def call(n, hc, w, hts):
            hts = None if hts is None else np.asarray(hts, np.int32)
            return lib.ctpn_forward_ragged(ctx._h, canvas.ctypes.data_as(C.c_void_p), 0, n, hc, w, None if hts is None else hts.ctypes.data_as(i32p))
        assert call(5, 96, 82, heights) == -3                                          # no weights yet
        ctx.load_weights(weights)
        assert call(5, 96, 82, None) == -1
        assert call(5, 96, 82, [96, 80, 49, 15, 33]) == -1 and call(5, 96, 82, [97, 80, 49, 16, 33]) == -1
        assert call(6, 96, 82, [96] * 6) == -4 and call(5, 112, 82, heights) == -4
        # a device canvas: the same results, and not a byte of it changed (the rows below the images included)
        dev = torch.from_numpy(np.array(canvas)).cuda()
        a = ctx.detect_ragged(device_ptr=dev.data_ptr(), shape=canvas.shape[:3], heights=heights, want_rois=True)
        b = ctx.detect_ragged(canvas, heights, want_rois=True)
        assert all(np.array_equal(p, q) for k in (0, 1) for p, q in zip(a[k], b[k]))
        assert np.array_equal(dev.cpu().numpy(), canvas)
    with ctpn_amd.Context(0, 5, 96, 82, "fp32", postproc_only=True) as ctx:
        hts = np.asarray(heights, np.int32)
        assert lib.ctpn_forward_ragged(ctx._h, canvas.ctypes.data_as(C.c_void_p), 0, 5, 96, 82, hts.ctypes.data_as(i32p)) == -3


def test_demo_batch_ragged_writes_the_same_result_files(weights, tmp_path):
    """a directory of small PNG files of one width and five heights: res_*.txt byte-equal with and without ragged batches"""
    from PIL import Image
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    src = tmp_path / "in"
    src.mkdir()
    # 100 pixels wide: resize_im enlarges every file six times, to 600 x (720, 690, 600, 624, 660, 720, 600)
    for i, h in enumerate((120, 115, 100, 104, 110, 120, 100)):
        im = ctpn_amd.weights.synthetic_images(1, h, 100, 20 + i)[0]
        Image.fromarray(np.ascontiguousarray(im[:, :, ::-1])).save(src / ("page%d.png" % i))
    names = demo_batch.list_images(str(src))
    assert len(names) == 7
    cfg.TEST.PRECISION = "bf16"
    outs = {}
    for ragged in (False, True):
        net = get_network("VGGnet_test")
        net.load_arena(weights)
        try:
            out = tmp_path / ("out%d" % ragged)
            log = []
            demo_batch.run(net, names, str(out), batch=4, write_images=False, log=log.append, ragged=ragged)
        finally:
            net.close()
        outs[ragged] = {p.name: p.read_bytes() for p in sorted(out.iterdir())}
        # five resized shapes; across heights: 720, 720, 690, 660 | 624, 600, 600
        assert " in %d batches " % (2 if ragged else 5) in log[-1], log
    assert sorted(outs[True]) == ["res_page%d.txt" % i for i in range(7)] and outs[True] == outs[False]
    assert any(len(v) > 0 for v in outs[True].values())
