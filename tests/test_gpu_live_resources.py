"""GPU: everything a ctx or a stateless entry point acquires is released again -- the library's own count (ctpn_debug_live_resources: device
bytes, page-locked bytes, events, streams, kept by the handle types of csrc/owned.h) is back at its starting values after ctpn_destroy and after
every hook that owns temporaries.

A ctx of 2 x 64 x 96 is driven through every path that allocates lazily, each at the smallest input it accepts: forwards (uniform, ragged), two
submits in flight (forward set 1), a ragged submit, the JPEG decoders in both entropy forms with a second, larger batch (a block is retired),
every writer and the crops, uniform and ragged, each a second time at a larger size (every buffer grows), and per-stage profiling. The baseline
is read once at the start of the module: whatever an earlier test of the process left for good (ctpn_nms's cache) is part of it."""
import ctypes as C
import gc

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
from out_ragged_cases import line
from util_jpeg import encode, scene

pytestmark = pytest.mark.gpu

MAXS = (2, 64, 96)


@pytest.fixture(scope="module")
def baseline():
    gc.collect()      # a ctx an earlier test dropped without closing goes now, not in the middle of a comparison
    return B.live_resources()


def images(n, h, w, seed):
    return ctpn_amd.weights.synthetic_images(n, h, w, seed)


def lines_for(h, w):
    """two lines inside an h x w image, one of them slanted"""
    return np.array([line(4.0, 4.0, w - 12.0, 10.0, 0.95, slant=2.0), line(6.0, h / 2.0, w / 2.0, 8.0, 0.9)], np.float64)


def writers(ctx, tmp_path, tag, n, h, w):
    """every writer and the crops over an n x h x w batch, uniform and as a ragged canvas"""
    px = images(n, h, w, 40)
    recs = [lines_for(h, w) for _ in range(n)]
    heights = [h - 16 * (i & 1) for i in range(n)]
    t = lambda name, k=n: [str(tmp_path / ("%s_%s_%d" % (tag, name, i))) for i in range(k)]      # noqa: E731
    for entropy in ("host", "device"):
        assert len(ctx.encode_jpeg_batch(px, entropy=entropy)) == n
        assert len(ctx.encode_jpeg_mixed([px[0], px[0][: h // 2, : w // 2]], entropy=entropy)) == 2
        assert len(ctx.write_line_crops(px, recs, crop_h=16, max_w=w, paths=t("crop_" + entropy, 2 * n), entropy=entropy)) == 2 * n
        ctx.write_annotated_files_ragged(images=px, heights=heights, recs=recs, scales=[1.0] * n, paths=t("ann_ragged_" + entropy), entropy=entropy)
    assert len(ctx.encode_png_batch(px)) == n
    assert len(ctx.encode_png_mixed([px[0], px[0][: h // 2, : w // 2]])) == 2
    crops, widths = ctx.crop_lines(px, recs, crop_h=16, max_w=w)
    assert crops.shape[0] == 2 * n == len(widths)
    crops, widths = ctx.crop_lines(px, recs, crop_h=16, max_w=w, heights=heights)
    assert crops.shape[0] == 2 * n
    assert len(ctx.write_line_crops(px, recs, crop_h=16, max_w=w, paths=t("crop_png", 2 * n), format="png")) == 2 * n
    assert len(ctx.write_line_crops(px, recs, crop_h=16, max_w=w, paths=t("crop_ragged", 2 * n), heights=heights)) == 2 * n
    assert len(ctx.write_line_crops(px, recs, crop_h=16, max_w=w, paths=t("crop_ragged_png", 2 * n), heights=heights, format="png")) == 2 * n
    ctx.write_annotated_png_files(images=px, recs=recs, scale=0.5, paths=t("ann_png"))
    ctx.write_annotated_png_files_ragged(images=px, heights=heights, recs=recs, scales=[0.5] * n, paths=t("ann_ragged_png"))
    files = [encode(scene(h, w, 3 + i), 90) for i in range(n)]
    ptr, shape = ctx.decode_jpeg_batch(files)             # a live batch: the annotated JPEG writer takes device images only
    ctx.write_annotated_files(ptr, shape, recs, 0.5, t("ann"))
    ctx.write_annotated_files(ptr, shape, recs, 1.0, t("ann_dev"), entropy="device")


def drive(ctx, arena, tmp_path):
    n, h, w = MAXS
    ctx.load_weights(arena)
    a, b = images(n, h, w, 11), images(n, h, w, 13)
    ctx.forward(a)
    ctx.forward_ragged(a, [h, h - 16])
    ctx.detect_submit(images=a, slot=0)
    ctx.detect_submit(images=b, slot=1)                   # finds slot 0 in flight: forward set 1
    assert ctx.forward_sets()[0] == 2 and ctx.forward_sets()[2] > 0
    ctx.detect_collect(0)
    ctx.detect_collect(1)
    ctx.detect_submit(images=a, slot=0, heights=[h - 16, h])
    ctx.detect_collect(0)
    small = [encode(scene(16, 16, 5), 90), encode(scene(16, 16, 6), 90)]      # a uniform batch: one layout
    for entropy in ("host", "device"):
        ptr, shape = ctx.decode_jpeg_batch(small, entropy=entropy)
        assert shape == (2, 16, 16)
        (ptr, shape), hts = ctx.decode_jpeg_ragged([encode(scene(16, 16, 5, True), 90), encode(scene(24, 16, 6), 90, 2)], [(16, 16), (24, 16)], [1.0, 1.0], 24, 16, entropy=entropy)
        assert tuple(hts) == (16, 24)
    for entropy in ("host", "device"):                    # larger files: both buffer sets grow, their device blocks are retired
        ptr, shape = ctx.decode_jpeg_batch([encode(scene(48, 64, 7 + i), 90) for i in range(2)], fx=0.5, fy=0.5, entropy=entropy)
        assert shape == (2, 24, 32)
        ctx.jpeg_batch_fetch(ptr, shape)
    writers(ctx, tmp_path, "small", 1, 32, 48)
    writers(ctx, tmp_path, "large", 2, 64, 96)            # every buffer of the output stages grows
    ctx.profile_enable(True)
    ctx.forward(a)
    ctx.profile_enable(False)
    ctx.profile_enable(2)
    ctx.forward(b)
    ctx.sync()
    assert ctx.profile_read()["conv_gemm"]["launches"] > 0


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_a_ctx_returns_everything_it_took(baseline, arena, tmp_path, prec):
    ctx = ctpn_amd.Context(0, *MAXS, prec)
    try:
        drive(ctx, arena, tmp_path)
        live = B.live_resources()
        assert all(x > y for x, y in zip(live, baseline)), (live, baseline)
    finally:
        ctx.close()
    assert B.live_resources() == baseline


def test_a_postproc_ctx_returns_everything_it_took(baseline):
    ctx = ctpn_amd.Context(0, 2, 64, 96, postproc_only=True)
    try:
        rng = np.random.default_rng(5)
        cls = rng.random((2, 4, 6, 20), np.float32)
        rois = ctx.proposals_from_host(cls, rng.standard_normal((2, 4, 6, 40)).astype(np.float32) * 0.1, [[64, 96, 1.0]] * 2)
        assert len(rois) == 2
        live = B.live_resources()
        assert all(x > y for x, y in zip(live, baseline)), (live, baseline)
    finally:
        ctx.close()
    assert B.live_resources() == baseline


def test_a_refused_create_leaves_nothing(baseline):
    lib = B.load_library()
    h = C.c_void_p()
    assert lib.ctpn_create(C.byref(h), 0, 1, 64, 64, 7) == -1 and not h.value          # unknown precision
    assert B.live_resources() == baseline
    assert lib.ctpn_create(C.byref(h), 0, 1, 8, 64, 1) == -1 and not h.value           # max_h = 8
    assert B.live_resources() == baseline


HOOKS = {
    "debug_cvt_bf16": lambda: B.debug_cvt_bf16(np.linspace(-3.0, 3.0, 257, dtype=np.float32)),
    "debug_lds_dma": lambda: B.debug_lds_dma(np.arange(2048, dtype=np.uint32).astype(np.uint8)),
    "debug_conv3x3": lambda: B.debug_conv3x3(np.ones((1, 4, 4, 64), np.float32), np.full((3, 3, 64, 64), 0.01, np.float32), np.zeros(64, np.float32), "bf16"),
    "resize_linear": lambda: B.resize_linear(images(1, 16, 24, 3)[0], 0.5, 0.5),
    "debug_connect": lambda: B.debug_connect(np.array([[0.9, 16.0 * k, 20.0, 16.0 * k + 15.0, 40.0] for k in range(4)], np.float32), (64, 96)),
}


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_a_stateless_hook_leaves_nothing(baseline, hook):
    before = B.live_resources()
    HOOKS[hook]()
    assert B.live_resources() == before == baseline
