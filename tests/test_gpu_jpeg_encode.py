"""GPU: the JPEG writer behind the C ABI (csrc/jpeg_enc.hip, api_jpeg_out.hip, api_out_stage.hip) against Pillow's files, byte for byte: ctpn_encode_jpeg_batch on
host and device pixels, draw_boxes_kernel against ctpn_draw_boxes through ctpn_write_annotated_files, demo_batch's encode='gpu' against its
default writer, batches in flight, buffer growth. (The arithmetic itself is pinned on the CPU from the kernels' source text:
tests/test_jpeg_encode.py.)"""
import io
import os

import numpy as np
import pytest
from PIL import Image

import ctpn_amd
from ctpn_amd import _binding as B
from util_jpeg import encode, pillow_bgr, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(arena):
    with ctpn_amd.Context(0, 4, 256, 384, "bf16") as c:
        c.load_weights(arena)
        yield c


def pillow_file(bgr, quality=95):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


def pictures(n, h, w, seed):
    """n different BGR images of one size: four scenes and noise, shifted"""
    base = [scene(h, w, seed + k) for k in range(3)] + [np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)]
    return np.stack([np.roll(base[i % 4], (7 * i, 13 * i), (0, 1)) for i in range(n)])


@pytest.mark.parametrize("h,w", [(600, 900), (1280, 1920)])
@pytest.mark.parametrize("n", [1, 3, 32])
def test_host_pixels_equal_pillow(ctx, n, h, w):
    quality = {1: 75, 3: 100, 32: 95}[n]
    imgs = pictures(n, h, w, n + h)
    files = ctx.encode_jpeg_batch(imgs, quality=quality)
    assert len(files) == n
    for i in range(n):
        assert files[i] == pillow_file(imgs[i], quality), (i, len(files[i]))


@pytest.mark.parametrize("quality", [1, 50, 75, 95, 100])
def test_small_and_odd_sizes_equal_pillow(ctx, quality):
    """every edge-expansion branch on the device, and the library's own quality tables against libjpeg's at five qualities"""
    for h, w in [(1, 1), (1, 17), (2, 15), (15, 2), (16, 16), (17, 1), (17, 17), (15, 33), (31, 47), (129, 127), (233, 377)]:
        imgs = pictures(3, max(h, 8), max(w, 8), h * 7 + w)[:, :h, :w]
        files = ctx.encode_jpeg_batch(imgs, quality=quality)
        for i in range(3):
            assert files[i] == pillow_file(imgs[i], quality), (h, w, i)


def test_every_quality_table(ctx):
    img = pictures(1, 24, 40, 5)
    for q in range(1, 101):
        assert ctx.encode_jpeg_batch(img, quality=q)[0] == pillow_file(img[0], q), q


def test_device_pixels_straight_from_the_decoder(ctx, tmp_path):
    """a batch of ctpn_decode_jpeg_files, still on the device, re-encoded: the bytes of Image.save of the fetched pixels"""
    for n, (h, w) in ((3, (600, 900)), (32, (120, 200)), (1, (1280, 1920))):
        names = []
        for i in range(n):
            names.append(str(tmp_path / ("d%d_%d.jpg" % (h, i))))
            with open(names[-1], "wb") as f:
                f.write(encode(scene(h, w, 11 * i + n), 92, 2))
        ptr, shape = ctx.decode_jpeg_files(names, h, w)
        files = ctx.encode_jpeg_batch(device_ptr=ptr, shape=shape, quality=95)
        px = ctx.jpeg_batch_fetch(ptr, shape)
        for i in range(n):
            assert files[i] == pillow_file(px[i], 95), (n, i)


def lines_for(h, w, seed):
    """records with both colours, overlapping lines, lines partly and wholly outside the image, skipped (thin) records, slanted quadrilaterals"""
    rng = np.random.default_rng(seed)
    recs = []

    def quad(x1, y1, x2, y2, score, slant=0.0):
        recs.append([x1, y1 + slant, x2, y1 - slant, x1, y2 + slant, x2, y2 - slant, score])
    for _ in range(12):
        x1, y1 = rng.uniform(-0.2 * w, 0.9 * w), rng.uniform(-0.2 * h, 0.9 * h)
        quad(x1, y1, x1 + rng.uniform(20, 0.6 * w), y1 + rng.uniform(8, 0.3 * h), rng.choice([0.95, 0.8, 0.9, 0.8999]), rng.uniform(-6, 6))
    quad(10.5, 20.25, w - 10.75, 60.5, 0.99)
    quad(30.0, 40.0, w * 0.7, 80.0, 0.5)                   # overlaps the previous one, other colour, drawn later
    quad(50.0, 30.0, w * 0.5, 70.0, 0.93)
    quad(-500.0, -300.0, -100.0, -200.0, 0.95)             # wholly outside
    quad(w + 5.0, 10.0, w + 300.0, 50.0, 0.95)
    quad(-40.0, h - 20.0, w + 40.0, h + 30.0, 0.7)         # partly outside, longer than the image
    quad(100.0, 98.0, 200.0, 140.0, 0.95)                  # skipped: |x1 - y1| < 5
    recs.append([60.0, 10.0, 300.0, 62.0, 60.0, 50.0, 300.0, 50.0, 0.95])      # skipped: |y2 - x1| < 5
    quad(5.0, 200.0, 6.0, 201.0, 0.95)                     # a dot
    return np.array(recs, np.float64)


@pytest.mark.parametrize("scale", [1.0, 2.0, 0.625])
def test_draw_kernel_equals_the_host_rasteriser(ctx, tmp_path, scale):
    """ctpn_write_annotated_files against ctpn_draw_boxes + ctpn_resize + Pillow on the fetched batch; scale 1.0 is the un-resized batch, where
    every byte of the file is the drawing's. The decoder's buffer is left as it was."""
    h, w = 240, 360
    datas = [encode(scene(h, w, 70 + i), 95, 0) for i in range(5)]
    ptr, shape = ctx.decode_jpeg_batch(datas, h, w)
    before = ctx.jpeg_batch_fetch(ptr, shape)
    recs = [lines_for(h, w, 1), lines_for(h, w, 2)[::-1].copy(), np.zeros((0, 9)), lines_for(h, w, 3)[:5], lines_for(h, w, 4)]
    paths = [str(tmp_path / ("a%d.jpg" % i)) for i in range(5)]
    ctx.write_annotated_files(ptr, shape, recs, scale, paths)
    assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), before)
    changed = 0
    for i in range(5):
        drawn = B.draw_boxes(before[i].copy(), recs[i])
        changed += int((drawn != before[i]).any())
        want = drawn if scale == 1.0 else B.resize_linear(drawn, 1.0 / scale, 1.0 / scale)
        with open(paths[i], "rb") as f:
            assert f.read() == pillow_file(want, 95), i
    assert changed == 4                                    # (the image without lines is written as it is)


def test_errors(ctx, tmp_path):
    imgs = pictures(2, 40, 56, 3)
    lib = B.load_library()
    with pytest.raises(B.CtpnError) as e:
        ctx.encode_jpeg_batch(imgs, quality=0)
    assert e.value.code == -1
    with pytest.raises(B.CtpnError) as e:
        ctx.encode_jpeg_batch(imgs, quality=101)
    assert e.value.code == -1
    import ctypes as C
    bufs = np.zeros((2, 64), np.uint8)
    ptrs = (C.c_void_p * 2)(bufs[0].ctypes.data, bufs[1].ctypes.data)
    caps, sizes = (C.c_size_t * 2)(64, 64), (C.c_size_t * 2)()
    assert lib.ctpn_encode_jpeg_batch(ctx._h, imgs.ctypes.data_as(C.c_void_p), 0, 2, 40, 56, 95, ptrs, caps, sizes) == -4
    assert [sizes[0], sizes[1]] == [len(pillow_file(imgs[i])) for i in range(2)]
    ptr, shape = ctx.decode_jpeg_batch([encode(scene(40, 56, 1), 90, 2)], 40, 56)
    with pytest.raises(B.CtpnError) as e:
        ctx.write_annotated_files(ptr, shape, [np.zeros((0, 9))], 1.0, [str(tmp_path / "no_such_dir" / "x.jpg")])
    assert e.value.code == -1 and "no_such_dir" in str(e.value)
    with pytest.raises(B.CtpnError):
        ctx.write_annotated_files(ptr, shape, [np.zeros((0, 9))], 0.0, [str(tmp_path / "x.jpg")])


def test_buffers_grow(ctx):
    small, big = pictures(1, 33, 47, 1), pictures(5, 700, 1100, 2)
    assert ctx.encode_jpeg_batch(small)[0] == pillow_file(small[0])
    files = ctx.encode_jpeg_batch(big, quality=90)
    for i in range(5):
        assert files[i] == pillow_file(big[i], 90)
    assert ctx.encode_jpeg_batch(small)[0] == pillow_file(small[0])


def test_three_batches_in_flight_write_the_lone_batch_files(ctx, tmp_path):
    """decode of batch k + 1, forward of batch k and the annotated files of batch k - 1, as demo_batch drives them, over six batches: every
    file equals the one its batch gives alone"""
    h, w, nb, n = 256, 384, 6, 4
    batches = [[encode(scene(h, w, 10 * b + i), 90, 2) for i in range(n)] for b in range(nb)]
    lone = []
    for b, datas in enumerate(batches):
        ptr, shape = ctx.decode_jpeg_batch(datas, h, w)
        recs = ctx.detect(device_ptr=ptr, shape=shape, mode="H")
        paths = [str(tmp_path / ("lone_%d_%d.jpg" % (b, i))) for i in range(n)]
        ctx.write_annotated_files(ptr, shape, recs, 1.0, paths)
        lone.append([open(p, "rb").read() for p in paths])
    assert sum(len(r) for r in recs) > 0
    pending = None

    def finish(job):
        slot, b, ptr, shape = job
        recs = ctx.detect_collect(slot, mode="H")
        paths = [str(tmp_path / ("fly_%d_%d.jpg" % (b, i))) for i in range(n)]
        ctx.write_annotated_files(ptr, shape, recs, 1.0, paths)
        for i in range(n):
            assert open(paths[i], "rb").read() == lone[b][i], (b, i)
    for k, datas in enumerate(batches):
        ptr, shape = ctx.decode_jpeg_batch(datas, h, w)
        ctx.detect_submit(device_ptr=ptr, shape=shape, slot=k & 1)
        if pending is not None:
            finish(pending)
        pending = (k & 1, k, ptr, shape)
    finish(pending)


def test_demo_batch_encode_gpu_writes_the_host_writers_files(tmp_path, arena):
    """demo_batch.run(decode='gpu', encode='gpu') against encode='host' on JPEG files of two sizes (one needs resize_im, so its annotated
    image is resized back by 1 / scale), a PNG and a CMYK JPEG: every res_*.txt and every image file byte-identical; the PNG and the CMYK
    file take the host writer."""
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    src, out_g, out_h = tmp_path / "in", tmp_path / "gpu", tmp_path / "host"
    src.mkdir()
    for i, (h, w) in enumerate([(300, 450), (300, 450), (600, 900), (300, 450), (600, 900), (300, 450)]):
        (src / ("im%02d.jpg" % i)).write_bytes(encode(scene(h, w, 40 + i), 90, 2))
    Image.fromarray(scene(300, 450, 99)).save(str(src / "im99.png"))
    Image.fromarray(scene(300, 450, 98)).convert("CMYK").save(str(src / "im98.jpg"), "JPEG", quality=90)
    cfg.TEST.PRECISION = "bf16"
    net = get_network("VGGnet_test")
    net.load_arena(arena)
    try:
        names = demo_batch.list_images(str(src))
        logs = []
        res_g = demo_batch.run(net, names, str(out_g), batch=3, write_images=True, log=logs.append, decode="gpu", encode="gpu")
        res_h = demo_batch.run(net, names, str(out_h), batch=3, write_images=True, log=lambda *_: None, decode="gpu", encode="host")
        assert "6 decoded on the device, 1 PNG files by the library, 1 on the host" in logs[0], logs
        assert "6 drawn, resized and JPEG-coded by the library" in logs[1] and "2 by the host writer" in logs[1], logs
        assert sorted(os.listdir(str(out_g))) == sorted(os.listdir(str(out_h))) and len(os.listdir(str(out_g))) == 16
        for nm in names:
            assert np.array_equal(res_g[nm], res_h[nm]), nm
        for f in sorted(os.listdir(str(out_g))):
            assert (out_g / f).read_bytes() == (out_h / f).read_bytes(), f
        assert sum(len(res_g[nm]) for nm in names) > 0
        with pytest.raises(ValueError):
            demo_batch.run(net, names, str(out_g), batch=3, decode="host", encode="gpu")
    finally:
        net.close()
