"""GPU: the PNG writer behind the C ABI (csrc/png_enc.hip, api_png_out.hip). The device form's files must equal the host form's
(ctpn_png_encode) byte for byte and decode (Pillow) to the pixels: the image set of tests/png_enc_ref.py grouped by size, host and device
pixels, a live batch of the JPEG decoder, calls of changing size alternating with the JPEG writer, ctpn_write_annotated_png_files against
ctpn_draw_boxes + ctpn_resize (exact: the format is lossless), the error codes, the traffic bound, and demo_batch's png_encode='gpu'.
(The tokeniser, the code construction and the container are pinned on the CPU from the kernels' source text: tests/test_png_encode.py.)"""
import ctypes as C
import io
import os

import numpy as np
import pytest
from PIL import Image

import ctpn_amd
from ctpn_amd import _binding as B
import png_enc_ref as R
from util_jpeg import encode, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(arena):
    with ctpn_amd.Context(0, 4, 256, 384, "bf16") as c:
        c.load_weights(arena)
        yield c


def pillow_bgr(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1]


def check(files, imgs):
    assert len(files) == len(imgs)
    for i, (f, im) in enumerate(zip(files, imgs)):
        assert f == B.png_encode(im), (i, im.shape, len(f))
        assert np.array_equal(pillow_bgr(f), im), (i, im.shape)


def three_pictures():
    """flat, noise, page: the images' parts of the buffers differ widely"""
    return np.stack([R.flat(96, 128), np.random.default_rng(3).integers(0, 256, (96, 128, 3), dtype=np.uint8), R.document_page(96, 128, seed=2)])


def test_the_cpu_set_grouped_by_size(ctx):
    groups = {}
    for name, im in R.images().items():
        groups.setdefault(im.shape, []).append(im)
    assert max(len(g) for g in groups.values()) >= 5      # the demo crops share one size
    for shape, members in groups.items():
        imgs = np.stack(members)
        check(ctx.encode_png_batch(imgs), imgs)
        st = ctx.png_encode_device_stats()
        assert st["device"] == len(members) and st["host"] == 0, (shape, st)


def test_three_different_pictures_in_one_batch_and_the_traffic_bound(ctx):
    imgs = three_pictures()
    files = ctx.encode_png_batch(imgs)
    check(files, imgs)
    assert len(files[0]) < len(files[2]) < len(files[1])
    st = ctx.png_encode_device_stats()
    n = len(imgs)
    assert st["device"] == n and st["host"] == 0 and st["pieces"] == n * ((96 * (1 + 3 * 128) + 255) // 256)
    assert st["d2h_bytes"] <= sum(len(f) for f in files) + 16 * n + 286 * 4 * n


def test_host_images_and_device_images_give_the_same_files(ctx):
    import torch
    imgs = np.stack([R.document_page(120, 200, seed=k) for k in range(3)])
    dev = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    a = ctx.encode_png_batch(imgs)
    b = ctx.encode_png_batch(device_ptr=dev.data_ptr(), shape=imgs.shape[:3])
    assert a == b
    check(a, imgs)


def test_a_live_batch_of_the_jpeg_decoder_goes_straight_in(ctx):
    datas = [encode(scene(48, 80, 5 + i), 92, 2) for i in range(2)]
    ptr, shape = ctx.decode_jpeg_batch(datas, 48, 80)
    files = ctx.encode_png_batch(device_ptr=ptr, shape=shape)
    check(files, ctx.jpeg_batch_fetch(ptr, shape))


def test_growing_and_shrinking_calls_alternating_with_the_jpeg_writer(ctx):
    rng = np.random.default_rng(8)
    for n, h, w in [(1, 9, 11), (2, 64, 96), (4, 200, 300), (2, 64, 96), (1, 9, 11), (3, 130, 70)]:
        imgs = np.stack([np.roll(R.document_page(h, w, seed=n + k), 3 * k, 1) for k in range(n)])
        imgs[:, ::7, ::5] = rng.integers(0, 256, imgs[:, ::7, ::5].shape, dtype=np.uint8)
        check(ctx.encode_png_batch(imgs), imgs)
        jf = ctx.encode_jpeg_batch(imgs, quality=90)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(imgs[0][:, :, ::-1])).save(buf, "JPEG", quality=90, subsampling=2)
        assert jf[0] == buf.getvalue()


def test_four_calls_back_to_back(ctx):
    imgs = three_pictures()
    first = ctx.encode_png_batch(imgs)
    for _ in range(3):
        assert ctx.encode_png_batch(imgs) == first
    check(first, imgs)


def lines3(h, w, seed):
    rng = np.random.default_rng(seed)
    recs = []
    for k in range(3):
        x1, y1 = rng.uniform(2, 0.4 * w), rng.uniform(2, 0.6 * h)
        x2, y2 = x1 + rng.uniform(20, 0.5 * w), y1 + rng.uniform(8, 0.3 * h)
        s = rng.uniform(-3, 3)
        recs.append([x1, y1 + s, x2, y1 - s, x1, y2 + s, x2, y2 - s, (0.95, 0.8, 0.9)[k]])
    return np.array(recs, np.float64)


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("on_device", [False, True])
def test_write_annotated_png_files_equals_draw_and_resize(ctx, tmp_path, scale, on_device):
    import torch
    h, w = 96, 128
    imgs = np.stack([scene(h, w, 21), R.document_page(h, w, seed=4)])
    recs = [lines3(h, w, 1), lines3(h, w, 2)]
    paths = [str(tmp_path / ("a%d.png" % i)) for i in range(2)]
    if on_device:
        dev = torch.from_numpy(imgs).cuda()
        torch.cuda.synchronize()
        ctx.write_annotated_png_files(device_ptr=dev.data_ptr(), shape=imgs.shape[:3], recs=recs, scale=scale, paths=paths)
        assert np.array_equal(dev.cpu().numpy(), imgs)      # the caller's batch is not drawn on
    else:
        ctx.write_annotated_png_files(images=imgs, recs=recs, scale=scale, paths=paths)
    for i in range(2):
        drawn = B.draw_boxes(imgs[i].copy(), recs[i])
        assert (drawn != imgs[i]).any()
        want = drawn if scale == 1.0 else B.resize_linear(drawn, 1.0 / scale, 1.0 / scale)
        with open(paths[i], "rb") as f:
            data = f.read()
        assert np.array_equal(pillow_bgr(data), want), i
        assert data == B.png_encode(want)
    # res-style empty line lists: the pictures themselves
    ctx.write_annotated_png_files(images=imgs, recs=[np.zeros((0, 9)), np.zeros((0, 9))], scale=1.0, paths=paths)
    for i in range(2):
        with open(paths[i], "rb") as f:
            assert np.array_equal(pillow_bgr(f.read()), imgs[i])


def test_an_unwritable_path_is_an_argument_error_with_its_name(ctx, tmp_path):
    imgs = three_pictures()[:2]
    bad = str(tmp_path / "no-such-directory" / "x.png")
    with pytest.raises(B.CtpnError) as e:
        ctx.write_annotated_png_files(images=imgs, recs=[np.zeros((0, 9))] * 2, scale=1.0, paths=[str(tmp_path / "ok.png"), bad])
    assert e.value.code == -1 and bad in str(e.value)


def test_errors(ctx):
    lib = B.load_library()
    imgs = three_pictures()[:1]
    px = imgs.ctypes.data_as(C.c_void_p)
    buf = np.zeros((1, 65536), np.uint8)
    ptrs, caps, sizes = (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(buf.shape[1]), (C.c_size_t * 1)()
    h = ctx._h
    assert lib.ctpn_encode_png_batch(h, px, 0, 1, 96, 128, ptrs, caps, sizes) == 0
    assert lib.ctpn_encode_png_batch(None, px, 0, 1, 96, 128, ptrs, caps, sizes) == -1
    assert lib.ctpn_encode_png_batch(h, None, 0, 1, 96, 128, ptrs, caps, sizes) == -1
    assert lib.ctpn_encode_png_batch(h, px, 0, 1, 96, 128, None, caps, sizes) == -1
    assert lib.ctpn_encode_png_batch(h, px, 0, 1, 96, 128, ptrs, None, sizes) == -1
    assert lib.ctpn_encode_png_batch(h, px, 0, 1, 96, 128, ptrs, caps, None) == -1
    assert lib.ctpn_encode_png_batch(h, px, 0, 0, 96, 128, ptrs, caps, sizes) == -1      # n = 0
    assert lib.ctpn_encode_png_batch(h, px, 0, 1, 0, 128, ptrs, caps, sizes) == -1
    # h (1 + 3 w) above 2^27: refused before any allocation or launch (a 12.9 GB batch could not be staged: the call returns at once)
    assert lib.ctpn_encode_png_batch(h, px, 0, 1, 65535, 65535, ptrs, caps, sizes) == -1
    assert "2^27" in lib.ctpn_last_error().decode()
    small = (C.c_size_t * 1)(100)
    assert lib.ctpn_encode_png_batch(h, px, 0, 1, 96, 128, ptrs, small, sizes) == B.CTPN_ERR_CAPACITY and sizes[0] == len(B.png_encode(imgs[0]))
    cnt = (C.c_int * 1)(0)
    keep, arr = B._path_array(["/tmp/never-written.png"])
    assert lib.ctpn_write_annotated_png_files(h, px, 0, 1, 65535, 65535, None, 0, cnt, 1.0, arr) == -1
    assert lib.ctpn_write_annotated_png_files(h, None, 0, 1, 96, 128, None, 0, cnt, 1.0, arr) == -1
    assert lib.ctpn_write_annotated_png_files(h, px, 0, 0, 96, 128, None, 0, cnt, 1.0, arr) == -1
    assert lib.ctpn_write_annotated_png_files(h, px, 0, 1, 96, 128, None, 0, None, 1.0, arr) == -1
    assert lib.ctpn_write_annotated_png_files(h, px, 0, 1, 96, 128, None, 0, cnt, 1.0, None) == -1
    assert lib.ctpn_write_annotated_png_files(h, px, 0, 1, 96, 128, None, 0, cnt, 0.0, arr) == -1
    assert not os.path.exists("/tmp/never-written.png")
    with ctpn_amd.Context(0, 1, 96, 128, postproc_only=True) as pp:
        assert lib.ctpn_encode_png_batch(pp._h, px, 0, 1, 96, 128, ptrs, caps, sizes) == -3
        assert lib.ctpn_write_annotated_png_files(pp._h, px, 0, 1, 96, 128, None, 0, cnt, 1.0, arr) == -3


def test_demo_batch_png_encode_gpu(tmp_path, arena):
    """demo_batch.run(decode='gpu', png_encode='gpu') against png_encode='host' on two PNG files and two JPEG files: the same res_*.txt,
    PNG outputs that decode to the same pixels, JPEG outputs untouched, and the two PNG files counted as the library's."""
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    src, out_g, out_h = tmp_path / "in", tmp_path / "gpu", tmp_path / "host"
    src.mkdir()
    for i in range(2):
        Image.fromarray(scene(150, 225, 60 + i)).save(str(src / ("p%d.png" % i)))
        (src / ("j%d.jpg" % i)).write_bytes(encode(scene(150, 225, 70 + i), 90, 2))
    cfg.TEST.PRECISION = "bf16"
    net = get_network("VGGnet_test")
    net.load_arena(arena)
    try:
        names = demo_batch.list_images(str(src))
        logs = []
        res_g = demo_batch.run(net, names, str(out_g), batch=2, write_images=True, log=logs.append, decode="gpu", png_encode="gpu")
        res_h = demo_batch.run(net, names, str(out_h), batch=2, write_images=True, log=lambda *_: None, decode="gpu", png_encode="host")
        assert "2 drawn, resized and JPEG-coded by the library" in logs[1] and "2 by the host writer" in logs[1], logs      # enc_gpu, enc_host
        assert "2 are PNG files, coded on the device" in logs[2], logs
        assert sorted(os.listdir(str(out_g))) == sorted(os.listdir(str(out_h))) and len(os.listdir(str(out_g))) == 8
        for nm in names:
            assert np.array_equal(res_g[nm], res_h[nm]), nm
        for f in sorted(os.listdir(str(out_g))):
            a, b = (out_g / f).read_bytes(), (out_h / f).read_bytes()
            if f.endswith(".png"):
                assert a[:8] == b[:8] and a != b and np.array_equal(pillow_bgr(a), pillow_bgr(b)), f
                assert a == B.png_encode(np.ascontiguousarray(pillow_bgr(b)))
            else:
                assert a == b, f
        with pytest.raises(ValueError):
            demo_batch.run(net, names, str(out_g), batch=2, decode="host", png_encode="gpu")
    finally:
        net.close()
