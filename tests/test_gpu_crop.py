"""GPU: ctpn_crop_lines (csrc/crop.hip, api_crops.hip) against the numpy restatement of its definition (tests/crop_ref.py), np.array_equal
over the whole output, padding included: host and device images, host and device output, uneven line counts, odd widths, lines outside the
image, buffer growth, the sizing call, real detections in both modes, demo_batch's crops_dir. (The arithmetic itself is pinned on the CPU
from the kernel's source text: tests/test_crop.py.)"""
import ctypes as C
import io
import os

import numpy as np
import pytest
from PIL import Image

import ctpn_amd
from ctpn_amd import _binding as B
import crop_ref as R
from util_jpeg import encode, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(arena):
    with ctpn_amd.Context(0, 4, 256, 384, "bf16") as c:
        c.load_weights(arena)
        yield c


def noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def box(x, y, ws, hs, slant=0.0, shear=0.0):
    return [x, y, x + ws, y + slant, x + shear, y + hs, x + ws + shear, y + hs + slant, 0.9]


def check(ctx, imgs, recs, crop_h, max_w, pad=0):
    crops, widths = ctx.crop_lines(imgs, recs, crop_h=crop_h, max_w=max_w, pad_value=pad)
    want, want_w = R.crop_lines(imgs, recs, crop_h, max_w, pad)
    assert crops.shape == want.shape and crops.dtype == np.uint8
    assert np.array_equal(widths, want_w)
    assert np.array_equal(crops, want)
    return crops, widths


@pytest.mark.parametrize("pad", [0, 255])
@pytest.mark.parametrize("crop_h", [8, 32])
def test_host_images_with_uneven_line_counts(ctx, crop_h, pad):
    imgs = noise(3, 48, 80, 1)
    recs = [np.array([box(3.0, 5.0, 40.0, 12.0), box(20.0, 20.0, 45.5, 10.0, slant=-7.25, shear=3.5)]), np.zeros((0, 9)),
            np.array([box(10.25, 7.5, 33.3, 9.75), box(5.0, 4.0, 50.0, 14.0, slant=6.0), box(-12.5, -6.0, 40.0, 16.0, shear=2.0)])]
    crops, widths = check(ctx, imgs, recs, crop_h, 64, pad)
    assert crops.shape[0] == 5
    # the zero in the middle: image 2's lines were cut from image 2
    assert np.array_equal(crops[2], R.crop_line(imgs[2], recs[2][0], crop_h, 64, pad)[0])
    # the same lines as a packed array with counts
    packed = np.full((3, 4, 9), 1e6)
    for i, r in enumerate(recs):
        packed[i, :len(r)] = r
    again, _ = ctx.crop_lines(imgs, packed, [2, 0, 3], crop_h=crop_h, max_w=64, pad_value=pad)
    assert np.array_equal(again, crops)


def test_odd_image_width_and_odd_crop_widths(ctx):
    """33 x 81 images (243 bytes per row); widths 1, 3, 5, 63 for the stores of the row tail; a squeezed line; a line wholly outside"""
    imgs = noise(2, 33, 81, 2)
    recs = [np.array([box(7.0, 4.0, float(ws), 8.0) for ws in (1, 3, 5, 63)] + [box(4.5, 6.25, 2.75, 8.0, slant=0.5)]),
            np.array([box(1.0, 2.0, 79.0, 4.0, slant=1.0), box(-300.0, -200.0, 50.0, 8.0), box(100.0, 40.0, 30.0, 8.0, slant=2.0)])]
    crops, widths = check(ctx, imgs, recs, 8, 64, 9)
    assert widths.tolist() == [1, 3, 5, 63, 3, 64, 50, 30]
    assert (crops[6][:, :50] == imgs[1][0, 0]).all() and (crops[6][:, 50:] == 9).all()      # above and left of the image: its first pixel
    assert (crops[7][:, :30] == imgs[1][32, 80]).all()                                      # below and right of it: its last
    check(ctx, imgs, recs, 32, 64)


def test_device_batch_is_cropped_where_it_lies(ctx, tmp_path):
    h, w, n = 120, 200, 3
    names = []
    for i in range(n):
        names.append(str(tmp_path / ("c%d.jpg" % i)))
        with open(names[-1], "wb") as f:
            f.write(encode(scene(h, w, 21 + i), 92, 2))
    recs = [np.array([box(10.0, 12.0, 150.0, 20.0, slant=4.0), box(-5.0, 80.0, 220.0, 30.0)]), np.array([box(33.3, 44.4, 99.9, 17.7, slant=-3.0, shear=2.0)]),
            np.array([box(0.0, 0.0, 200.0, 120.0), box(60.0, 50.0, 80.0, 16.0), box(150.0, 100.0, 80.0, 40.0, slant=5.0)])]
    ptr, shape = ctx.decode_jpeg_files(names, h, w)
    crops, widths = ctx.crop_lines(None, recs, crop_h=32, max_w=256, device_ptr=ptr, shape=shape)      # no fetch in front of it
    px = ctx.jpeg_batch_fetch(ptr, shape)
    want, want_w = R.crop_lines(px, recs, 32, 256)
    assert np.array_equal(widths, want_w) and np.array_equal(crops, want)


def test_device_output_equals_host_output(ctx):
    import torch
    imgs = noise(2, 48, 80, 3)
    recs = [np.array([box(3.0, 5.0, 40.0, 12.0, slant=2.0)]), np.array([box(10.0, 7.0, 60.0, 9.0), box(-4.0, 30.0, 50.0, 14.0, shear=3.0)])]
    host, widths = ctx.crop_lines(imgs, recs, crop_h=16, max_w=128, pad_value=3)
    buf = torch.full((host.size + 8,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    none, widths_d = ctx.crop_lines(imgs, recs, crop_h=16, max_w=128, pad_value=3, out_device_ptr=buf.data_ptr(), out_capacity=host.size)
    back = buf.cpu().numpy()
    assert none is None and np.array_equal(widths_d, widths)
    assert np.array_equal(back[:host.size].reshape(host.shape), host) and (back[host.size:] == 0xEE).all()
    with pytest.raises(B.CtpnError) as e:                  # three dwords per store: a device output is dword-aligned
        ctx.crop_lines(imgs, recs, crop_h=16, max_w=128, out_device_ptr=buf.data_ptr() + 1, out_capacity=host.size)
    assert e.value.code == -1 and "aligned" in str(e.value)


def test_buffers_grow_and_are_reused(ctx):
    small = noise(1, 33, 81, 4)
    small_recs = [np.array([box(5.0, 5.0, 50.0, 10.0, slant=3.0)])]
    first, _ = check(ctx, small, small_recs, 8, 64)
    rng = np.random.default_rng(5)
    big = noise(4, 256, 384, 6)
    big_recs = [np.array([box(rng.uniform(-20, 300), rng.uniform(-10, 240), rng.uniform(5, 380), rng.uniform(4, 40), rng.uniform(-8, 8), rng.uniform(-5, 5))
                          for _ in range(40)]) for _ in range(4)]
    crops, widths = check(ctx, big, big_recs, 32, 384)
    assert crops.shape[0] == 160 and widths.max() == 384 and widths.min() < 100
    third, _ = check(ctx, small, small_recs, 8, 64)
    assert np.array_equal(third, first)


def raw_call(ctx, imgs, packed, counts, crop_h, max_w, pad, out, capacity, widths, total):
    n, h, w = imgs.shape[:3]
    return ctx._lib.ctpn_crop_lines(ctx._h, imgs.ctypes.data_as(C.c_void_p), 0, n, h, w, B._ptr(packed, C.c_double), packed.shape[1], B._ptr(counts, C.c_int),
                                    crop_h, max_w, pad, None if out is None else out.ctypes.data_as(C.c_void_p), 0, capacity, B._ptr(widths, C.c_int), C.byref(total))


def test_sizing_capacity_and_empty_calls(ctx):
    imgs = noise(2, 48, 80, 7)
    packed = np.zeros((2, 3, 9))
    packed[0, 0], packed[1, 0], packed[1, 1] = box(3.0, 5.0, 40.0, 12.0), box(10.0, 7.0, 60.0, 9.0), box(-4.0, 30.0, 50.0, 14.0, shear=3.0)
    counts = np.array([1, 2], np.int32)
    widths, total = np.full(3, -1, np.int32), C.c_int(-1)
    assert raw_call(ctx, imgs, packed, counts, 16, 128, 0, None, 0, widths, total) == 0                    # sizes the call
    assert total.value == 3 and widths.tolist() == [R.width(packed[i, j], 16, 128) for i, j in ((0, 0), (1, 0), (1, 1))]
    need = 3 * 16 * 128 * 3
    out = np.full(need, 0xAB, np.uint8)
    total.value = -1
    assert raw_call(ctx, imgs, packed, counts, 16, 128, 0, out, need - 1, widths, total) == B.CTPN_ERR_CAPACITY
    assert total.value == 3 and (out == 0xAB).all() and b"need" in ctx._lib.ctpn_last_error()
    assert raw_call(ctx, imgs, packed, counts, 16, 128, 0, out, need, widths, total) == 0
    assert np.array_equal(out.reshape(3, 16, 128, 3), R.crop_lines(imgs, [packed[0, :1], packed[1, :2]], 16, 128)[0])
    # no lines at all: fine, nothing launched, nothing written
    out[:] = 0xAB
    total.value = -1
    assert raw_call(ctx, imgs, packed, np.zeros(2, np.int32), 16, 128, 0, out, need, widths, total) == 0 and total.value == 0 and (out == 0xAB).all()
    crops, w0 = ctx.crop_lines(imgs, [np.zeros((0, 9)), np.zeros((0, 9))], crop_h=16, max_w=128)
    assert crops.shape == (0, 16, 128, 3) and w0.shape == (0,)


def test_argument_and_state_errors(ctx):
    imgs = noise(1, 48, 80, 8)
    recs = [np.array([box(3.0, 5.0, 40.0, 12.0)])]
    for kw in ({"crop_h": 0}, {"crop_h": 257}, {"max_w": 0}, {"max_w": 6}, {"max_w": 65536}, {"pad_value": -1}, {"pad_value": 256}):
        with pytest.raises(B.CtpnError) as e:
            ctx.crop_lines(imgs, recs, **kw)
        assert e.value.code == -1, kw
    for v in (np.nan, np.inf):
        bad = [recs[0].copy()]
        bad[0][0, 5] = v
        with pytest.raises(B.CtpnError) as e:
            ctx.crop_lines(imgs, bad)
        assert e.value.code == -1 and "finite" in str(e.value)
    with pytest.raises(B.CtpnError) as e:                  # more lines than the capacity says
        ctx.crop_lines(imgs, np.zeros((1, 2, 9)), [3])
    assert e.value.code == -1
    with ctpn_amd.Context(0, 1, 64, 64, postproc_only=True) as pp:
        with pytest.raises(B.CtpnError) as e:
            pp.crop_lines(imgs, recs)
        assert e.value.code == -3 and "post-processing-only" in str(e.value)
    assert ctx.crop_lines(imgs, recs)[0].shape == (1, 32, 512, 3)      # the ctx is as usable as before


@pytest.mark.parametrize("mode", ["H", "O"])
def test_real_detections(ctx, mode):
    imgs = np.stack([np.ascontiguousarray(scene(256, 384, 30 + i)[:, :, ::-1]) for i in range(2)])
    recs = ctx.detect(imgs, mode=mode)
    print("mode %s: %s lines" % (mode, [len(r) for r in recs]))
    if sum(len(r) for r in recs) == 0:
        recs[1] = np.array([box(40.0, 60.0, 200.0, 24.0, slant=9.0)])
    crops, widths = check(ctx, imgs, recs, 32, 512)
    assert crops.shape[0] == sum(len(r) for r in recs) > 0


def test_demo_batch_writes_one_crop_file_per_line(tmp_path, arena):
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.ctpn import demo as D
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg
    src, out, crops_dir = tmp_path / "in", tmp_path / "out", tmp_path / "crops"
    src.mkdir()
    h, w = 120, 200
    for i in range(5):
        (src / ("im%02d.jpg" % i)).write_bytes(encode(scene(h, w, 50 + i), 90, 2))
    cfg.TEST.PRECISION = "bf16"
    net = get_network("VGGnet_test")
    net.load_arena(arena)
    try:
        names = demo_batch.list_images(str(src))
        logs = []
        res = demo_batch.run(net, names, str(out), batch=3, write_images=False, log=logs.append, decode="gpu", crops_dir=str(crops_dir), crop_h=32)
        total = sum(len(res[nm]) for nm in names)
        files = sorted(os.listdir(str(crops_dir)))
        assert len(files) == total > 0, logs
        assert "Text-line crops: %d of height 32" % total in logs[-1], logs
        assert sorted(os.listdir(str(out))) == ["res_im%02d.txt" % i for i in range(5)]
        # one file against the restatement: the line's crop out of the image the detector was fed, trimmed, through Pillow's writer
        nm = next(n for n in names if len(res[n]))
        f = D.resize_factor((h, w), TextLineCfg.SCALE, TextLineCfg.MAX_SCALE)
        ptr, shape = net.ctx.decode_jpeg_files([nm], h, w, f, f)
        px = net.ctx.jpeg_batch_fetch(ptr, shape)[0]
        k = len(res[nm]) - 1
        crop, wc = R.crop_line(px, res[nm][k], 32, 512)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(crop[:, :wc, ::-1])).save(buf, "JPEG", quality=95, subsampling=2, optimize=False)
        stem = os.path.basename(nm).split(".")[0]
        assert (crops_dir / ("%s_%d.jpg" % (stem, k))).read_bytes() == buf.getvalue()
        with pytest.raises(ValueError):
            demo_batch.run(net, names, str(out), batch=3, decode="host", crops_dir=str(crops_dir))
    finally:
        net.close()
