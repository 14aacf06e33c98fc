"""GPU: JPEG files of images of mixed sizes in one call (ctpn_encode_jpeg_mixed: jpeg_fdct_mixed_kernel over a descriptor table) and the
text-line crops written as files where they are cut (ctpn_write_line_crops), both entropy forms. Every file is compared byte for byte
with Pillow's save(quality=q, subsampling=2) of the same pixels, and with ctpn_encode_jpeg_batch of that image alone -- which ties the
mixed kernel to the uniform one. (The table, the work-item search and the pixel read are pinned on the CPU: tests/test_jpeg_encode_mixed.py.)

NOT HERE: an image whose FLAG the device coder raises (a DC difference above 11 bits, an AC coefficient above 10), placed among others.
tests/test_gpu_jpeg_huff_enc.py raises the flag with constructed COEFFICIENTS through ctpn_jpeg_entropy_encode_device; the calls tested
here start from PIXELS, and 8-bit pixels cannot reach such a coefficient with the standard tables: the largest magnitude of an 8 x 8 DCT
coefficient of samples in -128 .. 127 is 1020 (sqrt(2) * 127.5 * sum |cos((2 x + 1) pi / 4)| = 1.4142 * 127.5 * 5.657), below 1024, at
quality 100 (every divisor 1) already. The host fallback inside a mixed call is tested with the image the device coder hands over for its
SIZE instead (more than 2^20 blocks): the same branch, the same per-image coefficient offset."""
import ctypes as C
import io
import os

import numpy as np
import pytest
from PIL import Image

import ctpn_amd
from ctpn_amd import _binding as B
import crop_ref as R
from test_gpu_crop import box, noise
from util_jpeg import encode, scene

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (8, 8), (16, 16), (17, 17), (15, 129), (33, 127), (32, 128), (8, 512), (32, 1), (256, 4)]
FORMS = ("host", "device")


@pytest.fixture(scope="module")
def ctx(arena):
    with ctpn_amd.Context(0, 4, 256, 384, "bf16") as c:
        c.load_weights(arena)
        yield c


def pillow_file(bgr, quality=95):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


def picture(h, w, seed):
    """BGR: noise for odd seeds, a scene for even ones"""
    if seed % 2:
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return np.ascontiguousarray(scene(max(h, 8), max(w, 8), seed)[:h, :w])


@pytest.fixture(scope="module")
def pictures():
    """one picture per size: computed once, shared, never changed"""
    return [picture(h, w, 11 + k) for k, (h, w) in enumerate(SIZES)]


@pytest.fixture(scope="module")
def pillow_files(pictures):
    """(index, quality) -> Pillow's file"""
    out = {(k, 95): pillow_file(im) for k, im in enumerate(pictures)}
    for k in (SIZES.index((17, 17)), SIZES.index((33, 127))):
        for q in (1, 100):
            out[(k, q)] = pillow_file(pictures[k], q)
    return out


@pytest.fixture(scope="module")
def uniform_files(ctx, pictures, pillow_files):
    """(index, quality) -> ctpn_encode_jpeg_batch's file of that image alone"""
    return {(k, q): ctx.encode_jpeg_batch(pictures[k][None], quality=q)[0] for (k, q) in pillow_files}


def device_source(images, extra=5):
    """the images in one device buffer at a pitch WIDER than 3 w (and odd: rows start at every alignment), three readable bytes behind the
    last pixel -> (tensor, heights, widths, pitches, offsets)"""
    import torch
    pitches = [3 * im.shape[1] + extra for im in images]
    offsets, at = [], 7
    for im, p in zip(images, pitches):
        offsets.append(at)
        at += im.shape[0] * p + 3
    host = np.full(at + 16, 0xA5, np.uint8)
    for im, p, o in zip(images, pitches, offsets):
        h, w = im.shape[:2]
        host[o: o + h * p].reshape(h, p)[:, : 3 * w] = im.reshape(h, 3 * w)
    t = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    return t, [im.shape[0] for im in images], [im.shape[1] for im in images], pitches, offsets


def mixed(ctx, images, quality, entropy, source):
    if source == "host":
        return ctx.encode_jpeg_mixed(images, quality=quality, entropy=entropy)
    t, hs, ws, pt, of = device_source(images)
    return ctx.encode_jpeg_mixed(quality=quality, entropy=entropy, device_ptr=t.data_ptr(), heights=hs, widths=ws, pitches=pt, offsets=of)


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("entropy", FORMS)
def test_mixed_sizes_equal_pillow_and_the_uniform_call(ctx, pictures, pillow_files, uniform_files, entropy, source):
    files = mixed(ctx, pictures, 95, entropy, source)                      # the ten sizes as one call
    for k, f in enumerate(files):
        assert f == pillow_files[(k, 95)], (SIZES[k], "pillow")
        assert f == uniform_files[(k, 95)], (SIZES[k], "uniform")
    if entropy == "device":
        stats = ctx.jpeg_encode_device_stats()
        assert stats["device"] == len(SIZES) and stats["host"] == 0
        assert stats["blocks"] == sum(6 * ((h + 15) // 16) * ((w + 15) // 16) for h, w in SIZES)
    assert mixed(ctx, pictures[::-1], 95, entropy, source) == files[::-1]      # nothing depends on the neighbours
    for size in ((1, 1), (17, 17), (8, 512)):                                  # n = 1
        k = SIZES.index(size)
        assert mixed(ctx, [pictures[k]], 95, entropy, source) == [pillow_files[(k, 95)]], size
    pair = [SIZES.index((17, 17)), SIZES.index((33, 127))]
    for q in (1, 100):
        got = mixed(ctx, [pictures[k] for k in pair], q, entropy, source)
        assert got == [pillow_files[(k, q)] for k in pair] and got == [uniform_files[(k, q)] for k in pair], q


LINES = {  # max_w -> one list of lines per image: uneven counts, an image without lines, a line one pixel wide, a line squeezed to max_w
    64: [[box(3.0, 5.0, 40.0, 12.0), box(20.0, 20.0, 45.5, 10.0, slant=-7.25, shear=3.5), box(7.0, 4.0, 0.25, 8.0)], [],
         [box(1.0, 2.0, 79.0, 4.0, slant=1.0), box(-12.5, -6.0, 40.0, 16.0, shear=2.0), box(10.25, 7.5, 33.3, 9.75), box(5.0, 4.0, 50.0, 14.0, slant=6.0)]],
    512: [[box(3.0, 5.0, 70.0, 6.0), box(7.0, 4.0, 0.25, 8.0)], [],
          [box(1.0, 2.0, 79.0, 1.0), box(20.0, 20.0, 45.5, 10.0, slant=-7.25, shear=3.5), box(-12.5, -6.0, 40.0, 16.0, shear=2.0)]],
}


def crop_files(ctx, tmp_path, tag, recs, crop_h, max_w, quality, entropy, images=None, device_ptr=None, shape=None):
    total = sum(len(r) for r in recs)
    paths = [str(tmp_path / ("%s_%03d.jpg" % (tag, k))) for k in range(total)]
    widths = ctx.write_line_crops(images, recs, crop_h=crop_h, max_w=max_w, pad_value=77, device_ptr=device_ptr, shape=shape, paths=paths, quality=quality, entropy=entropy)
    return [open(p, "rb").read() for p in paths], widths


@pytest.mark.parametrize("entropy", FORMS)
@pytest.mark.parametrize("max_w", [64, 512])
@pytest.mark.parametrize("crop_h", [8, 31, 32])
def test_crop_files_equal_pillows_files_of_the_in_memory_crops(ctx, tmp_path, crop_h, max_w, entropy):
    imgs = noise(3, 48, 80, 1)
    recs = [np.array(r, np.float64).reshape(-1, 9) for r in LINES[max_w]]
    crops, widths = ctx.crop_lines(imgs, recs, crop_h=crop_h, max_w=max_w, pad_value=77)
    assert widths.min() == 1 and widths.max() == max_w and [len(r) for r in recs][1] == 0
    for q in (95, 50):
        files, w2 = crop_files(ctx, tmp_path, "q%d" % q, recs, crop_h, max_w, q, entropy, images=imgs)
        assert np.array_equal(w2, widths)
        for k, f in enumerate(files):
            assert f == pillow_file(crops[k, :, : widths[k]], q), (k, int(widths[k]), q)      # (the pad columns never enter a file)


@pytest.mark.parametrize("entropy", FORMS)
def test_device_batch_is_cropped_and_written_where_it_lies(ctx, tmp_path, entropy):
    h, w = 120, 200
    datas = [encode(scene(h, w, 21 + i), 92, 2) for i in range(3)]
    recs = [np.array([box(10.0, 12.0, 150.0, 20.0, slant=4.0), box(-5.0, 80.0, 220.0, 30.0)]), np.array([box(33.3, 44.4, 99.9, 17.7, slant=-3.0, shear=2.0)]),
            np.array([box(0.0, 0.0, 200.0, 120.0), box(60.0, 50.0, 80.0, 16.0), box(150.0, 100.0, 80.0, 40.0, slant=5.0)])]
    ptr, shape = ctx.decode_jpeg_batch(datas, h, w)
    files, widths = crop_files(ctx, tmp_path, "dev", recs, 32, 256, 95, entropy, device_ptr=ptr, shape=shape)      # no fetch in front of it
    crops, want_w = ctx.crop_lines(None, recs, crop_h=32, max_w=256, pad_value=77, device_ptr=ptr, shape=shape)
    assert np.array_equal(widths, want_w) and np.array_equal(crops, R.crop_lines(ctx.jpeg_batch_fetch(ptr, shape), recs, 32, 256, 77)[0])
    assert files == [pillow_file(crops[k, :, : want_w[k]]) for k in range(len(files))]


def raw_crops(ctx, fn, imgs, packed, counts, crop_h, max_w, quality, paths, widths, total):
    n, h, w = imgs.shape[:3]
    arr = None if paths is None else (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    return fn(ctx._h, imgs.ctypes.data_as(C.c_void_p), 0, n, h, w, B._ptr(packed, C.c_double), packed.shape[1], B._ptr(counts, C.c_int), crop_h, max_w, 0, quality, arr,
              None if widths is None else B._ptr(widths, C.c_int), C.byref(total))


@pytest.mark.parametrize("name", ["ctpn_write_line_crops", "ctpn_write_line_crops_device"])
def test_sizing_and_empty_calls(ctx, tmp_path, name):
    fn = getattr(ctx._lib, name)
    imgs = noise(2, 48, 80, 7)
    packed = np.zeros((2, 3, 9))
    packed[0, 0], packed[1, 0], packed[1, 1] = box(3.0, 5.0, 40.0, 12.0), box(10.0, 7.0, 60.0, 9.0), box(-4.0, 30.0, 50.0, 14.0, shear=3.0)
    counts = np.array([1, 2], np.int32)
    widths, total = np.full(3, -1, np.int32), C.c_int(-1)
    assert raw_crops(ctx, fn, imgs, packed, counts, 16, 128, 95, None, widths, total) == 0                  # paths == NULL sizes the call
    want = [R.width(packed[i, j], 16, 128) for i, j in ((0, 0), (1, 0), (1, 1))]
    assert total.value == 3 and widths.tolist() == want
    total.value = -1
    assert raw_crops(ctx, fn, imgs, packed, counts, 16, 128, 95, None, None, total) == 0 and total.value == 3      # widths_out is nullable
    # no lines at all: CTPN_OK, nothing launched, nothing written -- with paths or without
    d = tmp_path / "none"
    d.mkdir()
    total.value = -1
    assert raw_crops(ctx, fn, imgs, packed, np.zeros(2, np.int32), 16, 128, 95, [str(d / "never.jpg")], widths, total) == 0 and total.value == 0
    assert os.listdir(str(d)) == []
    got = ctx.write_line_crops(imgs, [np.zeros((0, 9)), np.zeros((0, 9))], crop_h=16, max_w=128, paths=[], entropy="device" if name.endswith("device") else "host")
    assert got.shape == (0,) and os.listdir(str(d)) == []
    assert np.array_equal(ctx.write_line_crops(imgs, [packed[0, :1], packed[1, :2]], crop_h=16, max_w=128), want)      # the binding's sizing call


def test_an_image_the_device_coder_hands_over_comes_back_through_the_host_half(ctx, pictures, pillow_files):
    """65500 x 688 (libjpeg reads no wider image than 65500): 4094 x 43 MCUs = 1 056 252 blocks, above the 2^20 one launch group holds -- the device form hands it to the host half,
    which reads its coefficients at the image's own offset; the images around it are coded on the device"""
    import torch
    big_h, big_w = 688, 65500
    small = [pictures[SIZES.index(s)] for s in ((17, 17), (33, 127), (8, 512))]
    t, hs, ws, pt, of = device_source(small)
    big = torch.full((big_h * big_w * 3 + 16,), 93, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    # one table over two device buffers: offsets are relative to the lower address
    lo = min(t.data_ptr(), big.data_ptr())
    hs, ws, pt = hs[:1] + [big_h] + hs[1:], ws[:1] + [big_w] + ws[1:], pt[:1] + [big_w * 3] + pt[1:]
    of = [o + t.data_ptr() - lo for o in of]
    of = of[:1] + [big.data_ptr() - lo] + of[1:]
    files = {}
    for entropy in FORMS:
        files[entropy] = ctx.encode_jpeg_mixed(quality=95, entropy=entropy, device_ptr=lo, heights=hs, widths=ws, pitches=pt, offsets=of)
    stats = ctx.jpeg_encode_device_stats()
    assert stats["host"] == 1 and stats["device"] == 3
    assert files["device"] == files["host"]
    ks = [SIZES.index(s) for s in ((17, 17), (33, 127), (8, 512))]
    assert [files["device"][i] for i in (0, 2, 3)] == [pillow_files[(k, 95)] for k in ks]
    got = np.asarray(Image.open(io.BytesIO(files["device"][1])))
    assert got.shape == (big_h, big_w, 3) and int(got.min()) == int(got.max()) == 93


@pytest.mark.parametrize("name", ["ctpn_encode_jpeg_mixed", "ctpn_encode_jpeg_mixed_device"])
def test_capacity(ctx, pictures, pillow_files, name):
    """a file that does not fit: CTPN_ERR_CAPACITY with the size set; its neighbours are delivered; NULL with capacity 0 sizes a file"""
    fn = getattr(ctx._lib, name)
    ks = [SIZES.index(s) for s in ((17, 17), (33, 127), (8, 512))]
    imgs = [pictures[k] for k in ks]
    want = [pillow_files[(k, 95)] for k in ks]
    n = len(imgs)
    src = np.concatenate([im.reshape(-1) for im in imgs])
    hs, ws = np.array([im.shape[0] for im in imgs], np.int32), np.array([im.shape[1] for im in imgs], np.int32)
    pt = (C.c_size_t * n)(*[3 * im.shape[1] for im in imgs])
    of = (C.c_size_t * n)(*np.cumsum([0] + [im.size for im in imgs[:-1]]).tolist())
    bufs = np.full((n, 1 << 16), 0xAA, np.uint8)
    out = (C.c_void_p * n)(bufs[0].ctypes.data, bufs[1].ctypes.data, None)
    caps, sizes = (C.c_size_t * n)(1 << 16, 100, 0), (C.c_size_t * n)()
    rc = fn(ctx._h, src.ctypes.data_as(C.c_void_p), 0, src.size, n, B._ptr(hs, C.c_int), B._ptr(ws, C.c_int), pt, of, 95, out, caps, sizes)
    assert rc == B.CTPN_ERR_CAPACITY and b"too small" in ctx._lib.ctpn_last_error()
    assert [sizes[i] for i in range(n)] == [len(f) for f in want]
    assert bufs[0, : sizes[0]].tobytes() == want[0] and bufs[1, :100].tobytes() == want[1][:100] and (bufs[1, 100:] == 0xAA).all()
    caps[1] = 1 << 16
    out[2], caps[2] = bufs[2].ctypes.data, len(want[2])                                  # exactly its size
    assert fn(ctx._h, src.ctypes.data_as(C.c_void_p), 0, src.size, n, B._ptr(hs, C.c_int), B._ptr(ws, C.c_int), pt, of, 95, out, caps, sizes) == 0
    assert [bufs[i, : sizes[i]].tobytes() for i in range(n)] == want


def test_buffers_grow_and_are_reused(ctx, pictures, pillow_files, tmp_path):
    """a small call, a large call, a small call, forms alternated: every call reproduces its files"""
    small = [pictures[SIZES.index((17, 17))]]
    want_small = [pillow_files[(SIZES.index((17, 17)), 95)]]
    large = [picture(200 + 37 * k, 300 + 53 * k, 40 + k) for k in range(6)] + pictures
    want_large = [pillow_file(im, 90) for im in large]
    for entropy in ("device", "host", "device"):
        assert ctx.encode_jpeg_mixed(small, entropy=entropy) == want_small
        assert ctx.encode_jpeg_mixed(large, quality=90, entropy=entropy) == want_large
        assert ctx.encode_jpeg_mixed(small, entropy=entropy) == want_small
    # ... and the crop writer between them: one line, many lines, one line
    imgs = noise(2, 48, 80, 9)
    one = [np.array([box(3.0, 5.0, 40.0, 12.0, slant=2.0)]), np.zeros((0, 9))]
    rng = np.random.default_rng(5)
    many = [np.array([box(rng.uniform(-10, 60), rng.uniform(-5, 40), rng.uniform(2, 90), rng.uniform(3, 20), rng.uniform(-4, 4), rng.uniform(-3, 3)) for _ in range(40)])
            for _ in range(2)]
    first, _ = crop_files(ctx, tmp_path, "a", one, 32, 64, 95, "host", images=imgs)
    crops, widths = ctx.crop_lines(imgs, many, crop_h=32, max_w=128, pad_value=77)
    files, _ = crop_files(ctx, tmp_path, "b", many, 32, 128, 95, "device", images=imgs)
    assert files == [pillow_file(crops[k, :, : widths[k]]) for k in range(80)]
    third, _ = crop_files(ctx, tmp_path, "c", one, 32, 64, 95, "host", images=imgs)
    assert third == first and ctx.encode_jpeg_mixed(small) == want_small


def test_crop_writes_between_decodes_and_submits_in_flight(ctx, tmp_path):
    """the crop write of batch k stands in the copy queue behind the decode of batch k + 1 and in front of that of batch k + 2, with batch
    k + 1's forward in flight: the crop files and the decoded batches are what they are with nothing else in flight"""
    h, w, nb, n = 256, 384, 4, 3
    batches = [[encode(scene(h, w, 10 * b + i), 90, 2) for i in range(n)] for b in range(nb)]
    recs = [np.array([box(10.0 + 5 * i, 12.0, 250.0, 20.0, slant=4.0), box(-5.0, 80.0 + 7 * i, 420.0, 30.0)]) for i in range(n)]
    lone_files, lone_px = [], []
    for b, datas in enumerate(batches):
        ptr, shape = ctx.decode_jpeg_batch(datas, h, w)
        lone_px.append(ctx.jpeg_batch_fetch(ptr, shape))
        lone_files.append(crop_files(ctx, tmp_path, "lone%d" % b, recs, 32, 512, 95, "host", device_ptr=ptr, shape=shape)[0])
    pending = None

    def finish(job):
        slot, b, ptr, shape = job
        ctx.detect_collect(slot, mode="H")
        files, _ = crop_files(ctx, tmp_path, "fly%d" % b, recs, 32, 512, 95, "device" if b != 2 else "host", device_ptr=ptr, shape=shape)
        assert files == lone_files[b], b
        assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), lone_px[b]), b
    for k, datas in enumerate(batches):
        ptr, shape = ctx.decode_jpeg_batch(datas, h, w)
        ctx.detect_submit(device_ptr=ptr, shape=shape, slot=k & 1)
        if pending is not None:
            finish(pending)                                # batch k - 1's crops, behind batch k's decode
            assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), lone_px[k]), k      # ... which they left as it was
        pending = (k & 1, k, ptr, shape)
    finish(pending)


def test_errors(ctx, tmp_path, pictures):
    lib = ctx._lib
    imgs = noise(1, 48, 80, 8)
    recs = [np.array([box(3.0, 5.0, 40.0, 12.0), box(10.0, 7.0, 60.0, 9.0)])]
    for entropy, name in zip(FORMS, ("ctpn_write_line_crops", "ctpn_write_line_crops_device")):
        bad = str(tmp_path / "no" / "such" / "dir" / "line.jpg")
        with pytest.raises(B.CtpnError) as e:                                  # a path that cannot be written: its name in the message
            ctx.write_line_crops(imgs, recs, paths=[str(tmp_path / "fine.jpg"), bad], entropy=entropy)
        assert e.value.code == -1 and bad in str(e.value) and name in str(e.value)
        for q in (0, 101):
            with pytest.raises(B.CtpnError) as e:
                ctx.write_line_crops(imgs, recs, paths=[str(tmp_path / "a.jpg"), str(tmp_path / "b.jpg")], quality=q, entropy=entropy)
            assert e.value.code == -1 and "quality" in str(e.value)
        for kw in ({"crop_h": 0}, {"crop_h": 257}, {"max_w": 6}, {"max_w": 65536}, {"pad_value": 256}):      # ctpn_crop_lines' own
            with pytest.raises(B.CtpnError) as e:
                ctx.write_line_crops(imgs, recs, paths=["a", "b"], entropy=entropy, **kw)
            assert e.value.code == -1, kw
        with pytest.raises(ValueError):
            ctx.write_line_crops(imgs, recs, paths=["only-one.jpg"], entropy=entropy)
    with pytest.raises(ValueError):
        ctx.write_line_crops(imgs, recs, paths=["a", "b"], entropy="gpu")
    im = pictures[SIZES.index((17, 17))]
    for entropy, name in zip(FORMS, ("ctpn_encode_jpeg_mixed", "ctpn_encode_jpeg_mixed_device")):
        for q in (0, 101):
            with pytest.raises(B.CtpnError) as e:
                ctx.encode_jpeg_mixed([im], quality=q, entropy=entropy)
            assert e.value.code == -1 and name in str(e.value) and "quality" in str(e.value)
        t, hs, ws, pt, of = device_source([im])
        with pytest.raises(B.CtpnError) as e:                                  # a pitch below 3 w
            ctx.encode_jpeg_mixed(entropy=entropy, device_ptr=t.data_ptr(), heights=hs, widths=ws, pitches=[3 * 17 - 1], offsets=of)
        assert e.value.code == -1 and "pitch" in str(e.value)
        with pytest.raises(B.CtpnError) as e:
            ctx.encode_jpeg_mixed(entropy=entropy, device_ptr=t.data_ptr(), heights=[0], widths=ws, pitches=pt, offsets=of)
        assert e.value.code == -1
    with ctpn_amd.Context(0, 1, 64, 64, postproc_only=True) as pp:
        for entropy in FORMS:
            with pytest.raises(B.CtpnError) as e:
                pp.encode_jpeg_mixed([im], entropy=entropy)
            assert e.value.code == -3 and "post-processing-only" in str(e.value)
            with pytest.raises(B.CtpnError) as e:
                pp.write_line_crops(imgs, recs, paths=["a", "b"], entropy=entropy)
            assert e.value.code == -3 and "post-processing-only" in str(e.value)
    assert lib.ctpn_abi_version() == 10
    assert ctx.encode_jpeg_mixed([im]) == [pillow_file(im)]                    # the ctx is as usable as before


def test_demo_batch_writes_the_same_crop_files_in_all_three_forms(tmp_path, arena):
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    src = tmp_path / "in"
    src.mkdir()
    h, w = 120, 200
    for i in range(5):
        (src / ("im%02d.jpg" % i)).write_bytes(encode(scene(h, w, 50 + i), 90, 2))
    cfg.TEST.PRECISION = "bf16"
    net = get_network("VGGnet_test")
    net.load_arena(arena)
    try:
        names = demo_batch.list_images(str(src))
        dirs = {}
        for form in ("host", "gpu", "gpu-entropy"):
            out, crops_dir, logs = tmp_path / ("out-" + form), tmp_path / ("crops-" + form), []
            res = demo_batch.run(net, names, str(out), batch=3, write_images=False, log=logs.append, decode="gpu", crops_dir=str(crops_dir), crop_h=32, crops_encode=form)
            total = sum(len(res[nm]) for nm in names)
            assert "Text-line crops: %d of height 32" % total in logs[-1], logs
            dirs[form] = ({f: (crops_dir / f).read_bytes() for f in sorted(os.listdir(str(crops_dir)))}, {f: (out / f).read_bytes() for f in sorted(os.listdir(str(out)))})
            assert len(dirs[form][0]) == total > 0 and sorted(dirs[form][1]) == ["res_im%02d.txt" % i for i in range(5)]
        for form in ("gpu", "gpu-entropy"):
            assert sorted(dirs[form][0]) == sorted(dirs["host"][0])
            assert dirs[form][0] == dirs["host"][0] and dirs[form][1] == dirs["host"][1], form
        for form, kw in (("gpu", {"decode": "gpu"}), ("gpu-entropy", {"decode": "host", "crops_dir": str(tmp_path / "x")})):
            with pytest.raises(ValueError):
                demo_batch.run(net, names, str(tmp_path / "never"), batch=3, crops_encode=form, **kw)
    finally:
        net.close()
