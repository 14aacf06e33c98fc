"""GPU: the device-entropy form of the JPEG writer (csrc/jpeg_huff_enc.hip) through the C ABI. Everything is exact byte equality against
the host-entropy form -- ctpn_jpeg_entropy_encode for coefficient sets, ctpn_encode_jpeg_batch / ctpn_write_annotated_files for pixels --
and against Pillow's save(quality=q, subsampling=2). (The per-thread text is pinned on the CPU first: tests/test_jpeg_huff_enc_host.py.)"""
import ctypes as C
import io
import os

import numpy as np
import pytest
from PIL import Image

import ctpn_amd
from ctpn_amd import _binding as B
from util_jpeg import encode, scene
import jpeg_huff_enc_cases as E

pytestmark = pytest.mark.gpu

CASES = E.cases()
ERR_STATE = -3


@pytest.fixture(scope="module")
def ctx(arena):
    with ctpn_amd.Context(0, 4, 256, 384, "bf16") as c:
        c.load_weights(arena)
        yield c


@pytest.fixture(scope="module")
def host_files():
    """name -> (status, bytes, message) of ctpn_jpeg_entropy_encode: computed once, shared, never changed"""
    return {k: E.host_file(c) for k, c in CASES.items()}


def pillow_file(bgr, quality=95):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


def picture(kind, h, w, seed):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return np.ascontiguousarray(scene(max(h, 8), max(w, 8), seed)[:h, :w])


def seam(ctx, names, capacities=None):
    cs = [CASES[k] for k in names]
    return B.jpeg_entropy_encode_device(ctx, [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs], capacities)


def test_the_cpu_cases_as_one_mixed_batch_equal_the_host_half(ctx, host_files):
    names = list(CASES)
    files, sizes, status = seam(ctx, names)
    message = B.load_library().ctpn_last_error().decode()
    stats = ctx.jpeg_encode_device_stats()
    for i, k in enumerate(names):
        st, data, _ = host_files[k]
        assert status[i] == st, k
        if st == 0:
            assert sizes[i] == len(data) and files[i] == data, k
        else:
            assert sizes[i] == 0 and k in E.OUT_OF_RANGE, k      # (the host call leaves its size argument as it was: 0)
    # the two out-of-range cases: the host half's status and message, and the stats say who coded what
    assert [status[names.index(k)] for k in E.OUT_OF_RANGE] == [-1, -1] and message == host_files[E.OUT_OF_RANGE[0]][2] and "outside what 8-bit baseline JPEG codes" in message
    assert stats["host"] == len(E.OUT_OF_RANGE) and stats["device"] == len(names) - len(E.OUT_OF_RANGE)
    assert stats["blocks"] == sum(CASES[k][0].size // 64 for k in names if k not in E.OUT_OF_RANGE)
    # every case alone gives the same file: nothing depends on the neighbours in the batch
    for k in ("1x1-420", "last-byte-ff", "scan-exact-422", "file-64x48-noise-q100-440"):
        f1, s1, st1 = seam(ctx, [k])
        assert st1[0] == 0 and f1[0] == host_files[k][1], k


def test_capacity_and_sizing(ctx, host_files):
    names = ["33x47-420", "ff-dense", "17x17-420", "max-block"]
    want = [host_files[k][1] for k in names]
    # out == NULL with capacity 0 sizes the file; a file that does not fit: CTPN_ERR_CAPACITY, the true size, the bytes that fit
    caps = [0, len(want[1]) - 1, len(want[2]), 100]
    files, sizes, status = seam(ctx, names, caps)
    assert list(status) == [-4, -4, 0, -4] and sizes == [len(d) for d in want]
    assert files[0] is None and files[1] == want[1][:-1] and files[2] == want[2] and files[3] == want[3][:100]
    assert "too small" in B.load_library().ctpn_last_error().decode()
    lib, n = B.load_library(), C.c_size_t(0)
    coef, l8, qt = CASES[names[3]]
    assert lib.ctpn_jpeg_entropy_encode(B._ptr(coef, C.c_int16), B._ptr(l8, C.c_int), B._ptr(qt.reshape(-1), C.c_uint16), None, 0, C.byref(n)) == -4 and n.value == sizes[3]


SIZES = [(1, 1), (15, 17), (16, 16), (17, 33), (256, 272), (600, 900)]


@pytest.mark.parametrize("quality", [1, 50, 95, 100])
def test_pixels_equal_the_host_form_and_pillow(ctx, quality):
    for k, (h, w) in enumerate(SIZES):
        for kind in ("noise", "scene"):
            img = picture(kind, h, w, 10 * k + quality)[None]
            dev = ctx.encode_jpeg_batch(img, quality=quality, entropy="device")
            assert ctx.jpeg_encode_device_stats()["device"] == 1
            assert dev == ctx.encode_jpeg_batch(img, quality=quality) and dev[0] == pillow_file(img[0], quality), (h, w, kind)
    for h, w in ((17, 33), (256, 272)):
        imgs = np.stack([picture("noise", h, w, 1), picture("scene", h, w, 2), picture("scene", h, w, 3)])
        dev = ctx.encode_jpeg_batch(imgs, quality=quality, entropy="device")
        assert ctx.jpeg_encode_device_stats()["device"] == 3 and ctx.jpeg_encode_device_stats()["host"] == 0
        assert dev == ctx.encode_jpeg_batch(imgs, quality=quality) and dev == [pillow_file(im, quality) for im in imgs], (h, w)


def lines_for(h, w, seed):
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(8):
        x1, y1 = rng.uniform(-0.1 * w, 0.8 * w), rng.uniform(-0.1 * h, 0.8 * h)
        x2, y2, s = x1 + rng.uniform(20, 0.5 * w), y1 + rng.uniform(8, 0.3 * h), rng.uniform(-5, 5)
        recs.append([x1, y1 + s, x2, y1 - s, x1, y2 + s, x2, y2 - s, rng.choice([0.95, 0.8])])
    return np.array(recs, np.float64)


@pytest.mark.parametrize("scale", [1.0, 0.625])
def test_device_inputs_and_annotated_files(ctx, tmp_path, scale):
    h, w, n = 240, 360, 4
    ptr, shape = ctx.decode_jpeg_batch([encode(scene(h, w, 30 + i), 95, 2) for i in range(n)], h, w)
    before = ctx.jpeg_batch_fetch(ptr, shape)
    dev = ctx.encode_jpeg_batch(device_ptr=ptr, shape=shape, quality=90, entropy="device")
    assert dev == ctx.encode_jpeg_batch(device_ptr=ptr, shape=shape, quality=90) and dev == [pillow_file(before[i], 90) for i in range(n)]
    recs = [lines_for(h, w, 1), np.zeros((0, 9)), lines_for(h, w, 2), lines_for(h, w, 3)[:3]]
    pd, ph = [str(tmp_path / ("d%d.jpg" % i)) for i in range(n)], [str(tmp_path / ("h%d.jpg" % i)) for i in range(n)]
    ctx.write_annotated_files(ptr, shape, recs, scale, pd, entropy="device")
    stats = ctx.jpeg_encode_device_stats()
    ctx.write_annotated_files(ptr, shape, recs, scale, ph)
    assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), before)
    sizes = 0
    for i in range(n):
        data = open(pd[i], "rb").read()
        sizes += len(data)
        assert data == open(ph[i], "rb").read() and data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9", i
    assert data != pillow_file(before[n - 1], 95)      # (lines were drawn)
    assert stats["device"] == n and stats["host"] == 0 and stats["d2h_bytes"] <= sizes + 64 * n
    with pytest.raises(B.CtpnError) as e:
        ctx.write_annotated_files(ptr, shape, recs, scale, pd[:-1] + [str(tmp_path / "no_such_dir" / "x.jpg")], entropy="device")
    assert e.value.code == -1 and "no_such_dir" in str(e.value) and "cannot open" in str(e.value)


def test_buffers_forms_and_batches_in_flight(ctx, tmp_path):
    """small, large, small; host and device forms alternated on one ctx; three decode batches in flight around the encodes"""
    small, big = np.stack([picture("scene", 33, 47, 1)]), np.stack([picture("noise" if i == 1 else "scene", 700, 1100, 2 + i) for i in range(3)])
    want_small, want_big = pillow_file(small[0]), [pillow_file(im, 90) for im in big]
    for entropy in ("device", "host", "device"):
        assert ctx.encode_jpeg_batch(small, entropy=entropy) == [want_small]
        assert ctx.encode_jpeg_batch(big, quality=90, entropy=entropy) == want_big
        assert ctx.encode_jpeg_batch(small, entropy="device") == [want_small]
    h, w, nb, n = 256, 384, 4, 3
    batches = [[encode(scene(h, w, 10 * b + i), 90, 2) for i in range(n)] for b in range(nb)]
    lone = []
    for b, datas in enumerate(batches):
        ptr, shape = ctx.decode_jpeg_batch(datas, h, w)
        recs = ctx.detect(device_ptr=ptr, shape=shape, mode="H")
        paths = [str(tmp_path / ("lone_%d_%d.jpg" % (b, i))) for i in range(n)]
        ctx.write_annotated_files(ptr, shape, recs, 1.0, paths)
        lone.append([open(p, "rb").read() for p in paths])
    pending = None

    def finish(job):
        slot, b, ptr, shape = job
        recs = ctx.detect_collect(slot, mode="H")
        paths = [str(tmp_path / ("fly_%d_%d.jpg" % (b, i))) for i in range(n)]
        ctx.write_annotated_files(ptr, shape, recs, 1.0, paths, entropy="device" if b != 2 else "host")
        for i in range(n):
            assert open(paths[i], "rb").read() == lone[b][i], (b, i)
    for k, datas in enumerate(batches):
        ptr, shape = ctx.decode_jpeg_batch(datas, h, w)
        ctx.detect_submit(device_ptr=ptr, shape=shape, slot=k & 1)
        if pending is not None:
            finish(pending)
        pending = (k & 1, k, ptr, shape)
    finish(pending)


def test_only_the_files_own_bytes_cross_to_the_host(ctx):
    """a condition on the design: result words and scan bytes, never a bound-sized buffer (the host form copies 1.66 MB per 600 x 900 image)"""
    imgs = np.stack([picture("scene", 600, 900, 5), picture("noise", 600, 900, 6), picture("scene", 600, 900, 7)])
    bound = B.jpeg_encode_capacity(600, 900)
    bufs = np.zeros((3, bound), np.uint8)
    ptrs = (C.c_void_p * 3)(*[bufs[i].ctypes.data for i in range(3)])
    caps, sizes = (C.c_size_t * 3)(bound, bound, bound), (C.c_size_t * 3)()
    assert B.load_library().ctpn_encode_jpeg_batch_device(ctx._h, imgs.ctypes.data_as(C.c_void_p), 0, 3, 600, 900, 95, ptrs, caps, sizes) == 0
    stats = ctx.jpeg_encode_device_stats()
    assert [bufs[i, : sizes[i]].tobytes() for i in range(3)] == [pillow_file(im) for im in imgs]
    assert stats["device"] == 3 and stats["blocks"] == 3 * 38 * 57 * 6 and 0 < stats["d2h_bytes"] <= sum(sizes) + 64 * 3


def test_errors(ctx, arena):
    lib = B.load_library()
    imgs = np.stack([picture("scene", 40, 56, 3)] * 2)
    for q in (0, 101):
        with pytest.raises(B.CtpnError) as e:
            ctx.encode_jpeg_batch(imgs, quality=q, entropy="device")
        assert e.value.code == -1 and "ctpn_encode_jpeg_batch_device" in str(e.value)
    bufs = np.zeros((2, 64), np.uint8)
    ptrs = (C.c_void_p * 2)(bufs[0].ctypes.data, bufs[1].ctypes.data)
    caps, sizes = (C.c_size_t * 2)(64, 64), (C.c_size_t * 2)()
    px = imgs.ctypes.data_as(C.c_void_p)
    assert lib.ctpn_encode_jpeg_batch_device(ctx._h, px, 0, 0, 40, 56, 95, ptrs, caps, sizes) == -1           # n = 0
    assert lib.ctpn_encode_jpeg_batch_device(ctx._h, None, 0, 2, 40, 56, 95, ptrs, caps, sizes) == -1
    assert lib.ctpn_encode_jpeg_batch_device(ctx._h, px, 0, 2, 40, 56, 95, None, caps, sizes) == -1
    assert lib.ctpn_encode_jpeg_batch_device(ctx._h, px, 0, 2, 40, 56, 95, ptrs, caps, None) == -1
    assert lib.ctpn_encode_jpeg_batch_device(ctx._h, px, 0, 2, 40, 56, 95, ptrs, caps, sizes) == -4            # too small: the sizes are set
    assert [sizes[0], sizes[1]] == [len(pillow_file(imgs[i])) for i in range(2)]
    assert lib.ctpn_write_annotated_files_device(ctx._h, None, 1, 8, 8, None, 0, None, 1.0, None, 95) == -1
    assert lib.ctpn_jpeg_entropy_encode_device(ctx._h, None, None, None, 1, None, None, None, None) == -1
    assert lib.ctpn_jpeg_entropy_encode_device_stats(ctx._h, None) == -1
    with pytest.raises(ValueError):
        ctx.encode_jpeg_batch(imgs, entropy="gpu")
    with ctpn_amd.Context(0, 1, 96, 160, postproc_only=True) as pp:
        with pytest.raises(B.CtpnError) as e:
            pp.encode_jpeg_batch(imgs, entropy="device")
        assert e.value.code == ERR_STATE
        with pytest.raises(B.CtpnError) as e:
            seam(pp, ["all-zero"])
        assert e.value.code == ERR_STATE and "post-processing-only" in str(e.value)
        ptr = C.c_void_p(1)      # (never dereferenced: the state is checked first)
        path = (C.c_char_p * 1)(b"x.jpg")
        cnt = np.zeros(1, np.int32)
        assert lib.ctpn_write_annotated_files_device(pp._h, ptr, 1, 8, 8, None, 0, B._ptr(cnt, C.c_int), 1.0, path, 95) == ERR_STATE


def test_demo_batch_encode_gpu_entropy_writes_encode_gpus_files(tmp_path, arena):
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    src, out_d, out_g = tmp_path / "in", tmp_path / "entropy", tmp_path / "gpu"
    src.mkdir()
    for i, (h, w) in enumerate([(300, 450), (300, 450), (600, 900), (300, 450)]):
        (src / ("im%02d.jpg" % i)).write_bytes(encode(scene(h, w, 40 + i), 90, 2))
    Image.fromarray(scene(300, 450, 99)).save(str(src / "im99.png"))
    cfg.TEST.PRECISION = "bf16"
    net = get_network("VGGnet_test")
    net.load_arena(arena)
    try:
        names = demo_batch.list_images(str(src))
        logs = []
        res_d = demo_batch.run(net, names, str(out_d), batch=3, write_images=True, log=logs.append, decode="gpu", encode="gpu-entropy")
        res_g = demo_batch.run(net, names, str(out_g), batch=3, write_images=True, log=lambda *_: None, decode="gpu", encode="gpu")
        assert "4 drawn, resized and JPEG-coded by the library" in logs[1] and "1 by the host writer" in logs[1], logs
        assert sorted(os.listdir(str(out_d))) == sorted(os.listdir(str(out_g))) and len(os.listdir(str(out_d))) == 10
        for nm in names:
            assert np.array_equal(res_d[nm], res_g[nm]), nm
        for f in sorted(os.listdir(str(out_d))):
            assert (out_d / f).read_bytes() == (out_g / f).read_bytes(), f
        with pytest.raises(ValueError):
            demo_batch.run(net, names, str(out_d), batch=3, decode="host", encode="gpu-entropy")
    finally:
        net.close()
