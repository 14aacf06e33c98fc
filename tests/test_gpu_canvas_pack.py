"""GPU: ragged canvases built on the device from decoded images and PNG files (include/ctpn_hip.h: ctpn_pack_canvas,
ctpn_decode_png_files_ragged; kernel: csrc/canvas_pack.hip). Correct means EQUAL, byte for byte: rows [0, heights[i]) of slot i are
oracle/resize_ref.py's of image i by factors[i] -- which is also what ctpn_resize returns for that image alone --, every byte below is 0,
and the whole is lib/utils/blob.py im_list_to_canvas of the individually resized images.

Shapes: the cases of tests/canvas_pack_cases.py -- wc 17 .. 20 (every residue mod 4), hc 16 and 23, n 1, 2 and 5, with and without a
byte-wise tail, copies, sources 1 .. 3 pixels wide and high, the factor wc / 43. Sources: host arrays, and device images at pitches 3 w,
3 w + 1, 3 w + 7 from base pointers at byte offsets 0 .. 3, inside guard bytes. Before every case the buffer set it will get is packed full
of 255, so a zero below an image is a zero the kernel wrote; the bytes behind the canvas are read before and after.
The detector runs at tests/test_gpu_ragged.py's smallest ragged shape (w 82, canvas 96; the sizes and factors of tests/jpeg_ragged_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
from ctpn_amd.lib.utils.blob import im_list_to_canvas
from oracle import resize_ref
import canvas_pack_cases as K
import jpeg_ragged_cases as J
import util

pytestmark = pytest.mark.gpu

GUARD = 64
DIRTY = (5, 23, 20)                # the largest canvas of the cases: n, hc, wc
DEVICE_FORMS = ((0, 0), (1, 1), (7, 2), (0, 3))      # (pitch - 3 w, byte offset of the base pointer)


@pytest.fixture(scope="module")
def weights():
    return util.stress_arena("biased")


@pytest.fixture(scope="module")
def ctx(weights):
    with ctpn_amd.Context(0, 5, 96, 96, "bf16") as c:
        c.load_weights(weights)
        yield c


def on_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


_HIP = []


def device_bytes(ptr, nbytes):
    """nbytes of device memory at ptr, through the HIP runtime this process has already loaded (the caller has waited for the work)"""
    if not _HIP:
        paths = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
        assert paths, "no HIP runtime mapped"
        _HIP.append(C.CDLL(paths[0]))
        _HIP[0].hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP[0].hipMemcpy.restype = C.c_int
    out = np.empty((nbytes,), np.uint8)
    assert _HIP[0].hipMemcpy(out.ctypes.data, C.c_void_p(int(ptr)), nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def dirty(ctx):
    """the buffer set the second-next pack gets, full of 255 (a full-height batch: the kernel stores the sources as they are); then one small
    pack into the other set. -> the dirtied canvas's pointer"""
    n, hc, wc = DIRTY
    (ptr, shape), hts = ctx.pack_canvas([np.full((hc, wc, 3), 255, np.uint8)] * n, [1.0] * n, hc, wc)
    assert tuple(hts) == (hc,) * n
    ctx.pack_canvas([np.zeros((16, 17, 3), np.uint8)], [1.0], 16, 17)
    assert ctx.jpeg_batch_fetch(ptr, shape).min() == 255
    return ptr


def _code(fn, *a, **kw):
    with pytest.raises(B.CtpnError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


@pytest.fixture(scope="module")
def lone_resizes():
    """ctpn_resize of every resized source image alone: {(case, i): array}, computed once, never changed"""
    out = {}
    for name, hc, wc, imgs, _ in K.cases():
        for i, ((h, w, f), src) in enumerate(zip(imgs, K.sources(name))):
            if f != 1.0:
                out[name, i] = B.resize_linear(src, f, f)
                out[name, i].setflags(write=False)
    return out


def test_the_oracle_rows_are_ctpn_resize_of_each_image_alone(lone_resizes):
    """the definition's two right-hand sides agree: the rest of this file compares against the oracle's canvas"""
    assert len(lone_resizes) > 40
    for (name, i), got in lone_resizes.items():
        want, heights = K.expected(name)
        assert got.shape == (heights[i], want.shape[2], 3) and np.array_equal(got, want[i, :heights[i]]), (name, i)


@pytest.mark.parametrize("form", ["host", "host-strided"] + ["device-p%d-o%d" % f for f in DEVICE_FORMS])
def test_canvas_equals_the_oracle_on_every_case(ctx, form):
    extra, front = (0, 0) if form.startswith("host") else tuple(int(t[1:]) for t in form.split("-")[1:])
    for name, hc, wc, imgs, _ in K.cases():
        want, want_h = K.expected(name)
        srcs = K.sources(name)
        p_dirty = dirty(ctx)
        nbytes = want.size
        behind = device_bytes(p_dirty + nbytes, GUARD)
        if nbytes + GUARD <= int(np.prod(DIRTY)) * 3:
            assert behind.min() == 255
        bufs = []
        if form == "host":
            items = srcs
        elif form == "host-strided":                                       # rows of a wider array: the binding passes the stride as the pitch
            wide = [np.full((s.shape[0], s.shape[1] + 3, 3), 0xA5, np.uint8) for s in srcs]
            for wd, s in zip(wide, srcs):
                wd[:, : s.shape[1]] = s
            items = [wd[:, : s.shape[1]] for wd, s in zip(wide, srcs)]
        else:
            items = []
            for s in srcs:
                buf, at, pitch = K.pitched(s, extra, front=front, guard=GUARD)
                t = on_device(buf)
                assert t.data_ptr() % 4 == 0
                bufs.append((buf, t))
                items.append((t.data_ptr() + at, s.shape[:2], pitch))
                assert (t.data_ptr() + at) % 4 == front
        (ptr, shape), heights = ctx.pack_canvas(items, K.factors(name), hc, wc)
        assert ptr == p_dirty and shape == (len(imgs), hc, wc)              # the dirtied set, in turn
        assert heights.dtype == np.int32 and np.array_equal(heights, want_h)
        got = ctx.jpeg_batch_fetch(ptr, shape)
        for i, dh in enumerate(want_h):
            assert np.array_equal(got[i, :dh], want[i, :dh]), (form, name, i, np.argwhere(got[i, :dh] != want[i, :dh])[:4])
            assert not got[i, dh:].any(), (form, name, i)                   # written by the kernel: the buffer held 255
        assert np.array_equal(got, want), (form, name)
        assert np.array_equal(device_bytes(ptr + nbytes, GUARD), behind), (form, name)      # nothing behind the canvas
        for buf, t in bufs:                                                 # device sources and their guards: not a byte changed
            assert np.array_equal(t.cpu().numpy(), buf), (form, name)


def test_canvas_is_im_list_to_canvas_of_the_lone_resizes(ctx, lone_resizes):
    name = "wc19_hc23_n5"
    _, hc, wc, imgs, _ = K.case(name)
    resized = [s if f == 1.0 else lone_resizes[name, i] for i, (s, (_, _, f)) in enumerate(zip(K.sources(name), imgs))]
    canvas, hts = im_list_to_canvas(resized)
    (ptr, shape), heights = ctx.pack_canvas(K.sources(name), K.factors(name), int(canvas.shape[1]), wc)      # the canvas no taller than its tallest image
    assert np.array_equal(heights, hts) and np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), canvas)


def test_argument_errors_name_the_image_and_leave_the_previous_canvas(ctx):
    name = "wc18_hc23_n5"
    _, hc, wc, imgs, _ = K.case(name)
    want, _ = K.expected(name)
    srcs, fac = K.sources(name), K.factors(name)
    (ptr, shape), _ = ctx.pack_canvas(srcs, fac, hc, wc)
    pack = ctx.pack_canvas
    # a width that does not map to wc: image 2 at factor 1
    code, msg = _code(pack, srcs, fac[:2] + [1.0] + fac[3:], hc, wc)
    assert code == -1 and "image 2" in msg and "width" in msg and "ctpn_pack_canvas" in msg
    # heights that map to 15 and to hc + 1
    code, msg = _code(pack, srcs[:3] + [np.zeros((15, wc, 3), np.uint8)], fac[:3] + [1.0], hc, wc)
    assert code == -1 and "image 3" in msg and "maps to 15" in msg
    code, msg = _code(pack, [np.zeros((hc + 1, wc, 3), np.uint8)] + srcs[1:], [1.0] + fac[1:], hc, wc)
    assert code == -1 and "image 0" in msg and "maps to %d" % (hc + 1) in msg
    # no image, a NULL image, a pitch below 3 w
    code, msg = _code(pack, [], [], hc, wc)
    assert code == -1 and "empty batch" in msg
    t = on_device(np.zeros((hc, wc, 3), np.uint8))
    code, msg = _code(pack, [(t.data_ptr(), (hc, wc)), (0, (hc, wc))], [1.0, 1.0], hc, wc)
    assert code == -1 and "image 1" in msg and "null" in msg
    code, msg = _code(pack, [(t.data_ptr(), (hc, wc), 3 * wc - 1)], [1.0], hc, wc)
    assert code == -1 and "image 0" in msg and "pitch" in msg
    # the ctx's limits: max_batch 5, 96 x 96
    code, msg = _code(pack, [np.zeros((16, wc, 3), np.uint8)] * 6, [1.0] * 6, hc, wc)
    assert code == -1 and "exceeds" in msg
    code, msg = _code(pack, [np.zeros((97, 17, 3), np.uint8)], [1.0], 97, 17)
    assert code == -1 and "exceeds" in msg
    code, msg = _code(pack, [np.zeros((16, 97, 3), np.uint8)], [1.0], 16, 97)
    assert code == -1 and "exceeds" in msg
    assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), want)           # none of them touched the live canvas
    with ctpn_amd.Context(0, 5, 96, 96, postproc_only=True) as pp:
        code, _ = _code(pp.pack_canvas, srcs, fac, hc, wc)
        assert code == -3
        code, _ = _code(pp.decode_png_ragged, ["a.png"], [(16, 17)], [1.0], 16, 17)
        assert code == -3


def test_buffer_sets_in_turn_with_the_jpeg_calls(ctx):
    a, b, c = "wc17_hc23_n5", "wc20_hc16_n2", "wc19_hc23_n2"

    def pack(name):
        _, hc, wc, _, _ = K.case(name)
        return ctx.pack_canvas(K.sources(name), K.factors(name), hc, wc)[0]
    pa, sa = pack(a)
    pb, sb = pack(b)
    assert pa != pb
    assert np.array_equal(ctx.jpeg_batch_fetch(pa, sa), K.expected(a)[0])   # A survived B
    pc, sc = pack(c)                                                        # A's set
    assert np.array_equal(ctx.jpeg_batch_fetch(pb, sb), K.expected(b)[0])   # B survived C
    assert np.array_equal(ctx.jpeg_batch_fetch(pc, sc), K.expected(c)[0])
    # ... and in turn with a JPEG decode: the same two sets
    (pj, sj), _ = ctx.decode_jpeg_ragged(J.files(), J.SIZES, J.FACTORS, J.HC, J.WC)
    assert np.array_equal(ctx.jpeg_batch_fetch(pc, sc), K.expected(c)[0])   # C survived the decode
    pd, sd = pack(a)
    assert np.array_equal(ctx.jpeg_batch_fetch(pj, sj), J.expected()[0])    # the decoded canvas survived a pack
    assert np.array_equal(ctx.jpeg_batch_fetch(pd, sd), K.expected(a)[0])
    # a device source that is itself a live decoded canvas: slot 0 of it (96 x 82 at factor 1), waited for in the copy queue
    (pj, sj), _ = ctx.decode_jpeg_ragged(J.files(), J.SIZES, J.FACTORS, J.HC, J.WC)
    (pe, se), he = ctx.pack_canvas([(pj, (J.HC, J.WC))], [1.0], J.HC, J.WC)
    assert tuple(he) == (J.HC,) and np.array_equal(ctx.jpeg_batch_fetch(pe, se)[0], J.expected()[0][0])


def _mixed_images():
    """synthetic pictures of the file sizes of tests/jpeg_ragged_cases.py: five sizes that their factors map to 82 wide, 96 .. 16 high"""
    return [ctpn_amd.weights.synthetic_images(1, h, w, 40 + i)[0] for i, (h, w) in enumerate(J.SIZES)]


def _host_canvas(images, factors, hc):
    resized = [im if f == 1.0 else resize_ref.resize_linear(im, f, f) for im, f in zip(images, factors)]
    canvas, heights = im_list_to_canvas(resized)
    full = np.zeros((len(images), hc) + canvas.shape[2:], np.uint8)
    full[:, : canvas.shape[1]] = canvas
    return full, heights


def test_detector_on_the_packed_canvas_equals_the_host_canvas(ctx):
    images = _mixed_images()
    order2, order3 = [4, 3, 2, 1, 0], [2, 0, 4, 1, 3]
    canvas, heights = _host_canvas(images, J.FACTORS, J.HC)
    assert tuple(heights) == J.HEIGHTS
    want = {}
    for mode in "HO":
        ctx.detect_submit(canvas, slot=0, heights=heights)
        want[mode] = ctx.detect_collect(0, mode=mode, want_rois=True)
    assert sum(len(x) for x in want["H"][0]) > 0 and all(len(r) > 0 for r in want["H"][1])

    def pack(order):
        return ctx.pack_canvas([images[i] for i in order], [J.FACTORS[i] for i in order], J.HC, J.WC)
    for mode in "HO":
        # the packed canvas where it lies: bit for bit the host canvas's rois and lines
        (ptr, shape), hts = pack(range(5))
        assert np.array_equal(hts, heights)
        ctx.detect_submit(device_ptr=ptr, shape=shape, heights=hts, slot=0)
        got = ctx.detect_collect(0, mode=mode, want_rois=True)
        # the same submit with two more packs at once behind it: the second one takes the submitted canvas's buffer set
        (ptr, shape), hts = pack(range(5))
        ctx.detect_submit(device_ptr=ptr, shape=shape, heights=hts, slot=1)
        pack(order2)
        (p3, s3), _ = pack(order3)
        assert p3 == ptr
        behind = ctx.detect_collect(1, mode=mode, want_rois=True)
        for k in range(5):
            for res in (got, behind):
                assert np.array_equal(res[1][k], want[mode][1][k]) and np.array_equal(res[0][k], want[mode][0][k]), (mode, k)
        assert np.array_equal(ctx.jpeg_batch_fetch(p3, s3), canvas[order3])


def _png_files(tmp_path):
    """three file sizes; gray, RGB, RGBA and palette; written by the library's own encoder and by Pillow. -> paths, shapes, factors"""
    from PIL import Image
    rng = np.random.RandomState(7)
    a = rng.randint(0, 256, (23, 19, 3)).astype(np.uint8)                  # BGR; f = 1
    b = rng.randint(0, 256, (10, 9, 3)).astype(np.uint8)                   # RGB for Pillow; f = 19 / 9 -> 21 x 19
    c = rng.randint(0, 256, (40, 43)).astype(np.uint8)                     # gray; f = 19 / 43 -> 18 x 19
    d = rng.randint(0, 256, (10, 9, 4)).astype(np.uint8)                   # RGBA
    e = rng.randint(0, 256, (40, 43)).astype(np.uint8)                     # palette indices
    paths = [str(tmp_path / ("f%d.png" % i)) for i in range(5)]
    open(paths[0], "wb").write(B.png_encode(a))
    Image.fromarray(b).save(paths[1])
    Image.fromarray(c).save(paths[2])
    Image.fromarray(d).save(paths[3])
    pal = Image.fromarray(e).convert("P")
    pal.putpalette(rng.randint(0, 256, 768).astype(np.uint8).tobytes())
    pal.save(paths[4])
    return paths, [(23, 19), (10, 9), (40, 43), (10, 9), (40, 43)], [1.0, 19.0 / 9.0, 19.0 / 43.0, 19.0 / 9.0, 19.0 / 43.0]


def test_png_files_of_mixed_sizes_and_kinds_into_one_canvas(ctx, tmp_path):
    paths, shapes, factors = _png_files(tmp_path)
    info = B.png_probe_files(paths)
    assert [tuple(r[:2]) for r in info.tolist()] == shapes and sorted(set(info[:, 2].tolist())) == [0, 2, 3, 6]      # gray, RGB, palette, RGBA
    decoded = [B.png_decode(open(p, "rb").read()) for p in paths]
    assert [d.shape for d in decoded] == [s + (3,) for s in shapes]
    dirty(ctx)
    (ptr, shape), heights = ctx.decode_png_ragged(paths, shapes, factors, 23, 19)
    got = ctx.jpeg_batch_fetch(ptr, shape)
    want, want_h = _host_canvas(decoded, factors, 23)
    assert tuple(want_h) == (23, 21, 18, 21, 18) and np.array_equal(heights, want_h)
    assert np.array_equal(got, want)                                        # the host-built canvas
    (p2, s2), h2 = ctx.pack_canvas(decoded, factors, 23, 19)
    assert np.array_equal(h2, want_h) and np.array_equal(ctx.jpeg_batch_fetch(p2, s2), got)      # pack_canvas of ctpn_png_decode's arrays
    assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), want)           # (and the PNG canvas survived that call)


def test_png_errors_carry_the_files_index_and_code(ctx, tmp_path):
    from PIL import Image
    paths, shapes, factors = _png_files(tmp_path)
    (ptr, shape), _ = ctx.decode_png_ragged(paths, shapes, factors, 23, 19)
    want = ctx.jpeg_batch_fetch(ptr, shape)
    dec = ctx.decode_png_ragged
    # 16-bit samples: the decoder's CTPN_ERR_UNSUPPORTED, with the file's index
    deep = str(tmp_path / "deep.png")
    Image.fromarray((np.arange(23 * 19, dtype=np.uint16) * 150).reshape(23, 19)).save(deep)
    code, msg = _code(dec, paths[:1] + [deep] + paths[2:], shapes[:1] + [(23, 19)] + shapes[2:], factors[:1] + [1.0] + factors[2:], 23, 19)
    assert code == B.CTPN_ERR_UNSUPPORTED and "file 1" in msg and "ctpn_decode_png_files_ragged" in msg
    # a file of another size than announced: file 2 is 40 x 43
    code, msg = _code(dec, paths, shapes[:2] + [(41, 43)] + shapes[3:], factors, 23, 19)
    assert code == -1 and "file 2" in msg
    # a missing file, a damaged one
    code, msg = _code(dec, paths[:4] + [str(tmp_path / "none.png")], shapes, factors, 23, 19)
    assert code == -1 and "file 4" in msg and "cannot read" in msg
    data = bytearray(open(paths[0], "rb").read())
    data[len(data) // 2] ^= 0x55
    bad = str(tmp_path / "bad.png")
    open(bad, "wb").write(bytes(data))
    code, msg = _code(dec, [bad] + paths[1:], shapes, factors, 23, 19)
    assert code == -1 and "file 0" in msg
    # the argument rule is pack_canvas's, in the files' words
    code, msg = _code(dec, paths, shapes, [1.0] + factors[1:3] + [1.0] + factors[4:], 23, 19)
    assert code == -1 and "file 3" in msg and "width" in msg
    assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), want)           # one failed call took the other set at most: the canvas is intact
    (p2, s2), _ = ctx.decode_png_ragged(paths, shapes, factors, 23, 19)     # and the ctx is usable
    assert np.array_equal(ctx.jpeg_batch_fetch(p2, s2), want)


def test_demo_batch_ragged_pack_gpu_writes_the_same_result_files(weights, tmp_path):
    """a folder of PNG files of four sizes that resize_im maps to width 600 and heights 720, 720, 690, 720: res_*.txt byte-equal with the
    canvases built on the device and without the switch, where PNG files stay size-grouped"""
    from PIL import Image
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    src = tmp_path / "in"
    src.mkdir()
    for i, (h, w) in enumerate(((120, 100), (240, 200), (115, 100), (60, 50))):
        im = ctpn_amd.weights.synthetic_images(1, h, w, 50 + i)[0]
        Image.fromarray(np.ascontiguousarray(im[:, :, ::-1])).save(src / ("page%d.png" % i))
    names = demo_batch.list_images(str(src))
    assert len(names) == 4
    cfg.TEST.PRECISION = "bf16"
    outs, logs = {}, {}
    for pack in ("host", "gpu"):
        net = get_network("VGGnet_test")
        net.load_arena(weights)
        try:
            out = tmp_path / ("out_" + pack)
            log = []
            demo_batch.run(net, names, str(out), batch=4, write_images=False, log=log.append, decode="gpu", ragged=True, ragged_pack=pack)
        finally:
            net.close()
        outs[pack] = {p.name: p.read_bytes() for p in sorted(out.iterdir())}
        logs[pack] = log
    # four file sizes: four size-grouped batches without the switch, one ragged batch with it
    assert " in 4 batches " in logs["host"][0] and " in 1 batches " in logs["gpu"][0], logs
    assert "4 PNG files by the library, 0 on the host" in logs["gpu"][0], logs["gpu"]
    assert sorted(outs["gpu"]) == ["res_page%d.txt" % i for i in range(4)] and outs["gpu"] == outs["host"]
    assert any(len(v) > 0 for v in outs["gpu"].values())
