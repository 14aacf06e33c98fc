"""GPU: the output stages over a ragged canvas (include/ctpn_hip.h, "Ragged batches OUT") through the C ABI. Each call's result for image i
is DEFINED as the uniform call's on that image alone, so everything here is an equality of bytes: annotated files, crops, crop files. The
canvas, scales and lines are tests/out_ragged_cases.py's: 96 x 82 slots, heights (96, 80, 49, 16, 33), scales (1, 0.5, 82/123, 2, 1), lines
across and below an image's last row; a host canvas carries a sentinel in its dead rows. (The kernels' per-thread text is held to the
oracles on the CPU: tests/test_out_ragged.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import jpeg_ragged_cases as J
import out_ragged_cases as OC
from test_gpu_jpeg_encode_mixed import pillow_file
from util_jpeg import encode, scene

pytestmark = pytest.mark.gpu

FORMS = ("host", "device")


@pytest.fixture(scope="module")
def ctx(arena):
    with ctpn_amd.Context(0, 5, 96, 96, "bf16") as c:
        c.load_weights(arena)
        yield c


def on_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def read(paths):
    return [open(p, "rb").read() for p in paths]


def lone_annotated(ctx, tmp_path, tag, canvas, heights, recs, scales):
    """the definition's right-hand side: write_annotated_files of every image alone, at its own scale"""
    out = []
    for i, h in enumerate(heights):
        t = on_device(OC.lone(canvas, heights, i))
        p = str(tmp_path / ("%s_lone%d.jpg" % (tag, i)))
        ctx.write_annotated_files(t.data_ptr(), (1, int(h), canvas.shape[2]), [recs[i]], scales[i], [p])
        out.append(open(p, "rb").read())
    return out


def lone_crops(ctx, canvas, heights, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad=OC.PAD):
    """crop_lines of every image alone, concatenated in image order"""
    crops, widths = [], []
    for i in range(len(heights)):
        c, w = ctx.crop_lines(OC.lone(canvas, heights, i)[None], [recs[i]], crop_h=crop_h, max_w=max_w, pad_value=pad)
        crops.append(c)
        widths.append(w)
    return np.concatenate(crops), np.concatenate(widths)


def lone_crop_files(ctx, tmp_path, tag, canvas, heights, recs):
    out = []
    for i in range(len(heights)):
        paths = [str(tmp_path / ("%s_lone%d_%d.jpg" % (tag, i, j))) for j in range(len(recs[i]))]
        ctx.write_line_crops(OC.lone(canvas, heights, i)[None], [recs[i]], crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, paths=paths)
        out += read(paths)
    return out


@pytest.fixture(scope="module")
def want(ctx, tmp_path_factory):
    """the lone images' annotated files, crops and crop files: computed once, shared, never changed"""
    tmp = tmp_path_factory.mktemp("lone")
    canvas, heights = OC.host_canvas()
    recs = OC.recs()
    crops, widths = lone_crops(ctx, canvas, heights, recs)
    crops.setflags(write=False)
    return {"annotated": lone_annotated(ctx, tmp, "w", canvas, heights, recs, OC.SCALES), "crops": crops, "widths": widths,
            "crop_files": lone_crop_files(ctx, tmp, "w", canvas, heights, recs)}


def device_canvas(ctx, entropy="host"):
    (ptr, shape), heights = ctx.decode_jpeg_ragged(J.files(), J.SIZES, J.FACTORS, J.HC, J.WC, entropy=entropy)
    return ptr, shape, heights


def annotated(ctx, tmp_path, tag, entropy, n=5, **src):
    paths = [str(tmp_path / ("%s_%d.jpg" % (tag, i))) for i in range(n)]
    ctx.write_annotated_files_ragged(paths=paths, entropy=entropy, **src)
    return read(paths)


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("entropy", FORMS)
def test_annotated_files_equal_the_uniform_call_on_every_image_alone(ctx, want, tmp_path, entropy, source):
    canvas, heights = OC.host_canvas()                           # (the decoder's canvas holds the same images over zeros)
    recs = OC.recs()
    if source == "host":
        files = annotated(ctx, tmp_path, "h", entropy, images=canvas, heights=heights, recs=recs, scales=OC.SCALES)
    else:
        ptr, shape, hts = device_canvas(ctx)                     # live: the call waits for the decode in the copy queue
        assert np.array_equal(hts, heights)
        files = annotated(ctx, tmp_path, "d", entropy, device_ptr=ptr, shape=shape, heights=hts, recs=recs, scales=OC.SCALES)
        got = ctx.jpeg_batch_fetch(ptr, shape)
        assert all(np.array_equal(got[i, :heights[i]], canvas[i, :heights[i]]) for i in range(5))
    for i, (f, w) in enumerate(zip(files, want["annotated"])):
        assert f == w, (i, entropy, source)
    # the files' sizes: every image at its own
    from PIL import Image
    import io
    assert [Image.open(io.BytesIO(f)).size[::-1] for f in files] == [OC.out_dims(int(h), OC.WC, s) for h, s in zip(heights, OC.SCALES)]


def test_one_slot_equals_pillows_file_of_the_host_drawing_and_the_oracles_resize(ctx, want):
    from oracle import resize_ref
    canvas, heights = OC.host_canvas()
    recs = OC.recs()
    for i in (2, 4):                                              # a resized slot with lines across and below its last row; an unresized one
        img = B.draw_boxes(OC.lone(canvas, heights, i), recs[i])
        if OC.SCALES[i] != 1.0:
            img = resize_ref.resize_linear(img, 1.0 / OC.SCALES[i], 1.0 / OC.SCALES[i])
        assert want["annotated"][i] == pillow_file(img), i


def test_crops_equal_the_lone_images_crops(ctx, want):
    canvas, heights = OC.host_canvas()
    recs = OC.recs()
    crops, widths = ctx.crop_lines(canvas, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, heights=heights)
    assert np.array_equal(widths, want["widths"]) and widths.min() == 1 and widths.max() == OC.MAX_W
    assert np.array_equal(crops, want["crops"])
    ptr, shape, hts = device_canvas(ctx, "device")
    crops, widths = ctx.crop_lines(None, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, device_ptr=ptr, shape=shape, heights=hts)
    assert np.array_equal(widths, want["widths"]) and np.array_equal(crops, want["crops"])
    # ... and into a device buffer
    t = on_device(np.full(want["crops"].size, 0xEE, np.uint8))
    none, widths = ctx.crop_lines(canvas, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, heights=heights, out_device_ptr=t.data_ptr(), out_capacity=want["crops"].size)
    assert none is None and np.array_equal(t.cpu().numpy().reshape(want["crops"].shape), want["crops"])


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("entropy", FORMS)
def test_crop_files_equal_the_uniform_calls_files(ctx, want, tmp_path, entropy, source):
    canvas, heights = OC.host_canvas()
    recs = OC.recs()
    paths = [str(tmp_path / ("c_%d_%d.jpg" % (i, j))) for i in range(5) for j in range(len(recs[i]))]
    kw = {"images": canvas}
    if source == "device":
        ptr, shape, _ = device_canvas(ctx)
        kw = {"device_ptr": ptr, "shape": shape}
    widths = ctx.write_line_crops(recs=recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, paths=paths, entropy=entropy, heights=heights, **kw)
    assert np.array_equal(widths, want["widths"])
    assert read(paths) == want["crop_files"]                      # image 0's lines, then image 1's (none), ...: the same order, the same bytes
    assert want["crop_files"][0] == pillow_file(want["crops"][0, :, : want["widths"][0]])


def raw_crops(ctx, name, canvas, heights, packed, counts, out, capacity, paths, widths, total):
    n, hc, w = canvas.shape[:3]
    head = (ctx._h, canvas.ctypes.data_as(C.c_void_p), 0, n, hc, w, B._ptr(heights, C.c_int), B._ptr(packed, C.c_double), packed.shape[1], B._ptr(counts, C.c_int),
            OC.CROP_H, OC.MAX_W, OC.PAD)
    if name == "ctpn_crop_lines_ragged":
        return ctx._lib.ctpn_crop_lines_ragged(*head, None if out is None else out.ctypes.data_as(C.c_void_p), 0, capacity, B._ptr(widths, C.c_int), C.byref(total))
    keep, arr = (None, None) if paths is None else B._path_array(paths)
    return getattr(ctx._lib, name)(*head, 95, arr, B._ptr(widths, C.c_int), C.byref(total))


def test_sizing_forms_and_the_empty_call(ctx, want, tmp_path):
    canvas, heights = OC.host_canvas()
    packed, counts = B._pack_lines(OC.recs(), None, 5)
    lines = int(counts.sum())
    need = want["crops"].size
    for name in ("ctpn_crop_lines_ragged", "ctpn_write_line_crops_ragged", "ctpn_write_line_crops_ragged_device"):
        widths, total = np.full(lines, -1, np.int32), C.c_int(-1)
        assert raw_crops(ctx, name, canvas, heights, packed, counts, None, 0, None, widths, total) == 0      # sizes the call
        assert total.value == lines and np.array_equal(widths, want["widths"]), name
        total.value = -1                                          # no lines at all: fine, nothing written
        paths = [str(tmp_path / ("never_%d.jpg" % k)) for k in range(lines)]
        out = np.full(need, 0xAB, np.uint8)
        assert raw_crops(ctx, name, canvas, heights, packed, np.zeros(5, np.int32), out, need, paths, widths, total) == 0 and total.value == 0
        assert (out == 0xAB).all() and not any(os.path.exists(p) for p in paths)
    out, total = np.full(need, 0xAB, np.uint8), C.c_int(-1)
    assert raw_crops(ctx, "ctpn_crop_lines_ragged", canvas, heights, packed, counts, out, need - 1, None, widths, total) == B.CTPN_ERR_CAPACITY
    assert total.value == lines and (out == 0xAB).all() and b"need" in ctx._lib.ctpn_last_error()
    assert raw_crops(ctx, "ctpn_crop_lines_ragged", canvas, heights, packed, counts, out, need, None, widths, total) == 0
    assert np.array_equal(out.reshape(want["crops"].shape), want["crops"])


def test_full_height_slots_and_equal_scales_give_the_uniform_calls_files(ctx, tmp_path):
    """the degenerate case: every height equal to hc, every scale equal -- the uniform calls on the same batch write the same files"""
    imgs = np.stack([np.ascontiguousarray(scene(48, 82, 60 + i)[:, :, ::-1]) for i in range(3)])
    recs = [np.array([OC.line(10.0, 20.0, 60.0, 12.0, 0.95, slant=2.0)]), np.zeros((0, 9)), np.array([OC.line(4.0, 30.0, 70.0, 25.0, 0.5), OC.line(30.0, 5.0, 40.0, 9.0, 0.93)])]
    heights = [48, 48, 48]
    t = on_device(imgs)
    for scale in (1.0, 82.0 / 123.0):
        u = [str(tmp_path / ("u%d_%g.jpg" % (i, scale))) for i in range(3)]
        ctx.write_annotated_files(t.data_ptr(), (3, 48, 82), recs, scale, u)
        for entropy in FORMS:
            assert annotated(ctx, tmp_path, "r%s%g" % (entropy, scale), entropy, n=3, device_ptr=t.data_ptr(), shape=(3, 48, 82), heights=heights, recs=recs,
                             scales=[scale] * 3) == read(u), (scale, entropy)
    crops, widths = ctx.crop_lines(imgs, recs, crop_h=16, max_w=64, pad_value=3)
    rc, rw = ctx.crop_lines(imgs, recs, crop_h=16, max_w=64, pad_value=3, heights=heights)
    assert np.array_equal(rw, widths) and np.array_equal(rc, crops)
    up = [str(tmp_path / ("uc%d.jpg" % k)) for k in range(3)]
    rp = [str(tmp_path / ("rc%d.jpg" % k)) for k in range(3)]
    ctx.write_line_crops(imgs, recs, crop_h=16, max_w=64, pad_value=3, paths=up)
    ctx.write_line_crops(imgs, recs, crop_h=16, max_w=64, pad_value=3, paths=rp, heights=heights, entropy="device")
    assert read(up) == read(rp)


def test_the_callers_canvas_is_not_modified(ctx, tmp_path):
    canvas, heights = OC.host_canvas()
    keep = canvas.copy()
    t = on_device(canvas)                                         # a device canvas WITH the sentinel rows
    recs = OC.recs()
    for entropy in FORMS:
        annotated(ctx, tmp_path, "m" + entropy, entropy, device_ptr=t.data_ptr(), shape=canvas.shape[:3], heights=heights, recs=recs, scales=OC.SCALES)
        annotated(ctx, tmp_path, "mh" + entropy, entropy, images=canvas, heights=heights, recs=recs, scales=OC.SCALES)
    ctx.crop_lines(None, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, device_ptr=t.data_ptr(), shape=canvas.shape[:3], heights=heights)
    assert np.array_equal(t.cpu().numpy(), keep) and np.array_equal(canvas, keep)
    ptr, shape, hts = device_canvas(ctx)
    before = ctx.jpeg_batch_fetch(ptr, shape)
    annotated(ctx, tmp_path, "live", "host", device_ptr=ptr, shape=shape, heights=hts, recs=recs, scales=OC.SCALES)
    assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), before)


ORDERS = ((0, 1, 2, 3, 4), (4, 3, 2, 1, 0), (2, 0, 4, 1, 3), (1, 3, 0, 2, 4))


def test_writes_between_ragged_decodes_and_submits_in_flight(ctx, tmp_path):
    """the writer and crop calls of batch k stand in the copy queue behind the ragged decode of batch k + 1 and in front of that of batch
    k + 2, with batch k + 1's forward in flight: detections, files and canvases are what they are with nothing else in flight"""
    files, all_recs = J.files(), OC.recs()

    def decode(order):
        (ptr, shape), hts = ctx.decode_jpeg_ragged([files[i] for i in order], [J.SIZES[i] for i in order], [J.FACTORS[i] for i in order], J.HC, J.WC)
        return ptr, shape, hts

    def outputs(tag, b, ptr, shape, hts):
        order = ORDERS[b]
        recs, scales = [all_recs[i] for i in order], [OC.SCALES[i] for i in order]
        ann = annotated(ctx, tmp_path, "%s%d" % (tag, b), "device" if b & 1 else "host", device_ptr=ptr, shape=shape, heights=hts, recs=recs, scales=scales)
        paths = [str(tmp_path / ("%s%d_c%d.jpg" % (tag, b, k))) for k in range(sum(len(r) for r in recs))]
        ctx.write_line_crops(recs=recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, device_ptr=ptr, shape=shape, paths=paths, heights=hts,
                             entropy="host" if b & 1 else "device")
        crops = ctx.crop_lines(None, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, device_ptr=ptr, shape=shape, heights=hts)[0]
        return ann, read(paths), crops

    import time
    t_start = time.time()
    quiet = []
    for b, order in enumerate(ORDERS):
        ptr, shape, hts = decode(order)
        px = ctx.jpeg_batch_fetch(ptr, shape)
        ctx.detect_submit(device_ptr=ptr, shape=shape, heights=hts, slot=0)
        lines = ctx.detect_collect(0, mode="H")
        quiet.append((px, lines, outputs("quiet", b, ptr, shape, hts)))
    pending = None

    def finish(job):
        slot, b, ptr, shape, hts = job
        lines = ctx.detect_collect(slot, mode="H")
        assert len(lines) == 5 and all(np.array_equal(a, q) for a, q in zip(lines, quiet[b][1])), b
        ann, crop_files, crops = outputs("fly", b, ptr, shape, hts)
        assert ann == quiet[b][2][0] and crop_files == quiet[b][2][1] and np.array_equal(crops, quiet[b][2][2]), b
        assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), quiet[b][0]), b
    for k, order in enumerate(ORDERS):
        ptr, shape, hts = decode(order)
        ctx.detect_submit(device_ptr=ptr, shape=shape, heights=hts, slot=k & 1)
        if pending is not None:
            finish(pending)                                       # batch k - 1's files, behind batch k's decode
            assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), quiet[k][0]), k      # ... which they left as it was
        pending = (k & 1, k, ptr, shape, hts)
    finish(pending)
    print("in-flight test: %.3f s wall, lines per image of batch 0: %s, annotated sizes %s, crop files %d" % (
        time.time() - t_start, [len(x) for x in quiet[0][1]], [len(f) for f in quiet[0][2][0]], len(quiet[0][2][1])))


def test_buffers_grow_and_are_reused(ctx, want, tmp_path):
    small = np.ascontiguousarray(scene(32, 24, 5)[None, :, :, ::-1])
    small_recs = [np.array([OC.line(2.0, 12.0, 18.0, 9.0, 0.95)])]

    def small_call(tag):
        f = annotated(ctx, tmp_path, tag, "device", n=1, images=small, heights=[20], recs=small_recs, scales=[0.75])
        c = ctx.crop_lines(small, small_recs, crop_h=8, max_w=32, heights=[20])[0]
        p = [str(tmp_path / (tag + "_crop.jpg"))]
        ctx.write_line_crops(small, small_recs, crop_h=8, max_w=32, paths=p, heights=[20])
        return f, c, read(p)
    first = small_call("s1")
    canvas, heights = OC.host_canvas()
    big_scales = [0.25, 0.25, 0.3, 0.2, 0.25]                     # 384 x 328 and more out of 96 x 82: every buffer grows
    big = annotated(ctx, tmp_path, "big", "host", images=canvas, heights=heights, recs=OC.recs(), scales=big_scales)
    assert big == lone_annotated(ctx, tmp_path, "big", canvas, heights, OC.recs(), big_scales)
    crops, widths = ctx.crop_lines(canvas, OC.recs(), crop_h=64, max_w=512, pad_value=OC.PAD, heights=heights)
    lc, lw = lone_crops(ctx, canvas, heights, OC.recs(), 64, 512)
    assert np.array_equal(widths, lw) and np.array_equal(crops, lc)
    third = small_call("s3")
    assert third[0] == first[0] and np.array_equal(third[1], first[1]) and third[2] == first[2]
    t = on_device(small[0, :20])
    p = str(tmp_path / "small_lone.jpg")
    ctx.write_annotated_files(t.data_ptr(), (1, 20, 24), small_recs, 0.75, [p])
    assert first[0] == read([p])


def test_errors(ctx, tmp_path):
    canvas, heights = OC.host_canvas()
    recs = OC.recs()
    paths = [str(tmp_path / ("e%d.jpg" % i)) for i in range(5)]
    crop_paths = [str(tmp_path / ("ec%d.jpg" % k)) for k in range(sum(len(r) for r in recs))]
    names = {"host": "ctpn_write_annotated_files_ragged", "device": "ctpn_write_annotated_files_ragged_device"}
    for entropy in FORMS:
        def ann(**kw):
            args = dict(images=canvas, heights=heights, recs=recs, scales=OC.SCALES, paths=paths, entropy=entropy)
            args.update(kw)
            ctx.write_annotated_files_ragged(**args)
        for h, text in ((15, "image 3: height 15 outside 16 .. 96"), (97, "image 3: height 97 outside 16 .. 96")):
            bad = np.array(heights)
            bad[3] = h
            with pytest.raises(B.CtpnError) as e:
                ann(heights=bad)
            assert e.value.code == -1 and text in str(e.value) and names[entropy] in str(e.value)
            for call in (lambda: ctx.crop_lines(canvas, recs, heights=bad), lambda: ctx.write_line_crops(canvas, recs, paths=crop_paths, heights=bad, entropy=entropy)):
                with pytest.raises(B.CtpnError) as e:
                    call()
                assert e.value.code == -1 and text in str(e.value)
        for s in (0.0, float("nan")):
            with pytest.raises(B.CtpnError) as e:
                ann(scales=[1.0, s, 1.0, 1.0, 1.0])
            assert e.value.code == -1 and "image 1: the scale is not finite and positive" in str(e.value)
        with pytest.raises(B.CtpnError) as e:                     # 82 / 0.00125 = 65600 columns
            ann(scales=[1.0, 1.0, 0.00125, 1.0, 1.0])
        assert e.value.code == -1 and "image 2: the resized image is empty or too large" in str(e.value)
        for q in (0, 101):
            with pytest.raises(B.CtpnError) as e:
                ann(quality=q)
            assert e.value.code == -1 and "quality" in str(e.value)
            with pytest.raises(B.CtpnError) as e:
                ctx.write_line_crops(canvas, recs, paths=crop_paths, heights=heights, quality=q, entropy=entropy)
            assert e.value.code == -1 and "quality" in str(e.value)
        bad = str(tmp_path / "no" / "such" / "dir" / "page.jpg")
        with pytest.raises(B.CtpnError) as e:                     # a path that cannot be written: its name in the message
            ann(paths=paths[:3] + [bad] + paths[4:])
        assert e.value.code == -1 and bad in str(e.value) and names[entropy] in str(e.value)
        with pytest.raises(B.CtpnError) as e:
            ctx.write_line_crops(canvas, recs, paths=crop_paths[:-1] + [bad], heights=heights, entropy=entropy)
        assert e.value.code == -1 and bad in str(e.value) and "ctpn_write_line_crops_ragged" in str(e.value)
        with pytest.raises(ValueError):
            ann(scales=OC.SCALES[:4])
    with ctpn_amd.Context(0, 1, 96, 96, postproc_only=True) as pp:
        for entropy in FORMS:
            with pytest.raises(B.CtpnError) as e:
                pp.write_annotated_files_ragged(images=canvas, heights=heights, recs=recs, scales=OC.SCALES, paths=paths, entropy=entropy)
            assert e.value.code == -3 and "post-processing-only" in str(e.value)
            with pytest.raises(B.CtpnError) as e:
                pp.write_line_crops(canvas, recs, paths=crop_paths, heights=heights, entropy=entropy)
            assert e.value.code == -3 and "post-processing-only" in str(e.value)
        with pytest.raises(B.CtpnError) as e:
            pp.crop_lines(canvas, recs, heights=heights)
        assert e.value.code == -3
    assert ctx._lib.ctpn_abi_version() == 10
    assert len(ctx.crop_lines(canvas, recs, crop_h=8, max_w=32, heights=heights)[1]) == len(crop_paths)      # the ctx is as usable as before


@pytest.mark.parametrize("form", ["gpu", "gpu-entropy"])
def test_demo_batch_ragged_outputs_writes_the_files_of_the_uniform_run(tmp_path, arena, form):
    """five files of five sizes that resize_im maps to width 600 and five heights, plus two of one size: --ragged --ragged-outputs with the
    library's writers writes the res files, annotated images and crop files of the same options without them: names and bytes"""
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    src = tmp_path / "in"
    src.mkdir()
    sizes = [(120, 100), (110, 100), (115, 100), (240, 200), (100, 100), (130, 100), (130, 100)]      # -> 720, 660, 690, 720, 600, 780, 780 rows of 600
    for i, (h, w) in enumerate(sizes):
        (src / ("im%02d.jpg" % i)).write_bytes(encode(scene(h, w, 50 + i), 90, 2 if i % 2 or i >= 5 else 0))      # (two layouts among the five; the pair shares one)
    cfg.TEST.PRECISION = "bf16"
    net = get_network("VGGnet_test")
    net.load_arena(arena)
    try:
        names = demo_batch.list_images(str(src))
        got = {}
        for ragged in (False, True):
            out, crops_dir, logs = tmp_path / ("out%d" % ragged), tmp_path / ("crops%d" % ragged), []
            res = demo_batch.run(net, names, str(out), batch=4, write_images=True, log=logs.append, decode=form, encode=form, crops_dir=str(crops_dir), crop_h=32,
                                 crops_encode=form, ragged=ragged, ragged_outputs=ragged)
            total = sum(len(res[nm]) for nm in names)
            print("ragged=%s form=%s: %d lines, logs: %s" % (ragged, form, total, logs))
            got[ragged] = ({f: (crops_dir / f).read_bytes() for f in sorted(os.listdir(str(crops_dir)))}, {f: (out / f).read_bytes() for f in sorted(os.listdir(str(out)))},
                           int(logs[0].split(" images in ")[1].split(" batches")[0]))
            assert len(got[ragged][0]) == total > 0, logs        # at least one crop file: the comparison is not empty
            assert "7 drawn, resized and JPEG-coded by the library (device + C++ pool), 0 by the host writer" in logs[1], logs
        print("crop files %d, out files %s" % (len(got[True][0]), {k: len(v) for k, v in got[True][1].items()}))
        assert got[False][2] == 6 and got[True][2] == 2          # six file sizes; across heights 780, 780, 720, 720 | 690, 660, 600
        assert sorted(got[True][1]) == sorted(["res_im%02d.txt" % i for i in range(7)] + ["im%02d.jpg" % i for i in range(7)])
        assert sorted(got[True][0]) == sorted(got[False][0]) and sorted(got[True][1]) == sorted(got[False][1])
        assert got[True][0] == got[False][0] and got[True][1] == got[False][1]
    finally:
        net.close()
