"""GPU: the PNG writer's table form behind the C ABI (csrc/png_enc.hip over the one-dimensional work-item grid, api_png_out.hip
png_code_table): ctpn_encode_png_mixed, ctpn_write_annotated_png_files_ragged, ctpn_write_line_crops_png[_ragged] and demo_batch's
crops_format / ragged_png. Everything is an equality of bytes: file i of a table is the host form's file of image i (ctpn_png_encode),
a ragged canvas's file i is the uniform writer's file of image i alone, crop file k is the host form's file of crop_lines' crop k.
(The item walk, the pitched read and the passes are pinned on the CPU from the kernels' source text: tests/test_png_encode_mixed.py.)"""
import ctypes as C
import io
import os

import numpy as np
import pytest
from PIL import Image

import ctpn_amd
from ctpn_amd import _binding as B
import jpeg_ragged_cases as J
import out_ragged_cases as OC
import png_enc_ref as R
from util_jpeg import encode, scene

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE


@pytest.fixture(scope="module")
def ctx(arena):
    with ctpn_amd.Context(0, 5, 256, 384, "bf16") as c:      # (five slots: the ragged canvas of tests/out_ragged_cases.py)
        c.load_weights(arena)
        yield c


def pillow_bgr(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1]


def on_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def read(paths):
    return [open(p, "rb").read() for p in paths]


def pieces(im):
    return (R.stream_bytes(*im.shape[:2]) + 255) // 256


def pitched(imgs):
    """one source block of exactly the images' size, back to back, every second image at a pitch wider than 3 w, the pads a sentinel
    -> (block, heights, widths, pitches, offsets)"""
    hs, ws = [im.shape[0] for im in imgs], [im.shape[1] for im in imgs]
    pitches = [3 * w + (1 + k % 7 if k & 1 else 0) for k, w in enumerate(ws)]
    offsets, at = [], 0
    for h, w, p in zip(hs, ws, pitches):
        offsets.append(at)
        at += (h - 1) * p + 3 * w
    block = np.full(at, SENTINEL, np.uint8)
    for im, p, o in zip(imgs, pitches, offsets):
        h, w = im.shape[:2]
        for y in range(h):
            block[o + y * p: o + y * p + 3 * w] = im[y].reshape(-1)
    return block, hs, ws, pitches, offsets


def check(files, imgs):
    assert len(files) == len(imgs)
    for i, (f, im) in enumerate(zip(files, imgs)):
        assert f == B.png_encode(im), (i, im.shape, len(f))
        assert np.array_equal(pillow_bgr(f), im), (i, im.shape)


def check_stats(ctx, files, imgs):
    st, n = ctx.png_encode_device_stats(), len(imgs)
    assert st["device"] == n and st["host"] == 0 and st["pieces"] == sum(pieces(im) for im in imgs), st
    assert st["d2h_bytes"] <= sum(len(f) for f in files) + 16 * n + 1144 * n, st      # a condition: histograms, records, the files' own bytes


@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_the_cpu_set_as_one_table(ctx, order):
    imgs = list(R.images().values())
    if order == "reversed":
        imgs = imgs[::-1]
    files = ctx.encode_png_mixed(imgs)                             # a host source: copied in the copy queue
    check(files, imgs)
    check_stats(ctx, files, imgs)
    block, hs, ws, pitches, offsets = pitched(imgs)                # a device source of exactly the images' bytes, odd pitches and alignments
    t = on_device(block)
    again = ctx.encode_png_mixed(device_ptr=t.data_ptr(), heights=hs, widths=ws, pitches=pitches, offsets=offsets)
    assert again == files
    check_stats(ctx, again, imgs)
    assert np.array_equal(t.cpu().numpy(), block)


def test_a_live_batch_of_the_jpeg_decoder_as_a_table(ctx):
    datas = [encode(scene(48, 80, 5 + i), 92, 2) for i in range(3)]
    ptr, shape = ctx.decode_jpeg_batch(datas, 48, 80)
    n, h, w = shape
    files = ctx.encode_png_mixed(device_ptr=ptr, heights=[h] * n, widths=[w] * n, pitches=[3 * w] * n, offsets=[i * h * w * 3 for i in range(n)])
    assert files == ctx.encode_png_batch(device_ptr=ptr, shape=shape)
    check(files, ctx.jpeg_batch_fetch(ptr, shape))


def test_growing_and_shrinking_tables_alternating_with_the_other_writers(ctx):
    rng = np.random.default_rng(8)
    shapes = [[(9, 11)], [(64, 96), (3, 28)], [(200, 300), (2, 10923), (64, 96), (1, 85)], [(64, 96)], [(9, 11), (130, 70), (40, 700)]]
    for k, table in enumerate(shapes):
        imgs = [R.document_page(h, w, seed=k + j) if h >= 40 and w >= 40 else rng.integers(0, 3, (h, w, 3), dtype=np.uint8) for j, (h, w) in enumerate(table)]
        check(ctx.encode_png_mixed(imgs), imgs)
        check(ctx.encode_png_batch(imgs[0][None]), imgs[:1])
        jf = ctx.encode_jpeg_mixed(imgs[:1], quality=90)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(imgs[0][:, :, ::-1])).save(buf, "JPEG", quality=90, subsampling=2)
        assert jf[0] == buf.getvalue()
    imgs = [R.flat(96, 128), rng.integers(0, 256, (33, 57, 3), dtype=np.uint8), R.document_page(96, 128, seed=2)]
    first = ctx.encode_png_mixed(imgs)
    for _ in range(3):                                             # four identical calls back to back
        assert ctx.encode_png_mixed(imgs) == first
    check(first, imgs)


def raw_mixed(ctx, h_ctx, imgs, caps, null_out=False):
    n = len(imgs)
    src = np.concatenate([im.reshape(-1) for im in imgs])
    hs, ws = np.array([im.shape[0] for im in imgs], np.int32), np.array([im.shape[1] for im in imgs], np.int32)
    pt = (C.c_size_t * n)(*[3 * int(w) for w in ws])
    of = (C.c_size_t * n)(*[int(v) for v in np.cumsum([0] + [im.size for im in imgs])[:-1]])
    bufs = [np.full(max(c, 1), 0xAB, np.uint8) for c in caps]
    out = (C.c_void_p * n)(*[None if null_out else b.ctypes.data for b in bufs])
    cp, sizes = (C.c_size_t * n)(*caps), (C.c_size_t * n)()
    rc = ctx._lib.ctpn_encode_png_mixed(h_ctx, src.ctypes.data_as(C.c_void_p), 0, src.size, n, B._ptr(hs, C.c_int), B._ptr(ws, C.c_int), pt, of, out, cp, sizes)
    return rc, list(sizes), bufs


def test_sizing_capacity_and_state(ctx, tmp_path):
    imgs = [R.document_page(40, 60, seed=1), R.flat(7, 9)]
    want = [B.png_encode(im) for im in imgs]
    rc, sizes, _ = raw_mixed(ctx, ctx._h, imgs, [0, 0], null_out=True)      # the sizing call
    assert rc == B.CTPN_ERR_CAPACITY and sizes == [len(f) for f in want]
    rc, sizes, bufs = raw_mixed(ctx, ctx._h, imgs, [len(want[0]) - 1, len(want[1])])
    assert rc == B.CTPN_ERR_CAPACITY and sizes == [len(f) for f in want] and (bufs[0] == 0xAB).all() and bufs[1].tobytes() == want[1]
    caps = [B.png_encode_capacity(*im.shape[:2]) for im in imgs]             # ... always fits
    rc, sizes, bufs = raw_mixed(ctx, ctx._h, imgs, caps)
    assert rc == 0 and [b[:s].tobytes() for b, s in zip(bufs, sizes)] == want
    canvas, heights = OC.host_canvas()
    recs = OC.recs()
    crop_paths = [str(tmp_path / ("c%d.png" % k)) for k in range(sum(len(r) for r in recs))]
    with ctpn_amd.Context(0, 1, 96, 96, postproc_only=True) as pp:
        rc, _, _ = raw_mixed(ctx, pp._h, imgs, caps)
        assert rc == -3 and b"post-processing-only" in ctx._lib.ctpn_last_error()
        with pytest.raises(B.CtpnError) as e:
            pp.write_annotated_png_files_ragged(images=canvas, heights=heights, recs=recs, scales=OC.SCALES, paths=[str(tmp_path / ("p%d.png" % i)) for i in range(5)])
        assert e.value.code == -3
        for hts in (None, heights):
            with pytest.raises(B.CtpnError) as e:
                pp.write_line_crops(canvas, recs, paths=crop_paths, heights=hts, format="png")
            assert e.value.code == -3
    bad = str(tmp_path / "no-such-directory" / "x.png")                      # an unwritable path: its name in the message
    with pytest.raises(B.CtpnError) as e:
        ctx.write_annotated_png_files_ragged(images=canvas, heights=heights, recs=recs, scales=OC.SCALES, paths=[str(tmp_path / ("q%d.png" % i)) for i in range(4)] + [bad])
    assert e.value.code == -1 and bad in ctx._lib.ctpn_last_error().decode() and "ctpn_write_annotated_png_files_ragged" in str(e.value)
    with pytest.raises(B.CtpnError) as e:
        ctx.write_line_crops(canvas, recs, paths=crop_paths[:-1] + [bad], heights=heights, format="png")
    assert e.value.code == -1 and bad in str(e.value) and "ctpn_write_line_crops_png_ragged" in str(e.value)
    with pytest.raises(ValueError):
        ctx.write_line_crops(canvas, recs, paths=crop_paths, heights=heights, format="png", entropy="device")
    check(ctx.encode_png_mixed(imgs), imgs)                                  # the ctx is as usable as before


@pytest.fixture(scope="module")
def lone(ctx, tmp_path_factory):
    """the definitions' right-hand sides, computed once: write_annotated_png_files of every image alone; crop_lines of the canvas"""
    tmp = tmp_path_factory.mktemp("lone_png")
    canvas, heights = OC.host_canvas()
    recs = OC.recs()
    files = []
    for i, h in enumerate(heights):
        p = str(tmp / ("lone%d.png" % i))
        ctx.write_annotated_png_files(images=OC.lone(canvas, heights, i)[None], recs=[recs[i]], scale=OC.SCALES[i], paths=[p])
        files += read([p])
    crops, widths = ctx.crop_lines(canvas, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, heights=heights)
    crops.setflags(write=False)
    return {"annotated": files, "crops": crops, "widths": widths}


@pytest.mark.parametrize("source", ["host", "device"])
def test_ragged_annotated_png_files_equal_the_uniform_call_on_every_image_alone(ctx, lone, tmp_path, source):
    canvas, heights = OC.host_canvas()                             # 0xAB in the dead rows: a read below an image changes bytes
    recs = OC.recs()
    paths = [str(tmp_path / ("%s%d.png" % (source, i))) for i in range(5)]
    if source == "host":
        keep = canvas.copy()
        ctx.write_annotated_png_files_ragged(images=canvas, heights=heights, recs=recs, scales=OC.SCALES, paths=paths)
        assert np.array_equal(canvas, keep)
    else:                                                          # the live canvas of the ragged decoder: the call waits for it in the copy queue
        (ptr, shape), hts = ctx.decode_jpeg_ragged(J.files(), J.SIZES, J.FACTORS, J.HC, J.WC)
        assert np.array_equal(hts, heights)
        ctx.write_annotated_png_files_ragged(device_ptr=ptr, shape=shape, heights=hts, recs=recs, scales=OC.SCALES, paths=paths)
        got = ctx.jpeg_batch_fetch(ptr, shape)
        assert all(np.array_equal(got[i, :heights[i]], canvas[i, :heights[i]]) for i in range(5))
    files = read(paths)
    for i, (f, w) in enumerate(zip(files, lone["annotated"])):
        assert f == w, (i, source)
    dims = [OC.out_dims(int(h), OC.WC, s) for h, s in zip(heights, OC.SCALES)]
    assert dims[1] == (160, 164) and dims[3] == (8, 41) and dims[4] == (33, 82) and OC.SCALES[4] == 1.0      # two groups; the smallest; scale 1 behind resized ones
    assert (R.stream_bytes(160, 164) + 255) // 256 == 309
    assert [Image.open(io.BytesIO(f)).size[::-1] for f in files] == dims
    st = ctx.png_encode_device_stats()
    assert st["device"] == 5 and st["host"] == 0 and st["pieces"] == sum((R.stream_bytes(h, w) + 255) // 256 for h, w in dims)
    img = B.draw_boxes(OC.lone(canvas, heights, 4), recs[4])      # an unresized slot: the host form of the host drawing
    assert files[4] == B.png_encode(img)


def test_a_shuffled_canvas_gives_the_same_file_per_image(ctx, lone, tmp_path):
    order = (2, 0, 4, 1, 3)
    canvas, heights = OC.host_canvas(order)
    recs = OC.recs()
    paths = [str(tmp_path / ("s%d.png" % i)) for i in range(5)]
    ctx.write_annotated_png_files_ragged(images=canvas, heights=heights, recs=[recs[i] for i in order], scales=[OC.SCALES[i] for i in order], paths=paths)
    assert read(paths) == [lone["annotated"][i] for i in order]


@pytest.mark.parametrize("ragged", [False, True])
def test_png_crop_files_are_the_host_forms_files_of_the_crops(ctx, lone, tmp_path, ragged):
    canvas, heights = OC.host_canvas()
    recs = OC.recs()
    if ragged:
        images, hts, crops, widths = canvas, heights, lone["crops"], lone["widths"]
    else:                                                          # a uniform batch: the full-height slots of the canvas
        images, hts = canvas[[0]], None
        recs = recs[:1]
        crops, widths = ctx.crop_lines(images, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD)
    lines = sum(len(r) for r in recs)
    paths = [str(tmp_path / ("c%d_%d.png" % (ragged, k))) for k in range(lines)]
    got = ctx.write_line_crops(images, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, paths=paths, heights=hts, format="png")
    assert np.array_equal(got, widths) and len(widths) == lines
    files = read(paths)
    for k, f in enumerate(files):
        assert f == B.png_encode(np.ascontiguousarray(crops[k, :, :widths[k]])), k
        px = pillow_bgr(f)
        assert px.shape == (OC.CROP_H, widths[k], 3) and np.array_equal(px, crops[k, :, :widths[k]])
    if ragged:                                                     # (some crop is narrower than max_w: its pad columns exist, and stay out)
        assert widths.min() < OC.MAX_W and (crops[int(np.argmin(widths)), :, widths.min():] == OC.PAD).all()
    # total, widths and the sizing form: the JPEG call's
    jp = [str(tmp_path / ("j%d_%d.jpg" % (ragged, k))) for k in range(lines)]
    assert np.array_equal(ctx.write_line_crops(images, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, paths=jp, heights=hts), got)
    for fmt in ("jpg", "png"):
        assert np.array_equal(ctx.write_line_crops(images, recs, crop_h=OC.CROP_H, max_w=OC.MAX_W, pad_value=OC.PAD, paths=None, heights=hts, format=fmt), got)
    none = [np.zeros((0, 9))] * len(recs)                          # no lines: fine, nothing written
    assert len(ctx.write_line_crops(images, none, crop_h=OC.CROP_H, max_w=OC.MAX_W, paths=[], heights=hts, format="png")) == 0


def test_demo_batch_ragged_png_and_png_crops(tmp_path, arena):
    """three PNG files and three JPEG files of six sizes that resize_im maps to width 600: the library's PNG writers over the ragged batches
    against the host writers -- the same res files and names, PNG outputs and crops that decode to the same pixels, a ragged PNG batch"""
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    src = tmp_path / "in"
    src.mkdir()
    for i, (h, w) in enumerate([(120, 100), (110, 100), (115, 100)]):
        Image.fromarray(scene(h, w, 60 + i)).save(str(src / ("p%d.png" % i)))
    for i, (h, w) in enumerate([(240, 200), (100, 100), (130, 100)]):
        (src / ("j%d.jpg" % i)).write_bytes(encode(scene(h, w, 70 + i), 90, 2))
    cfg.TEST.PRECISION = "bf16"
    net = get_network("VGGnet_test")
    net.load_arena(arena)
    try:
        names = demo_batch.list_images(str(src))
        got = {}
        for form in ("gpu", "host"):
            out, crops_dir, logs = tmp_path / ("out_" + form), tmp_path / ("crops_" + form), []
            res = demo_batch.run(net, names, str(out), batch=4, write_images=True, log=logs.append, decode="gpu", crops_dir=str(crops_dir), crop_h=32, ragged=True,
                                 ragged_outputs=True, png_encode=form, ragged_png=form == "gpu", crops_format="png", crops_encode=form)
            print("form=%s: %d lines, logs: %s" % (form, sum(len(res[nm]) for nm in names), logs))
            got[form] = ({f: (out / f).read_bytes() for f in sorted(os.listdir(str(out)))}, {f: (crops_dir / f).read_bytes() for f in sorted(os.listdir(str(crops_dir)))}, res, logs)
        g, h = got["gpu"], got["host"]
        assert any("ragged PNG batches" in l and "from 1 ragged" in l for l in g[3]), g[3]
        assert any("3 are PNG files, coded on the device" in l for l in g[3]), g[3]
        assert sorted(g[0]) == sorted(h[0]) == sorted(["res_%s%d.txt" % (c, i) for c in "pj" for i in range(3)] + ["p%d.png" % i for i in range(3)] + ["j%d.jpg" % i for i in range(3)])
        assert sorted(g[1]) == sorted(h[1]) and len(g[1]) == sum(len(g[2][nm]) for nm in names) > 0 and all(f.endswith(".png") for f in g[1])
        for nm in names:
            assert np.array_equal(g[2][nm], h[2][nm]), nm
        for f in g[0]:
            if f.endswith(".txt") or f.endswith(".jpg"):
                assert g[0][f] == h[0][f], f
            else:
                assert g[0][f] != h[0][f] and np.array_equal(pillow_bgr(g[0][f]), pillow_bgr(h[0][f])), f
                assert g[0][f] == B.png_encode(np.ascontiguousarray(pillow_bgr(h[0][f]))), f
        for f in g[1]:
            assert np.array_equal(pillow_bgr(g[1][f]), pillow_bgr(h[1][f])), f
            assert g[1][f] == B.png_encode(np.ascontiguousarray(pillow_bgr(h[1][f]))), f
    finally:
        net.close()
