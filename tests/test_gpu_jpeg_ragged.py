"""GPU: JPEG files of mixed sizes, layouts and orientations decoded into one ragged device batch (include/ctpn_hip.h,
ctpn_decode_jpeg_batch_ragged) through the C ABI. The canvas is DEFINED by the uniform call on every file alone, so everything here is an
equality of bytes: the fetched canvas, the heights, and what the detector makes of the live canvas. The set (tests/jpeg_ragged_cases.py) is
the smallest geometry at which each part can go wrong: five layouts, factors 1 / 2 / 82/123 / 0.5, an EXIF quarter turn, a restart
interval, a height that rounds half to even onto the ragged minimum of 16, in a canvas 96 x 82 (odd block counts, a width that is no
multiple of 4, IDCT workgroups that straddle images)."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import jpeg_ragged_cases as J
import util
from util_jpeg import encode, scene

pytestmark = pytest.mark.gpu

ORDERS = ((0, 1, 2, 3, 4), (4, 3, 2, 1, 0))


@pytest.fixture(scope="module")
def weights():
    return util.stress_arena("biased")


@pytest.fixture(scope="module")
def ctx():
    with ctpn_amd.Context(0, 5, 112, 96, "bf16") as c:
        yield c


@pytest.fixture(scope="module")
def lone(ctx):
    """every file through ctpn_decode_jpeg_batch(n = 1, fx = fy = f_i): computed once, never modified"""
    out = []
    for data, (h, w), f in zip(J.files(), J.SIZES, J.FACTORS):
        ptr, shape = ctx.decode_jpeg_batch([data], h, w, f, f)
        im = ctx.jpeg_batch_fetch(ptr, shape)[0]
        im.setflags(write=False)
        out.append(im)
    return out


def _args(order):
    files = J.files()
    return [files[i] for i in order], [J.SIZES[i] for i in order], [J.FACTORS[i] for i in order]


def _want(lone, order, hc=J.HC):
    return J.canvas_of([lone[i] for i in order], hc)


def test_the_lone_decodes_are_the_oracles(lone):
    """the definition's right-hand side against the CPU pins (Pillow's decode, oracle/resize_ref.py): the two references of this file agree"""
    want, heights = J.expected()
    assert tuple(heights) == J.HEIGHTS
    for i, im in enumerate(lone):
        assert np.array_equal(im, want[i, :heights[i]]), i


@pytest.mark.parametrize("entropy", ["host", "device"])
@pytest.mark.parametrize("source", ["memory", "paths"])
def test_canvas_equals_the_uniform_call_on_every_file(ctx, lone, tmp_path, entropy, source):
    for order, hc in [(o, J.HC) for o in ORDERS] + [(ORDERS[0], 112)]:
        files, sizes, factors = _args(order)
        if source == "paths":
            for k, d in enumerate(files):
                (tmp_path / ("f%d.jpg" % k)).write_bytes(d)
            files = [str(tmp_path / ("f%d.jpg" % k)) for k in range(len(files))]
        (ptr, shape), heights = ctx.decode_jpeg_ragged(files, sizes, factors, hc, J.WC, entropy=entropy)
        assert shape == (5, hc, J.WC)
        want, want_h = _want(lone, order, hc)
        assert np.array_equal(heights, want_h) and heights.dtype == np.int32
        for (h, w), f, got in zip(sizes, factors, heights):
            assert got == (h if f == 1.0 else B.resize_dims(h, w, f, f)[0])
        got = ctx.jpeg_batch_fetch(ptr, shape)
        for k in range(5):
            assert np.array_equal(got[k], want[k]), (entropy, source, order, hc, k, np.argwhere(got[k] != want[k])[:4])
        if entropy == "device":
            assert ctx.jpeg_entropy_device_stats()["device"] == 5


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_one_workgroup_over_two_small_images_equals_pillow(ctx, entropy):
    """16 x 16 gray (4 blocks) and 24 x 16 4:2:0 (8 + 2 + 2 blocks) at factor 1: the IDCT's one workgroup holds both images and 16 dead
    lanes' blocks, which load and store nothing (csrc/jpeg_pixel.h). No other test decodes these shapes."""
    from util_jpeg import pillow_bgr
    files = [encode(scene(16, 16, 5, True), 90), encode(scene(24, 16, 6), 90, 2)]
    (ptr, shape), heights = ctx.decode_jpeg_ragged(files, [(16, 16), (24, 16)], [1.0, 1.0], 24, 16, entropy=entropy)
    assert shape == (2, 24, 16) and tuple(heights) == (16, 24)
    got = ctx.jpeg_batch_fetch(ptr, shape)
    assert np.array_equal(got[0, :16], pillow_bgr(files[0])) and not got[0, 16:].any()
    assert np.array_equal(got[1], pillow_bgr(files[1]))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_live_canvas_feeds_the_detector(weights, lone, prec):
    """detect_submit on the live device canvas against detect_ragged on the fetched host canvas: rois, anchors and lines in modes H and O, with
    two decode + submit pairs in flight and the third decode reusing the first one's buffers"""
    orders = (ORDERS[0], ORDERS[1], (2, 0, 4, 1, 3))
    with ctpn_amd.Context(0, 5, 96, 96, prec) as c:
        c.load_weights(weights)
        want = {}
        for order in orders:
            canvas, heights = _want(lone, order)
            for mode in "HO":
                want[order, mode] = c.detect_ragged(canvas, heights, mode=mode, want_rois=True)
            c.forward_ragged(canvas, heights)
            want[order, "prop"] = c.proposals(np.array([[h, J.WC, 1.0] for h in heights], np.float32), want_anchors=True)
        assert sum(len(x) for o in orders for x in want[o, "H"][0]) > 0 and all(len(r) > 0 for o in orders for r in want[o, "prop"][0])
        for mode in "HO":
            got, pending = {}, None
            for k, order in enumerate(orders):
                files, sizes, factors = _args(order)
                (ptr, shape), heights = c.decode_jpeg_ragged(files, sizes, factors, J.HC, J.WC, entropy="device" if k == 1 else "host")
                c.detect_submit(device_ptr=ptr, shape=shape, heights=heights, slot=k & 1)
                if pending is not None:
                    got[pending[1]] = c.detect_collect(pending[0], mode=mode, want_rois=True)
                pending = (k & 1, order)
            got[pending[1]] = c.detect_collect(pending[0], mode=mode, want_rois=True)
            for order in orders:
                for k in range(5):
                    assert np.array_equal(got[order][1][k], want[order, mode][1][k]), (prec, mode, order, k)
                    assert np.array_equal(got[order][0][k], want[order, mode][0][k]), (prec, mode, order, k)
        # the proposal layer's anchors, from a forward on the live canvas
        for order in orders[:2]:
            files, sizes, factors = _args(order)
            (ptr, shape), heights = c.decode_jpeg_ragged(files, sizes, factors, J.HC, J.WC)
            c.forward_ragged(None, heights, device_ptr=ptr, shape=shape)
            rois, anchors = c.proposals(np.array([[h, J.WC, 1.0] for h in heights], np.float32), want_anchors=True)
            for k in range(5):
                assert np.array_equal(rois[k], want[order, "prop"][0][k]) and np.array_equal(anchors[k], want[order, "prop"][1][k]), (prec, order, k)


def test_alternation_with_the_uniform_call(ctx, lone):
    """ragged and uniform decodes in turn on one ctx, growing then shrinking; a live canvas survives one later call of either kind"""
    from util_jpeg import pillow_bgr
    big = [encode(scene(300, 450, 70 + i), 85, 0) for i in range(3)]
    small = [encode(scene(40, 56, 80), 90, 2)]
    files, sizes, factors = _args(ORDERS[0])
    want, _ = _want(lone, ORDERS[0])
    (p1, s1), _ = ctx.decode_jpeg_ragged(files, sizes, factors, J.HC, J.WC)
    p2, s2 = ctx.decode_jpeg_batch(big, 300, 450)                                     # the other set, grown
    assert np.array_equal(ctx.jpeg_batch_fetch(p1, s1), want)                         # the canvas survived it
    (p3, s3), h3 = ctx.decode_jpeg_ragged(files[3:4], sizes[3:4], factors[3:4], 16, J.WC, entropy="device")      # shrinking: one file, the smallest canvas
    got = ctx.jpeg_batch_fetch(p2, s2)
    for i, d in enumerate(big):
        assert np.array_equal(got[i], pillow_bgr(d)), i                              # the uniform batch survived the ragged call
    assert s3 == (1, 16, J.WC) and tuple(h3) == (16,) and np.array_equal(ctx.jpeg_batch_fetch(p3, s3)[0], lone[3])
    p4, s4 = ctx.decode_jpeg_batch(small)
    assert np.array_equal(ctx.jpeg_batch_fetch(p3, s3)[0], lone[3])
    files, sizes, factors = _args(ORDERS[1])
    (p5, s5), _ = ctx.decode_jpeg_ragged(files, sizes, factors, 112, J.WC, entropy="device")                     # growing again, a taller canvas
    assert np.array_equal(ctx.jpeg_batch_fetch(p4, s4)[0], pillow_bgr(small[0]))
    assert np.array_equal(ctx.jpeg_batch_fetch(p5, s5), _want(lone, ORDERS[1], 112)[0])
    with pytest.raises(B.CtpnError):
        ctx.jpeg_batch_fetch(p5 + 64, s5)                                             # not a live batch


def _code(fn, *a, **kw):
    with pytest.raises(B.CtpnError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


def test_errors_return_before_any_launch(ctx, lone):
    """argument checks and per-file refusals: each returns with the file's index, and the ctx is usable afterwards"""
    from PIL import Image
    import io
    files, sizes, factors = _args(ORDERS[0])
    dec = ctx.decode_jpeg_ragged
    for entropy in ("host", "device"):
        # a width that does not map to wc: file 1 at factor 1 is 41 wide
        code, msg = _code(dec, files, sizes, [1.0, 1.0] + factors[2:], J.HC, J.WC, entropy=entropy)
        assert code == -1 and "file 1" in msg
        # heights: 33 x 164 at 0.45 gives 15 rows x 74 -- use a file that maps to the width but is too short / too tall
        short = encode(scene(15, 82, 90), 90, 2)
        code, msg = _code(dec, files + [short], sizes + [(15, 82)], factors + [1.0], J.HC, J.WC, entropy=entropy)
        assert code == -1 and "file 5" in msg and "16" in msg
        code, msg = _code(dec, files, sizes, factors, 95, J.WC, entropy=entropy)       # image 0 has 96 rows
        assert code == -1 and "file 0" in msg
        # a wrong file_h: the size given maps onto the canvas, the file is another one
        code, msg = _code(dec, files, [(90, 82)] + sizes[1:], factors, J.HC, J.WC, entropy=entropy)
        assert code == -1 and "file 0" in msg
        code, msg = _code(dec, files, sizes[:2] + [(148, 246)] + sizes[3:], factors[:2] + [82.0 / 246.0] + factors[3:], J.HC, J.WC, entropy=entropy)
        assert code == -1 and "file 2" in msg
        # CMYK and truncated files: the host decoder's
        buf = io.BytesIO()
        Image.fromarray(scene(96, 82, 91)).convert("CMYK").save(buf, "JPEG", quality=90)
        code, msg = _code(dec, files[:1] + [buf.getvalue()], sizes[:1] + [(96, 82)], [1.0, 1.0], J.HC, J.WC, entropy=entropy)
        assert code == B.CTPN_ERR_UNSUPPORTED and "file 1" in msg
        code, msg = _code(dec, [files[0][: len(files[0]) // 2]] + files[1:], sizes, factors, J.HC, J.WC, entropy=entropy)
        assert code == B.CTPN_ERR_UNSUPPORTED and "file 0" in msg
    # a progressive file: refused by the device-entropy form, decoded by the host form
    prog = encode(scene(96, 82, 92), 90, 2, progressive=True)
    code, msg = _code(dec, files + [prog], sizes + [(96, 82)], factors + [1.0], J.HC, J.WC, entropy="device")
    assert code == B.CTPN_ERR_UNSUPPORTED and "file 5" in msg
    (ptr, shape), heights = dec(files + [prog], sizes + [(96, 82)], factors + [1.0], J.HC, J.WC)
    p1, s1 = ctx.decode_jpeg_batch([prog], 96, 82)
    want = ctx.jpeg_batch_fetch(p1, s1)[0]
    got = ctx.jpeg_batch_fetch(ptr, shape)
    assert tuple(heights) == J.HEIGHTS + (96,) and np.array_equal(got[5], want) and np.array_equal(got[:5], _want(lone, ORDERS[0])[0])
    # a post-processing-only ctx
    with ctpn_amd.Context(0, 1, 96, 96, postproc_only=True) as pp:
        code, _ = _code(pp.decode_jpeg_ragged, files, sizes, factors, J.HC, J.WC)
        assert code == -3
    with pytest.raises(ValueError):
        dec(files, sizes, factors, J.HC, J.WC, entropy="gpu")
    with pytest.raises(ValueError):
        dec([files[0], "a.jpg"], sizes[:2], factors[:2], J.HC, J.WC)


@pytest.mark.parametrize("decode", ["gpu", "gpu-entropy"])
def test_demo_batch_ragged_device_decode_writes_the_same_result_files(weights, tmp_path, decode):
    """a directory of small JPEG files of many sizes, layouts and one quarter turn that resize_im maps to width 600 and five heights, plus a
    PNG: res_*.txt (and, for decode="gpu", the annotated images) byte-equal with and without ragged batches, in fewer batches"""
    from PIL import Image
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    from util_jpeg import encode_custom, with_exif_orientation
    src = tmp_path / "in"
    src.mkdir()

    def picture(h, w, seed):
        return np.ascontiguousarray(ctpn_amd.weights.synthetic_images(1, h, w, seed)[0][:, :, ::-1])
    made = [
        encode(picture(120, 100, 30), 90, 2),                                       # x 6  -> 720 x 600
        encode(picture(240, 200, 31), 90, 0),                                       # x 3  -> 720 x 600, another file size and layout
        encode(picture(115, 100, 32), 85, 1),                                       #      -> 690 x 600
        encode(np.ascontiguousarray(picture(100, 100, 33)[..., 1]), 90),                                 # gray -> 600 x 600
        with_exif_orientation(encode(picture(100, 104, 34), 90, 2), 6),             # stored 100 x 104, turned 104 x 100 -> 624 x 600
        encode_custom(picture(110, 100, 35), 1, 2, q=6),                            # 4:4:0 -> 660 x 600
        encode(picture(60, 50, 36), 90, 2, restart_marker_blocks=2),                # x 12 -> 720 x 600
        encode(picture(100, 100, 37), 90, 2, progressive=True),                     # progressive: the host-entropy form's
    ]
    for i, d in enumerate(made):
        (src / ("page%d.jpg" % i)).write_bytes(d)
    Image.fromarray(picture(100, 100, 38)).save(src / "page8.png")
    names = demo_batch.list_images(str(src))
    assert len(names) == 9
    cfg.TEST.PRECISION = "bf16"
    outs, nbatches = {}, {}
    for ragged in (False, True):
        net = get_network("VGGnet_test")
        net.load_arena(weights)
        try:
            out = tmp_path / ("out%d" % ragged)
            log = []
            demo_batch.run(net, names, str(out), batch=4, write_images=decode == "gpu", log=log.append, decode=decode, ragged=ragged)
        finally:
            net.close()
        outs[ragged] = {p.name: p.read_bytes() for p in sorted(out.iterdir())}
        assert "8 decoded on the device, 1 PNG files by the library, 0 on the host" in log[0], log
        nbatches[ragged] = int(log[0].split(" images in ")[1].split(" batches")[0])
    # eight file sizes and the PNG: nine batches; across heights 720, 720, 720, 690 | 660, 624, 600, 600 and the PNG: three
    assert nbatches == {False: 9, True: 3}
    res = ["res_page%d.txt" % i for i in range(9)]
    assert sorted(n for n in outs[True] if n.startswith("res_")) == res and outs[True] == outs[False]
    assert any(len(outs[True][n]) > 0 for n in res)
    if decode == "gpu":      # the annotated images too: cut from the fetched canvas, written by the host writer -- the same files
        assert sorted(n for n in outs[True] if not n.startswith("res_")) == ["page%d.jpg" % i for i in range(8)] + ["page8.png"]


def test_beyond_range_files_of_mixed_layouts_equal_each_file_alone(ctx, golden_dir):
    """tests/jpeg_beyond_cases.py RAGGED: five files whose coefficients leave the range an encoder reaches (16-bit tables, wrapping products,
    row-0-only and column-0-only blocks; 4:2:0, 4:2:2, 4:4:0, gray, an EXIF transpose; 32 and 16 and 24 rows) in one ragged call at
    factor 1, host and device entropy decoding: every slot equals the uniform call on that file alone, and both equal the committed vectors
    (tests/golden/jpeg_beyond_cases.npz). Not compared with a live Pillow: out of range the pin is libjpeg-turbo's x86 SIMD arithmetic, which
    a host without SIMD would not reproduce; the vectors carry it."""
    import os
    import jpeg_beyond_cases as BC
    g = np.load(os.path.join(golden_dir, "jpeg_beyond_cases.npz"))
    names = list(BC.RAGGED)
    files = [g["file_" + n].tobytes() for n in names]
    want = [g["bgr_" + n] for n in names]
    sizes = [B.jpeg_probe(d)[:2] for d in files]
    assert [tuple(w.shape[:2]) for w in want] == sizes and {s[1] for s in sizes} == {BC.RAGGED_WC} and len({s[0] for s in sizes}) == 3
    lone = []
    for d in files:
        ptr, shape = ctx.decode_jpeg_batch([d])
        lone.append(ctx.jpeg_batch_fetch(ptr, shape)[0])
    for entropy in ("host", "device"):
        for order in (list(range(5)), [4, 3, 2, 1, 0]):
            (ptr, shape), heights = ctx.decode_jpeg_ragged([files[i] for i in order], [sizes[i] for i in order], [1.0] * 5, BC.RAGGED_HC, BC.RAGGED_WC, entropy=entropy)
            assert shape == (5, BC.RAGGED_HC, BC.RAGGED_WC) and list(heights) == [sizes[i][0] for i in order]
            got = ctx.jpeg_batch_fetch(ptr, shape)
            for k, i in enumerate(order):
                assert np.array_equal(got[k, :heights[k]], lone[i]), (entropy, order, names[i])
                assert np.array_equal(got[k, :heights[k]], want[i]), (entropy, order, names[i])
                assert not got[k, heights[k]:].any()
            if entropy == "device":
                assert ctx.jpeg_entropy_device_stats()["device"] == 5
