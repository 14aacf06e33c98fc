"""GPU (-m gpu): the Huffman decode of sequential JPEG files on the device (csrc/jpeg_huff.hip) through the C ABI. Expected values are
the library's HOST half (ctpn_jpeg_entropy_decode) for coefficients and Pillow for pixels, never the code under test; the stats prove the
device path ran rather than its host fallback. The files are tests/jpeg_huff_cases.py's, which tests/test_jpeg_huff_host.py has put through
the sanitised CPU emulation of the same source first -- the two damaged files below included."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import jpeg_huff_cases as H
from util_jpeg import cv2_like_bgr, encode, encode_custom, pillow_bgr, scene, with_exif_orientation

pytestmark = pytest.mark.gpu
ERR_STATE = -3      # CTPN_ERR_STATE


@pytest.fixture(scope="module")
def ctx(arena):
    with ctpn_amd.Context(0, 8, 600, 900, "bf16") as c:
        c.load_weights(arena)
        yield c


def host_half(data, cap):
    lib = B.load_library()
    keep, ptr, n = B._bytes_ptr(data)
    coef, qt, l8 = np.zeros(cap, np.int16), np.zeros((3, 64), np.uint16), np.zeros(8, np.int32)
    rc = lib.ctpn_jpeg_entropy_decode(ptr, n, B._ptr(coef, C.c_int16), cap, B._ptr(qt, C.c_uint16), B._ptr(l8, C.c_int))
    return rc, coef, qt, l8


@pytest.mark.parametrize("S", [128, 0], ids=["S128", "default"])
def test_seam_equals_the_host_half_on_a_batch_of_mixed_layouts(ctx, S):
    files = list(H.cases().values())
    coef, qt, l8, st = B.jpeg_entropy_decode_device(ctx, files, S)
    stats = ctx.jpeg_entropy_device_stats()
    assert stats["device"] == len(files) and stats["host"] == 0 and stats["subsequences"] > len(files) and stats["rounds"] >= 1, stats
    for i, (name, d) in enumerate(H.cases().items()):
        rc, c0, q0, l0 = host_half(d, coef.shape[1])
        assert rc == 0 and st[i] == 0, name
        assert np.array_equal(coef[i], c0) and np.array_equal(qt[i], q0) and np.array_equal(l8[i], l0), name


def test_more_subsequences_in_one_segment_than_a_workgroup_holds(ctx):
    """One 600 x 900 noise file, quality 95, no restart markers: ONE segment of more than 2048 subsequences of 1024 bits (the count
    is computed below from the scan's bits and compared with the stats) and 12996 blocks -- many times the 256 a workgroup takes per step of
    the block-count scan and of the DC prefix sum."""
    d = encode(H.noise(600, 900, 1), 95, 2)
    f = H.parse(d)
    nbits = H.unstuff_segments(d[f["scan"]:], 0, f["mcux"] * f["mcuy"])[1][0][1]
    nsub = -(-nbits // 1024)
    assert nsub > 8 * 256 and f["mcux"] * f["mcuy"] * 6 > 8 * 256
    coef, qt, l8, st = B.jpeg_entropy_decode_device(ctx, [d])
    stats = ctx.jpeg_entropy_device_stats()
    assert stats == {"device": 1, "host": 0, "subsequences": nsub, "rounds": stats["rounds"]} and stats["rounds"] >= 1, stats
    rc, c0, q0, l0 = host_half(d, coef.shape[1])
    assert rc == 0 and st[0] == 0 and np.array_equal(coef[0], c0) and np.array_equal(qt[0], q0) and np.array_equal(l8[0], l0)


@pytest.mark.parametrize("sub", [2, 0, 1], ids=["420", "444", "422"])
def test_a_batch_of_four_at_600x900_equals_the_host_form_and_pillow(ctx, sub):
    datas = [encode(scene(600, 900, 100 + i), 90, sub) for i in range(4)]
    ptr, shape = ctx.decode_jpeg_batch(datas, 600, 900, entropy="device")
    assert shape == (4, 600, 900)
    got = ctx.jpeg_batch_fetch(ptr, shape)
    assert ctx.jpeg_entropy_device_stats()["device"] == 4 and ctx.jpeg_entropy_device_stats()["host"] == 0
    ptr, shape = ctx.decode_jpeg_batch(datas, 600, 900, entropy="host")
    assert np.array_equal(got, ctx.jpeg_batch_fetch(ptr, shape))
    for i, d in enumerate(datas):
        assert np.array_equal(got[i], pillow_bgr(d)), i


def test_the_eight_exif_orientations(ctx):
    for o in range(1, 9):
        d = with_exif_orientation(encode(scene(40, 24, o), 90, 2), o)
        want = cv2_like_bgr(d)
        ptr, shape = ctx.decode_jpeg_batch([d], entropy="device")
        got = ctx.jpeg_batch_fetch(ptr, shape)[0]
        assert ctx.jpeg_entropy_device_stats()["device"] == 1
        ptr, shape = ctx.decode_jpeg_batch([d], entropy="host")
        assert shape == (1,) + want.shape[:2] and np.array_equal(got, want) and np.array_equal(got, ctx.jpeg_batch_fetch(ptr, shape)[0]), o


def test_decode_with_resize(ctx):
    datas = [encode(scene(300, 450, 7 + i), 88, 2) for i in range(2)]
    ptr, shape = ctx.decode_jpeg_batch(datas, 300, 450, 2.0, 2.0, entropy="device")
    want = np.stack([B.resize_linear(pillow_bgr(d), 2.0, 2.0) for d in datas])
    assert shape == want.shape[:3] and np.array_equal(ctx.jpeg_batch_fetch(ptr, shape), want)
    assert ctx.jpeg_entropy_device_stats()["device"] == 2


def test_three_batches_in_flight_feed_the_detector_as_the_host_form_does(ctx):
    batches = [[encode(scene(256, 384, 10 * b + i), 90, 2) for i in range(4)] for b in range(3)]

    def feed(entropy):
        got, pending = [], None
        for k, datas in enumerate(batches):
            ptr, shape = ctx.decode_jpeg_batch(datas, 256, 384, entropy=entropy)
            ctx.detect_submit(device_ptr=ptr, shape=shape, slot=k & 1)
            if pending is not None:
                got.append(ctx.detect_collect(pending, mode="H"))
            pending = k & 1
        got.append(ctx.detect_collect(pending, mode="H"))
        return got
    want, got = feed("host"), feed("device")
    assert ctx.jpeg_entropy_device_stats()["device"] == 4 and sum(len(x) for b in want for x in b) > 0
    for b in range(3):
        for i in range(4):
            assert np.array_equal(got[b][i], want[b][i]), (b, i)


def test_the_references_demo_files(ctx, tmp_path, golden_dir):
    """tests/golden/demo_files.npz: the four JPEG files (two 4:4:0, one with EXIF orientation 6) through the device path, from paths."""
    g = np.load(os.path.join(golden_dir, "demo_files.npz"))
    n = 0
    for nm in g["names"]:
        key = str(nm).replace(".", "_")
        if not str(nm).endswith(".jpg"):
            continue                                    # (010.png is not this call's)
        p = tmp_path / str(nm)
        p.write_bytes(g["file_" + key].tobytes())
        h, w = (int(v) for v in g["shape_" + key][:2])
        ptr, shape = ctx.decode_jpeg_files([str(p)], h, w, entropy="device")
        got = ctx.jpeg_batch_fetch(ptr, shape)[0]
        assert ctx.jpeg_entropy_device_stats()["device"] == 1 and ctx.jpeg_entropy_device_stats()["host"] == 0, key
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(g["sha256_" + key]), key
        n += 1
    assert n == 4


def test_routing_and_errors(ctx):
    a, b = encode(scene(48, 64, 1), 90, 2), encode(scene(48, 64, 2), 90, 0)
    with pytest.raises(B.CtpnError) as e:
        ctx.decode_jpeg_batch([encode(scene(48, 64, 1), 90, 2, progressive=True)], 48, 64, entropy="device")
    assert e.value.code == B.CTPN_ERR_UNSUPPORTED and "progressive" in str(e.value)
    with pytest.raises(B.CtpnError) as e:
        ctx.decode_jpeg_batch([a, b], 48, 64, entropy="device")
    with pytest.raises(B.CtpnError) as e0:
        ctx.decode_jpeg_batch([a, b], 48, 64)
    assert e.value.code == e0.value.code == B.CTPN_ERR_UNSUPPORTED and str(e.value) == str(e0.value)
    with ctpn_amd.Context(0, 1, 96, 160, postproc_only=True) as pc:
        with pytest.raises(B.CtpnError) as e:
            pc.decode_jpeg_batch([a], 48, 64, entropy="device")
        assert e.value.code == ERR_STATE
        with pytest.raises(B.CtpnError) as e:
            B.jpeg_entropy_decode_device(pc, [a])
        assert e.value.code == ERR_STATE
    with pytest.raises(B.CtpnError) as e:
        B.jpeg_entropy_decode_device(ctx, [a], 100)
    assert e.value.code == -1
    ptr, shape = ctx.decode_jpeg_batch([a], 48, 64, entropy="device")        # and the ctx is still usable
    assert np.array_equal(ctx.jpeg_batch_fetch(ptr, shape)[0], pillow_bgr(a))


def test_a_truncated_file_and_an_invalid_code_fall_back_to_the_host_half(ctx):
    """The two damaged files of the GPU suite (tests/test_jpeg_huff_host.py::test_the_two_damaged_files_of_the_gpu_test runs the sanitised
    emulation on these bytes): the device raises the file's flag, the library runs the host half on it, the caller sees the host form's
    status and message."""
    good = H.cases()["64x48-noise-q95-444"]
    for damaged in H.gpu_damaged_files():
        h, w = B.jpeg_probe(damaged)[:2]
        with pytest.raises(B.CtpnError) as e0:
            ctx.decode_jpeg_batch([damaged], h, w)
        with pytest.raises(B.CtpnError) as e:
            ctx.decode_jpeg_batch([damaged], h, w, entropy="device")
        assert (e.value.code, str(e.value)) == (e0.value.code, str(e0.value))
        stats = ctx.jpeg_entropy_device_stats()
        assert stats["device"] == 0 and stats["host"] == 1, stats
        coef, qt, l8, st = B.jpeg_entropy_decode_device(ctx, [good, damaged])
        assert st.tolist() == [0, e0.value.code]
        stats = ctx.jpeg_entropy_device_stats()
        assert stats["device"] == 1 and stats["host"] == 1, stats
        assert np.array_equal(coef[0], host_half(good, coef.shape[1])[1])


def test_batch_cli_gpu_entropy_writes_what_decode_gpu_writes(tmp_path, arena):
    from PIL import Image
    from ctpn_amd.ctpn import demo_batch
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    src = tmp_path / "in"
    src.mkdir()
    for i, kw in enumerate([{}, {}, {"progressive": True}]):
        (src / ("im%02d.jpg" % i)).write_bytes(encode(scene(300, 450, 40 + i), 90, 2, **kw))
    (src / "im03.jpg").write_bytes(encode_custom(scene(200, 300, 44), 1, 2, q=6))
    Image.fromarray(scene(300, 450, 99)).save(str(src / "im99.png"))
    cfg.TEST.PRECISION = "bf16"
    net = get_network("VGGnet_test")
    net.load_arena(arena)
    try:
        names = demo_batch.list_images(str(src))
        logs = []
        res_e = demo_batch.run(net, names, str(tmp_path / "e"), batch=4, write_images=False, log=logs.append, decode="gpu-entropy")
        assert net.ctx.jpeg_entropy_device_stats()["device"] >= 1
        res_g = demo_batch.run(net, names, str(tmp_path / "g"), batch=4, write_images=False, log=lambda *_: None, decode="gpu")
        assert "4 decoded on the device, 1 PNG files by the library, 0 on the host" in logs[0], logs
        for nm in names:
            assert np.array_equal(res_e[nm], res_g[nm]), nm
            stem = os.path.basename(nm).split(".")[0]
            assert (tmp_path / "e" / ("res_%s.txt" % stem)).read_bytes() == (tmp_path / "g" / ("res_%s.txt" % stem)).read_bytes(), stem
    finally:
        net.close()
