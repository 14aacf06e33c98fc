"""CPU: the JPEG writer over a table of images of mixed sizes (ctpn_encode_jpeg_mixed, ctpn_write_line_crops), without a device.
  * the text jpeg_fdct_mixed_kernel shares with the host -- csrc/jpeg_enc_mixed_dev.h: descriptors, work-item prefix and search, the pixel
    read -- compiled with g++ under ASan + UBSan as a stand-alone program (tests/jpeg_enc_mixed_host.cpp) and run as a subprocess over one
    table of ten sizes, as listed and reversed: every work item maps back to its (image, MCU row, tile), every coefficient offset lies in
    its image's block, rows at a pitch wider than the image are read without touching a byte outside the image's exactly-sized block, and
    the coefficients lead -- through the library's host entropy half -- to Pillow's files, byte for byte, at quality 1, 50, 95, 100;
  * the four new symbols, their bindings, ABI version 10; the argument errors that need no device; the demo option's refusals."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util_jpeg import scene  # noqa: E402
from test_jpeg_encode import entropy_decode_raw, noise, pillow_file, zigzag_order  # noqa: E402

from ctpn_amd import _binding as B  # noqa: E402

SIZES = [(1, 1), (8, 8), (16, 16), (17, 17), (15, 129), (33, 127), (32, 128), (8, 512), (32, 1), (256, 4)]
NEW_SYMBOLS = ("ctpn_encode_jpeg_mixed", "ctpn_encode_jpeg_mixed_device", "ctpn_write_line_crops", "ctpn_write_line_crops_device")


@pytest.fixture(scope="module")
def program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpeg_enc_mixed_host") / "jpeg_enc_mixed_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(root, "tests", "jpeg_enc_mixed_host.cpp")], check=True)
    return exe


def picture(h, w, seed):
    """RGB: a scene for even seeds, noise for odd ones"""
    if seed % 2:
        return noise(h, w, seed)
    return np.ascontiguousarray(scene(max(h, 8), max(w, 8), seed=seed)[:h, :w])


@pytest.fixture(scope="module")
def pictures():
    """one picture per size, computed once and never changed"""
    return [picture(h, w, 7 + k) for k, (h, w) in enumerate(SIZES)]


@pytest.mark.parametrize("order", ["listed", "reversed"])
@pytest.mark.parametrize("quality", [1, 50, 95, 100])
def test_table_of_ten_sizes_under_sanitizers_writes_pillows_files(program, pictures, tmp_path, quality, order):
    imgs = pictures if order == "listed" else pictures[::-1]
    _, qt, _ = entropy_decode_raw(pillow_file(np.zeros((8, 8, 3), np.uint8), quality))      # the tables as Pillow's file of that quality carries them
    with open(str(tmp_path / "batch.bin"), "wb") as f:
        f.write(struct.pack("<i", len(imgs)))
        f.write(np.ascontiguousarray(qt[:2]).astype("<u2").tobytes())
        for rgb in imgs:
            f.write(struct.pack("<ii", rgb.shape[0], rgb.shape[1]))
            f.write(np.ascontiguousarray(rgb[:, :, ::-1]).tobytes())
    r = subprocess.run([program, str(tmp_path / "batch.bin"), str(tmp_path / "coef.out")], capture_output=True, text=True)
    assert r.stderr == "", r.stderr[-3000:]
    assert r.returncode == 0, r.stdout[-2000:]
    words = r.stdout.split()
    want_items = sum(((h + 15) // 16) * (((w + 15) // 16 + 7) // 8) for h, w in (im.shape[:2] for im in imgs))
    assert words[-1] == "ok" and int(words[1]) == len(imgs) and int(words[4]) == want_items, r.stdout
    raw = open(str(tmp_path / "coef.out"), "rb").read()
    count = struct.unpack("<q", raw[:8])[0]
    coef = np.frombuffer(raw[8:], "<i2")
    assert coef.size == count == int(words[6])
    zz, at = zigzag_order(), 0
    for rgb in imgs:
        h, w = rgb.shape[:2]
        mcux, mcuy = (w + 15) // 16, (h + 15) // 16
        mine = coef[at: at + 384 * mcux * mcuy].reshape(-1, 64)      # packed at the prefix sums of the images' own counts
        at += 384 * mcux * mcuy
        nat = np.zeros_like(mine)
        nat[:, zz] = mine
        layout = np.array([h, w, 3, 2, 2 * mcux, mcux, 2 * mcuy, mcuy], np.int32)
        assert B.jpeg_entropy_encode(nat, layout, qt) == pillow_file(rgb, quality), (h, w, quality, order)
    assert at == count


def test_the_four_symbols_exist_are_bound_and_the_abi_version_is_still_10(root):
    lib = B.load_library()
    assert lib.ctpn_abi_version() == 10
    declared = B._declare(C.CDLL(B.lib_path()))
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in declared and ("int    %s(" % name) in hdr, name
    assert declared["ctpn_encode_jpeg_mixed"] == declared["ctpn_encode_jpeg_mixed_device"]
    assert declared["ctpn_write_line_crops"] == declared["ctpn_write_line_crops_device"]
    for name in ("encode_jpeg_mixed", "write_line_crops"):
        assert callable(getattr(B.Context, name))


def test_one_copy_of_the_forward_dct_body_and_of_the_pixel_read(root):
    """jenc_load4 lives in the shared header; jpeg_enc.hip holds ONE body (the LDS arrays, the two DCT passes) and two wrappers that call it"""
    csrc = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    unit, hdr = open(os.path.join(csrc, "jpeg_enc.hip")).read(), open(os.path.join(csrc, "jpeg_enc_mixed_dev.h")).read()
    assert hdr.count("void jenc_load4(") == 1 and "void jenc_load4(" not in unit
    assert unit.count("jfdct_1d(x, o, true)") == 1 and unit.count("__shared__ int ws[32][8][9]") == 1
    assert unit.count("jenc_fdct_item(") == 3                      # the body and its two callers
    for kernel in ("jpeg_fdct_kernel", "jpeg_fdct_mixed_kernel"):
        assert unit.count("void %s(" % kernel) == 1


def mixed_args(n=2, h=8, w=8, pitch=24, source_bytes=None):
    src = np.zeros(n * h * pitch, np.uint8)
    hs, ws = np.full(n, h, np.int32), np.full(n, w, np.int32)
    pt, of = (C.c_size_t * n)(*([pitch] * n)), (C.c_size_t * n)(*[i * h * pitch for i in range(n)])
    bufs = np.zeros((n, 4096), np.uint8)
    out = (C.c_void_p * n)(*[bufs[i].ctypes.data for i in range(n)])
    caps, sizes = (C.c_size_t * n)(*([4096] * n)), (C.c_size_t * n)()
    keep = (src, hs, ws, bufs)
    return keep, [src.ctypes.data_as(C.c_void_p), 0, src.size if source_bytes is None else source_bytes, n, B._ptr(hs, C.c_int), B._ptr(ws, C.c_int), pt, of, 95, out, caps, sizes]


@pytest.mark.parametrize("name", NEW_SYMBOLS[:2])
def test_mixed_call_checks_its_arguments_before_it_touches_a_device(name):
    """a null ctx stands behind every other check that needs no device: each call below fails on the argument named, with its message"""
    lib = B.load_library()
    fn = getattr(lib, name)
    keep, args = mixed_args()
    assert fn(None, *args) == -1 and b"null pointer" in lib.ctpn_last_error()
    # (from here on a ctx that is never dereferenced: the state and the device come behind the argument checks)
    fake = C.c_void_p(1)
    for k in (0, 4, 5, 6, 7, 9, 10, 11):
        bad = list(args)
        bad[k] = None
        assert fn(fake, *bad) == -1 and b"null pointer" in lib.ctpn_last_error(), k
    for n in (0, -3):
        bad = list(args)
        bad[3] = n
        assert fn(fake, *bad) == -1 and b"empty batch" in lib.ctpn_last_error()
    for q in (0, 101):
        bad = list(args)
        bad[8] = q
        assert fn(fake, *bad) == -1 and b"quality" in lib.ctpn_last_error()
    for h, w in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, 8)):
        keep2, bad = mixed_args(h=8, w=8)
        keep2[1][1], keep2[2][1] = h, w
        assert fn(fake, *bad) == -1 and b"image 1: bad size" in lib.ctpn_last_error(), (h, w)
    keep2, bad = mixed_args(pitch=23)
    assert fn(fake, *bad) == -1 and b"pitch is below 3 * width" in lib.ctpn_last_error()
    # the last image ends one byte behind the source; an offset behind it; both fit exactly when the last row is not padded
    keep2, bad = mixed_args(pitch=32, source_bytes=2 * 8 * 32 - 9)
    assert fn(fake, *bad) == -1 and b"image 1 does not lie inside source_bytes" in lib.ctpn_last_error()
    keep2, bad = mixed_args()
    bad[7][0] = 10 ** 9
    assert fn(fake, *bad) == -1 and b"image 0 does not lie inside source_bytes" in lib.ctpn_last_error()
    keep2, bad = mixed_args()
    bad[1] = 1                                                     # a device source: nothing bounds its pitches and offsets but this
    bad[6][1] = 1 << 40
    assert fn(fake, *bad) == -1 and b"image 1: pitch or offset of 2^40 bytes or more" in lib.ctpn_last_error()
    keep2, bad = mixed_args()
    bad[1] = 1
    bad[7][0] = 1 << 40
    assert fn(fake, *bad) == -1 and b"image 0: pitch or offset of 2^40 bytes or more" in lib.ctpn_last_error()
    keep2, bad = mixed_args()
    bad[9][1] = None                                               # a null output with a capacity
    assert fn(fake, *bad) == -1 and b"null output pointer" in lib.ctpn_last_error()


@pytest.mark.parametrize("name", NEW_SYMBOLS[2:])
def test_crop_writer_checks_its_arguments_before_it_touches_a_device(name):
    lib = B.load_library()
    fn = getattr(lib, name)
    total = C.c_int(-1)
    cnt = np.zeros(1, np.int32)
    img = np.zeros((8, 8, 3), np.uint8)
    px = img.ctypes.data_as(C.c_void_p)
    assert fn(None, px, 0, 1, 8, 8, None, 0, B._ptr(cnt, C.c_int), 32, 512, 0, 95, None, None, C.byref(total)) == -1 and total.value == 0
    assert b"null pointer" in lib.ctpn_last_error() and name.encode() in lib.ctpn_last_error()
    fake = C.c_void_p(1)
    assert fn(fake, px, 0, 1, 8, 8, None, 0, B._ptr(cnt, C.c_int), 32, 512, 0, 95, None, None, None) == -1      # total_out is always written: never null
    assert fn(fake, px, 0, 0, 8, 8, None, 0, B._ptr(cnt, C.c_int), 32, 512, 0, 95, None, None, C.byref(total)) == -1
    for crop_h, max_w, pad in ((0, 512, 0), (257, 512, 0), (32, 6, 0), (32, 65536, 0), (32, 512, 256)):
        assert fn(fake, px, 0, 1, 8, 8, None, 0, B._ptr(cnt, C.c_int), crop_h, max_w, pad, 95, None, None, C.byref(total)) == -1, (crop_h, max_w, pad)
    cnt[0] = 1                                                     # more lines than the capacity says
    assert fn(fake, px, 0, 1, 8, 8, None, 0, B._ptr(cnt, C.c_int), 32, 512, 0, 95, None, None, C.byref(total)) == -1 and b"line count" in lib.ctpn_last_error()


def test_demo_refuses_crops_encode_without_its_prerequisites_before_any_work(tmp_path):
    """demo_batch.run raises before it touches the net (None here): crops_encode='gpu' needs crops_dir, and it needs decode='gpu'"""
    from ctpn_amd.ctpn import demo_batch
    for enc in ("gpu", "gpu-entropy"):
        with pytest.raises(ValueError, match="crops_dir"):
            demo_batch.run(None, [], str(tmp_path / "out"), decode="gpu", crops_encode=enc)
        with pytest.raises(ValueError):
            demo_batch.run(None, [], str(tmp_path / "out"), decode="host", crops_dir=str(tmp_path / "crops"), crops_encode=enc)
        with pytest.raises(ValueError, match="decode='gpu'"):
            demo_batch.run(None, [], str(tmp_path / "out"), crops_encode=enc)
    with pytest.raises(ValueError, match="crops_encode"):
        demo_batch.run(None, [], str(tmp_path / "out"), decode="gpu", crops_dir=str(tmp_path / "crops"), crops_encode="device")
    with pytest.raises(ValueError):
        demo_batch.write_crops(None, str(tmp_path), [], [], encode="device")
    assert not (tmp_path / "out").exists() and not (tmp_path / "crops").exists()
    ap = demo_batch.build_parser()
    assert ap.parse_args([]).crops_encode == "host" and ap.parse_args(["--crops-encode", "gpu-entropy"]).crops_encode == "gpu-entropy"
