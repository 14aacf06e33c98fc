"""CPU: the JPEG encoder behind the C ABI against Pillow's files, BYTE FOR BYTE (Pillow = libjpeg-turbo, the encoder family cv2.imwrite
links; save(quality=q, subsampling=2, optimize=False) is cv2.imwrite's arithmetic at q = 95).
  * the host half (ctpn_jpeg_entropy_encode: header + baseline Huffman coding) from the coefficients ctpn_jpeg_entropy_decode reads out of
    Pillow's own files;
  * the device half's SOURCE TEXT (csrc/jpeg_enc_pixel.h, what jpeg_fdct_kernel is built from) compiled with g++ (tests/jpeg_enc_host.cpp)
    and driven like the kernel: pixels -> coefficients -> the library's entropy coder -> Pillow's file."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util_jpeg import scene  # noqa: E402

from ctpn_amd import _binding as B  # noqa: E402

QUALITIES = (1, 50, 75, 95, 100)
SIZES = [(1, 1), (2, 3), (7, 9), (8, 8), (16, 16), (17, 33), (31, 47), (48, 64), (100, 75), (233, 377), (600, 900)]
EDGES = (1, 2, 15, 16, 17)


def pillow_file(rgb, quality):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def zigzag_order():
    """natural index of the k-th coefficient of the zig-zag sequence, from the walk itself (ITU-T T.81 figure 5), not from a table"""
    order, (y, x), up = [], (0, 0), True
    for _ in range(64):
        order.append(8 * y + x)
        if up:
            if x == 7:
                y, up = y + 1, False
            elif y == 0:
                x, up = x + 1, False
            else:
                y, x = y - 1, x + 1
        else:
            if y == 7:
                x, up = x + 1, True
            elif x == 0:
                y, up = y + 1, True
            else:
                y, x = y + 1, x - 1
    return np.array(order)


def entropy_decode_raw(data):
    L = B.load_library()
    h, w, _, _ = B.jpeg_probe(data)
    cap = int(L.ctpn_jpeg_coef_capacity(h, w))
    coef, qt, l8 = np.zeros(cap, np.int16), np.zeros((3, 64), np.uint16), np.zeros(8, np.int32)
    keep, ptr, n = B._bytes_ptr(data)
    B._check(L.ctpn_jpeg_entropy_decode(ptr, n, coef.ctypes.data_as(C.POINTER(C.c_int16)), cap, qt.ctypes.data_as(C.POINTER(C.c_uint16)),
                                        l8.ctypes.data_as(C.POINTER(C.c_int))))
    return coef, qt, l8


@pytest.fixture(scope="module")
def device_source_on_host(root, tmp_path_factory):
    """csrc/jpeg_enc_pixel.h compiled with g++ (tests/jpeg_enc_host.cpp) -> encode(rgb, quality) = the file the device path would write"""
    so = str(tmp_path_factory.mktemp("jpeg_enc_host") / "libjpeg_enc_host.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, os.path.join(root, "tests", "jpeg_enc_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.jpeg_enc_quant_mismatches.restype = C.c_longlong
    zz = zigzag_order()

    def encode(rgb, quality):
        h, w = rgb.shape[:2]
        bgr = np.ascontiguousarray(rgb[:, :, ::-1])
        # the tables as Pillow's own file of that quality carries them (tests the library's jpeg_quality_scaling separately, below)
        _, qt, l8 = entropy_decode_raw(pillow_file(np.zeros((8, 8, 3), np.uint8), quality))
        mcux, mcuy = (w + 15) // 16, (h + 15) // 16
        coef_zz = np.zeros(6 * mcux * mcuy * 64, np.int16)
        q2 = np.ascontiguousarray(qt[:2])
        assert lib.jpeg_enc_coefficients_host(bgr.ctypes.data_as(C.c_void_p), h, w, q2.ctypes.data_as(C.c_void_p), coef_zz.ctypes.data_as(C.c_void_p)) == 0
        nat = np.zeros_like(coef_zz).reshape(-1, 64)
        nat[:, zz] = coef_zz.reshape(-1, 64)                                   # zig-zag position k holds natural index zz[k]
        layout = np.array([h, w, 3, 2, 2 * mcux, mcux, 2 * mcuy, mcuy], np.int32)
        return B.jpeg_entropy_encode(nat, layout, qt)
    encode.lib = lib
    return encode


def test_abi_version_is_still_10_and_the_symbols_exist():
    lib = B.load_library()
    assert lib.ctpn_abi_version() == 10
    for name in ("ctpn_jpeg_encode_capacity", "ctpn_jpeg_entropy_encode", "ctpn_encode_jpeg_batch", "ctpn_write_annotated_files"):
        assert hasattr(lib, name)


@pytest.mark.parametrize("quality", QUALITIES)
def test_entropy_round_trip_reproduces_pillows_file(quality):
    """ctpn_jpeg_entropy_decode then ctpn_jpeg_entropy_encode: header, tables, Huffman codes, stuffing and padding are Pillow's."""
    for k, (h, w) in enumerate(SIZES):
        for img in (scene(h, w, seed=k), noise(h, w, k)):
            data = pillow_file(img, quality)
            coef, qt, l8 = entropy_decode_raw(data)
            assert B.jpeg_entropy_encode(coef, l8, qt) == data, (h, w, quality)


@pytest.mark.parametrize("quality", QUALITIES)
def test_device_source_compiled_for_the_host_writes_pillows_file(device_source_on_host, quality):
    for k, (h, w) in enumerate(SIZES):
        for img in (scene(h, w, seed=k + 3), noise(h, w, k + 3)):
            assert device_source_on_host(img, quality) == pillow_file(img, quality), (h, w, quality)


def test_every_edge_expansion_branch(device_source_on_host):
    """widths and heights of 1, 2, 15, 16, 17: partial MCUs, luma blocks wholly outside the image (dummy blocks), one-pixel rows and columns"""
    for h in EDGES:
        for w in EDGES:
            for q in (50, 95):
                for img in (scene(max(h, 8), max(w, 8), seed=h * 31 + w)[:h, :w], noise(h, w, h * 31 + w)):
                    img = np.ascontiguousarray(img)
                    assert device_source_on_host(img, q) == pillow_file(img, q), (h, w, q)


def test_demo_files(device_source_on_host, golden_dir):
    g = np.load(os.path.join(golden_dir, "demo_files.npz"))
    for name in g["names"]:
        key = "file_" + str(name).replace(".", "_")
        rgb = np.asarray(Image.open(io.BytesIO(g[key].tobytes())).convert("RGB"))
        assert device_source_on_host(rgb, 95) == pillow_file(rgb, 95), name


def test_quantiser_multiply_shift_equals_division(device_source_on_host):
    """jenc_quant divides by 8 q with one multiplication: exact for every baseline table value and every magnitude the FDCT of 8-bit samples
    can reach (|c| <= 8 * 1024 * sqrt 2 < 16384; tested to 20000)"""
    assert device_source_on_host.lib.jpeg_enc_quant_mismatches(20000) == 0


def test_round_trip_at_every_quality():
    """the header's DQT segments and an all-zero scan for every quality 1 .. 100 (8-bit tables throughout: force_baseline). The library's OWN
    tables -- jpeg_quality_scaling -- are reachable through a ctx only: tests/test_gpu_jpeg_encode.py covers them."""
    for q in range(1, 101):
        data = pillow_file(np.full((16, 16, 3), 128, np.uint8), q)
        coef, qt, l8 = entropy_decode_raw(data)
        assert not coef.any() and qt.max() <= 255
        assert B.jpeg_entropy_encode(coef, l8, qt) == data


def test_capacity_bounds_noise_at_quality_100(device_source_on_host):
    for k, (h, w) in enumerate([(1, 1), (16, 16), (17, 33), (233, 377), (600, 900)]):
        for img in (noise(h, w, 50 + k), (noise(h, w, 60 + k) > 127).astype(np.uint8) * 255):
            n = len(device_source_on_host(img, 100))
            assert n == len(pillow_file(img, 100)) and n <= B.jpeg_encode_capacity(h, w), (h, w, n)
    assert B.jpeg_encode_capacity(0, 5) == 0 and B.jpeg_encode_capacity(5, 70000) == 0


def test_argument_and_capacity_errors():
    lib = B.load_library()
    data = pillow_file(scene(33, 47), 90)
    coef, qt, l8 = entropy_decode_raw(data)
    i16, u16, i32, u8 = C.POINTER(C.c_int16), C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    n = C.c_size_t(0)
    out = np.zeros(len(data), np.uint8)
    args = (coef.ctypes.data_as(i16), l8.ctypes.data_as(i32), qt.ctypes.data_as(u16))
    assert lib.ctpn_jpeg_entropy_encode(None, args[1], args[2], out.ctypes.data_as(u8), out.size, C.byref(n)) == -1
    assert lib.ctpn_jpeg_entropy_encode(args[0], args[1], args[2], out.ctypes.data_as(u8), out.size, None) == -1
    # too small: CTPN_ERR_CAPACITY with the size set, nothing written behind the capacity
    out[:] = 0xAA
    assert lib.ctpn_jpeg_entropy_encode(*args, out.ctypes.data_as(u8), 100, C.byref(n)) == -4
    assert n.value == len(data) and (out[100:] == 0xAA).all() and b"too small" in lib.ctpn_last_error()
    assert lib.ctpn_jpeg_entropy_encode(*args, out.ctypes.data_as(u8), out.size, C.byref(n)) == 0 and out.tobytes() == data
    bad = l8.copy()
    bad[4] += 1                                            # block columns that do not belong to the width
    assert lib.ctpn_jpeg_entropy_encode(args[0], bad.ctypes.data_as(i32), args[2], out.ctypes.data_as(u8), out.size, C.byref(n)) == -1
    gray = l8.copy()
    gray[2] = 1
    assert lib.ctpn_jpeg_entropy_encode(args[0], gray.ctypes.data_as(i32), args[2], out.ctypes.data_as(u8), out.size, C.byref(n)) == -6
    q16 = qt.copy()
    q16[0, 5] = 300                                        # not a baseline table
    assert lib.ctpn_jpeg_entropy_encode(args[0], args[1], q16.ctypes.data_as(u16), out.ctypes.data_as(u8), out.size, C.byref(n)) == -6
    big = coef.copy()
    big[1] = 5000                                          # an AC coefficient of 13 bits
    assert lib.ctpn_jpeg_entropy_encode(big.ctypes.data_as(i16), args[1], args[2], out.ctypes.data_as(u8), out.size, C.byref(n)) == -1
    # the ctx entry points check their arguments before they touch a device
    z = C.c_size_t(0)
    assert lib.ctpn_encode_jpeg_batch(None, None, 0, 1, 8, 8, 95, None, None, None) == -1
    assert lib.ctpn_write_annotated_files(None, None, 1, 8, 8, None, 0, None, 1.0, None, 95) == -1
    assert z.value == 0


def test_host_encoder_is_clean_under_address_sanitizer(root):
    """the tests above against the host-AddressSanitizer build of the library (make asan; the environment of tools/run_asan.sh)"""
    lib = os.path.join(root, "text-detection-ctpn_amd", "libctpn_hip_asan.so")
    csrc = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "include", "ctpn_hip.h")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(s) for s in srcs):
        r = subprocess.run(["make", "-C", csrc, "asan", "-j", "8"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    rt = subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True, check=True).stdout.strip()
    env = dict(os.environ, CTPN_NO_TORCH="1", CTPN_LIB_PATH=lib, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_jpeg_encode.py"), "-q", "-m", "not gpu", "-p", "no:cacheprovider",
                        "-k", "not address_sanitizer"], capture_output=True, text=True, env=env, cwd=root, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "AddressSanitizer" not in tail, tail
