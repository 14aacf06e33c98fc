"""CPU: the PNG writer (csrc/png_enc.hip, csrc/api_png_out.hip) before it reaches a GPU. Its per-piece source, csrc/png_enc_dev.h, is
compiled with g++ under AddressSanitizer + UBSan into a stand-alone program (tests/png_enc_host.cpp) that runs every pass as a loop over
thread indices, all images of tests/png_enc_ref.py as one batch, and writes the files. Every file must inflate (zlib) to the filtered
stream, decode (Pillow, ctpn_png_decode) to the pixels, hold the tokens the rule restated in png_enc_ref.py gives -- counted, by kind --,
and equal the library's host form (ctpn_png_encode) byte for byte, with the sanitizers silent. Then the host form through the C ABI, and
the size conditions (caps, not measurements).

The set's stream sizes around one piece are 255, 256, 258 and 259 bytes: h (1 + 3 w) = 257 has no solution."""
import ctypes as C
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import ctpn_amd  # noqa: F401
from ctpn_amd import _binding as B
import png_enc_ref as R

IMAGES = R.images()
NAMES = list(IMAGES)
EXTRA = {"flat-600x900": (R.flat(600, 900), 0), "page-300x450-near-only": (IMAGES["page-300x450"], 1)}


@pytest.fixture(scope="module")
def program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("png_enc_host") / "png_enc_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(root, "tests", "png_enc_host.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def result(program, tmp_path_factory):
    """one run of the program over the set and the two extra images: name -> dict(file, lit, near, far, bits), and its output"""
    d = tmp_path_factory.mktemp("png_enc_out")
    order = [(k, IMAGES[k], 0) for k in NAMES] + [(k, im, fl) for k, (im, fl) in EXTRA.items()]
    with open(d / "cases.bin", "wb") as f:
        for _, im, fl in order:
            f.write(struct.pack("<3i", im.shape[0], im.shape[1], fl) + np.ascontiguousarray(im).tobytes())
    r = subprocess.run([program, str(d / "cases.bin"), str(d)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "image":
            k = int(t[1])
            rec = dict(zip(t[2::2], (int(v) for v in t[3::2])))
            rec["file"] = (d / ("%d.png" % k)).read_bytes()
            assert len(rec["file"]) == rec["bytes"]
            out[order[k][0]] = rec
    assert len(out) == len(order) and r.stdout.splitlines()[-1] == "cases %d ok" % len(order)
    return out, r.stdout


def chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body)
        out.append((kind, body))
        at += 12 + n
    assert at == len(data)
    return out


def test_the_set_is_what_it_is_meant_to_be():
    sizes = {k: R.stream_bytes(*im.shape[:2]) for k, im in IMAGES.items()}
    assert {255, 256, 258, 259} <= set(sizes.values())
    assert 1 + 3 * 85 == 256 and 1 + 3 * 10922 == 32767 and 1 + 3 * 10923 == 32770
    t = R.tokenise(R.filtered(IMAGES["repeated-rows"]), 301)
    assert t["l2_gt"] > 0 and t["l1_gt"] > 0 and t["tie"] > 0
    t = R.tokenise(R.filtered(IMAGES["noise-64x96"]), 289)
    assert t["near"] + t["far"] < 8 and t["lit"] > 18000
    t = R.tokenise(R.filtered(IMAGES["flat-40x700"]), 2101)
    assert max(t["lengths"]) == 256 and t["lit"] < 3 * 40 + 2 * 330      # runs cut at piece ends: never 258 at P = 256
    assert R.tokenise(R.filtered(IMAGES["2x10922"]), 32767)["far"] > 100 and R.tokenise(R.filtered(IMAGES["2x10923"]), 32770)["far"] == 0
    assert sum(k.startswith("demo-") for k in IMAGES) == 5


def test_the_code_length_builder_holds_its_three_properties(result):
    lines = [l for l in result[1].splitlines() if l.startswith("lengths ")]
    assert len(lines) == 5 and all(l.endswith(" ok") and "kraft 32768 / 32768" in l for l in lines), lines
    assert "fibonacci-40: max 15 " in lines[0]


@pytest.mark.parametrize("name", NAMES + list(EXTRA))
def test_every_file_is_the_defined_container_and_decodes_to_the_pixels(result, name):
    im = IMAGES[name] if name in IMAGES else EXTRA[name][0]
    rec = result[0][name]
    h, w = im.shape[:2]
    ch = chunks(rec["file"])
    assert [k for k, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert ch[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0) and ch[2][1] == b""
    z = ch[1][1]
    assert z[:2] == b"\x78\x01" and z[2] & 7 == 0b101      # BFINAL = 1, BTYPE = 2
    want = R.filtered(im).tobytes()
    d = zlib.decompressobj()
    assert d.decompress(z) == want and d.eof and d.unused_data == b""
    assert struct.unpack(">I", z[-4:])[0] == zlib.adler32(want)
    assert (rec["bits"] + 7) // 8 == len(z) - 6
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(rec["file"])).convert("RGB"))[:, :, ::-1], im)
    assert np.array_equal(B.png_decode(rec["file"]), im)
    assert len(rec["file"]) <= B.png_encode_capacity(h, w)


@pytest.mark.parametrize("name", NAMES + ["page-300x450-near-only"])
def test_the_tokens_are_the_rules(result, name):
    im, far = (IMAGES[name], True) if name in IMAGES else (EXTRA[name][0], False)
    t = R.tokenise(R.filtered(im), 1 + 3 * im.shape[1], far=far)
    rec = result[0][name]
    assert t["covered"] == R.stream_bytes(*im.shape[:2])
    assert (rec["lit"], rec["near"], rec["far"]) == (t["lit"], t["near"], t["far"])


@pytest.mark.parametrize("name", NAMES + ["flat-600x900"])
def test_the_library_host_form_writes_the_same_bytes(result, name):
    im = IMAGES[name] if name in IMAGES else EXTRA[name][0]
    assert B.png_encode(im) == result[0][name]["file"]


def test_size_conditions(result):
    flat = result[0]["flat-600x900"]["file"]
    assert len(flat) < 600 * 900 * 3 // 20
    assert len(result[0]["page-300x450"]["file"]) < len(result[0]["page-300x450-near-only"]["file"])


def test_host_form_through_the_c_abi():
    lib = B.load_library()
    assert lib.ctpn_abi_version() == 10
    for n in ("ctpn_png_encode_capacity", "ctpn_png_encode", "ctpn_encode_png_batch", "ctpn_write_annotated_png_files", "ctpn_png_encode_device_stats"):
        assert hasattr(lib, n), n
    im = IMAGES["9x85-page"]
    h, w = im.shape[:2]
    px = im.ctypes.data_as(C.POINTER(C.c_uint8))
    size = C.c_size_t(0)
    assert lib.ctpn_png_encode(px, h, w, None, 0, C.byref(size)) == B.CTPN_ERR_CAPACITY      # sizing with NULL
    need = size.value
    assert 63 < need <= lib.ctpn_png_encode_capacity(h, w)
    buf = np.zeros((need + 8,), np.uint8)
    buf[need:] = 0xAB
    size = C.c_size_t(0)
    assert lib.ctpn_png_encode(px, h, w, buf.ctypes.data_as(C.POINTER(C.c_uint8)), need - 1, C.byref(size)) == B.CTPN_ERR_CAPACITY and size.value == need
    assert not buf[:need].any()      # nothing written into a buffer that is too small
    assert lib.ctpn_png_encode(px, h, w, buf.ctypes.data_as(C.POINTER(C.c_uint8)), need, C.byref(size)) == 0 and size.value == need
    assert (buf[need:] == 0xAB).all()
    assert np.array_equal(B.png_decode(buf[:need].tobytes()), im)
    # argument errors
    out = buf.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.ctpn_png_encode(None, h, w, out, need, C.byref(size)) == -1
    assert lib.ctpn_png_encode(px, h, w, out, need, None) == -1
    assert lib.ctpn_png_encode(px, h, w, None, need, C.byref(size)) == -1
    for bad in ((0, w), (h, 0), (-1, w), (65536, 1), (1, 65536)):
        assert lib.ctpn_png_encode(px, bad[0], bad[1], out, need, C.byref(size)) == -1
        assert lib.ctpn_png_encode_capacity(*bad) == 0
    assert lib.ctpn_png_encode_capacity(65535, 65535) == 2 * 65535 * (1 + 3 * 65535) + 171 + 63
    stats = (C.c_longlong * 4)()
    assert lib.ctpn_png_encode_device_stats(None, stats) == -1
    assert lib.ctpn_encode_png_batch(None, None, 0, 1, 8, 8, None, None, None) == -1
    assert lib.ctpn_write_annotated_png_files(None, None, 0, 1, 8, 8, None, 0, None, 1.0, None) == -1


@pytest.mark.parametrize("name", NAMES)
def test_decode_of_encode_is_the_identity_and_the_capacity_holds(name):
    im = IMAGES[name]
    data = B.png_encode(im)
    assert len(data) <= B.png_encode_capacity(*im.shape[:2])
    assert np.array_equal(B.png_decode(data), im)
