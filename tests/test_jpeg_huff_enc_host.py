"""CPU: the device Huffman coder (csrc/jpeg_huff_enc.hip) before it reaches a GPU. Its per-thread source, csrc/jpeg_huff_enc_dev.h, is
compiled with g++ under AddressSanitizer + UBSan into a stand-alone program (tests/jpeg_huff_enc_host.cpp) that runs every pass as a loop
over thread indices; this file writes the cases for it -- the coefficient sets of tests/jpeg_huff_enc_cases.py and the file the library's
HOST half (ctpn_jpeg_entropy_encode) writes for each -- and runs it as a child process. Every file must come out byte for byte (the scan
body between the host's header and EOI), the two out-of-range cases must raise the flag, and the sanitizers must stay silent."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ctpn_amd  # noqa: F401
from ctpn_amd import _binding as B
import jpeg_huff_enc_cases as E

CASES = E.cases()


@pytest.fixture(scope="module")
def program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpeg_huff_enc_host") / "jpeg_huff_enc_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(root, "tests", "jpeg_huff_enc_host.cpp")], check=True)
    return exe


def pack_case(c):
    coef, l8, _ = c
    status, data, _ = E.host_file(c)
    data = data or b""
    h, w, hs, vs = int(l8[0]), int(l8[1]), int(l8[3]) & 0xff, int(l8[6]) // int(l8[7])
    return struct.pack("<8i", h, w, hs, vs, status, E.HEADER_BYTES, coef.size, len(data)) + np.ascontiguousarray(coef, np.int16).tobytes() + data


def run(program, tmp_path, records):
    cf = tmp_path / "cases.bin"
    cf.write_bytes(b"".join(records))
    r = subprocess.run([program, str(cf)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    words = r.stdout.split()
    return dict(zip(words[-8::2], (int(v) for v in words[-7::2])))


def test_the_cases_are_what_they_are_meant_to_be():
    files = {k: E.host_file(c) for k, c in CASES.items()}
    for k in E.OUT_OF_RANGE:
        assert files[k][0] == -1 and "outside what 8-bit baseline JPEG codes" in files[k][2]
    assert all(st == 0 for k, (st, _, _) in files.items() if k not in E.OUT_OF_RANGE)
    body = lambda k: files[k][1][E.HEADER_BYTES: -2]
    assert all(d[E.HEADER_BYTES - 14: E.HEADER_BYTES - 12] == b"\xff\xda" for _, d, _ in files.values() if d)
    # category 0 and EOB alone, six times: 6 x (2 + 4), 4 x (2 + 4) + 2 x (2 + 2) bits -> 32 bits for 4:2:0
    assert E.unstuffed_bits(files["all-zero"][1]) == 4 * 6 + 2 * 4 and len(body("all-zero")) == 4
    # the bit count's restatement, which found the two padding cases, agrees with the size of every file
    for k, (st, d, _) in files.items():
        if d:
            bits = E.unstuffed_bits(d)
            assert (bits + 7) // 8 + d[E.HEADER_BYTES: -2].count(b"\xff\x00") == len(d) - E.HEADER_BYTES - 2, k
    # the 1660-bit bound is reached: every block of max-block but the first of each component, whose DC difference has 10 bits not 11
    assert E.unstuffed_bits(files["max-block"][1]) >= 9 * 1650
    assert b"\xff\x00\xff\x00" in body("ff-runs") and body("ff-dense").count(b"\xff\x00\xff\x00") > 100
    assert body("last-byte-ff")[-2:] == b"\xff\x00" and E.unstuffed_bits(files["last-byte-ff"][1]) % 8 != 0
    assert E.unstuffed_bits(files["no-padding"][1]) % 8 == 0
    assert E.unstuffed_bits(files["256x272-dense-420"][1]) // 8 > 2 * E.SCAN_ITEMS * 64       # the chunk sum takes more than two steps
    assert sum(k.startswith("file-") for k in CASES) >= 15


def test_every_case_is_reproduced_byte_for_byte_with_the_sanitizers_silent(program, tmp_path):
    summary = run(program, tmp_path, [pack_case(c) for c in CASES.values()])
    n, bad = len(CASES), len(E.OUT_OF_RANGE)
    assert summary == {"cases": n, "coded": 2 * (n - bad), "flagged": 2 * bad, "bad": 0}


def test_a_wrong_byte_in_the_expected_file_is_noticed(program, tmp_path):
    """the program compares: one flipped bit in the middle of a file's scan body must make it fail"""
    rec = bytearray(pack_case(CASES["33x47-420"]))
    rec[-40] ^= 0x10
    cf = tmp_path / "cases.bin"
    cf.write_bytes(bytes(rec))
    r = subprocess.run([program, str(cf)], capture_output=True, text=True)
    assert r.returncode == 1 and "FAIL case 0" in r.stdout and "bad 2" in r.stdout


def test_abi_is_10_and_the_four_symbols_exist():
    lib = B.load_library()
    assert lib.ctpn_abi_version() == 10
    for n in ("ctpn_encode_jpeg_batch_device", "ctpn_write_annotated_files_device", "ctpn_jpeg_entropy_encode_device", "ctpn_jpeg_entropy_encode_device_stats"):
        assert hasattr(lib, n), n
    out = (C.c_longlong * 4)()
    assert lib.ctpn_jpeg_entropy_encode_device_stats(None, out) == -1
    assert lib.ctpn_jpeg_entropy_encode_device(None, None, None, None, 0, None, None, None, None) == -1
    assert lib.ctpn_encode_jpeg_batch_device(None, None, 0, 1, 8, 8, 95, None, None, None) == -1
    assert lib.ctpn_write_annotated_files_device(None, None, 1, 8, 8, None, 0, None, 1.0, None, 95) == -1
