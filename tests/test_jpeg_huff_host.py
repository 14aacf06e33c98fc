"""CPU: the device Huffman decoder (csrc/jpeg_huff.hip) before it reaches a GPU. Its per-thread source, csrc/jpeg_huff_dev.h, is compiled
with g++ under AddressSanitizer + UBSan into a stand-alone program (tests/jpeg_huff_host.cpp) that runs every pass as a loop over thread
indices; this file writes the cases for it -- frame, DHT segments, scan bytes, and what the library's HOST half (ctpn_jpeg_entropy_decode)
returns for the same bytes -- and runs it as a child process. Undamaged files must come out equal to the host half with no flag raised, at
every subsequence size; damaged files (truncated, single-bit flips in the scan) must end with a raised flag or with the host half's
coefficients, and with the sanitizers silent: a damaged file may not cause an out-of-range access, whatever its bits say."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ctpn_amd  # noqa: F401
from ctpn_amd import _binding as B
import jpeg_huff_cases as H

S_VALUES = ["128", "256", "1024", "4096"]
CASES = H.cases()


@pytest.fixture(scope="module")
def program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpeg_huff_host") / "jpeg_huff_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(root, "tests", "jpeg_huff_host.cpp")], check=True)
    return exe


def host_half(data):
    """(status, coefficients or None) of ctpn_jpeg_entropy_decode for these bytes."""
    lib = B.load_library()
    try:
        h, w = B.jpeg_probe(data)[:2]
    except B.CtpnError as e:
        return e.code, None
    cap = int(lib.ctpn_jpeg_coef_capacity(h, w))
    keep, ptr, n = B._bytes_ptr(data)
    coef, qt, l8 = np.zeros(cap, np.int16), np.zeros(192, np.uint16), np.zeros(8, np.int32)
    rc = lib.ctpn_jpeg_entropy_decode(ptr, n, B._ptr(coef, C.c_int16), cap, B._ptr(qt, C.c_uint16), B._ptr(l8, C.c_int))
    if rc:
        return rc, None
    nc, bw0, bw1, bh0, bh1 = int(l8[2]), int(l8[4]), int(l8[5]), int(l8[6]), int(l8[7])
    return 0, coef[: (bw0 * bh0 + (2 * bw1 * bh1 if nc == 3 else 0)) * 64]


def pack_case(data, must_decode):
    """One record of the case file, or None for bytes whose headers do not reach the scan (the parser's business, not the decoder's)."""
    f = H.parse(data)
    if f is None:
        return None
    status, coef = host_half(data)
    pad3 = lambda v: list(v) + [0] * (3 - len(v))
    rec = struct.pack("<18i", status, int(must_decode), f["ncomp"], f["mcux"], f["mcuy"], f["dri"], *pad3(f["hs"]), *pad3(f["vs"]), *pad3(f["td"]), *pad3(f["ta"]))
    for cl in (0, 1):
        for tid in range(4):
            counts, vals = f["dht"].get((cl, tid), ([0] * 16, []))
            rec += struct.pack("<2i", int((cl, tid) in f["dht"]), len(vals)) + bytes(counts) + bytes(vals) + bytes(256 - len(vals))
    scan = data[f["scan"]:]
    body = coef.tobytes() if coef is not None else b""
    return rec + struct.pack("<2q", len(scan), len(body) // 2) + scan + body


def run(program, tmp_path, records):
    cf, df = tmp_path / "cases.bin", tmp_path / "dump.bin"
    cf.write_bytes(b"".join(records))
    r = subprocess.run([program, str(cf), str(df)] + S_VALUES, capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    summary = dict(zip(r.stdout.split()[-12::2], (int(v) for v in r.stdout.split()[-11::2])))
    return summary, df.read_bytes()


def test_every_case_equals_the_host_half_at_every_subsequence_size(program, tmp_path):
    recs = [pack_case(d, True) for d in CASES.values()]
    assert all(r is not None for r in recs)
    summary, dump = run(program, tmp_path, recs)
    assert summary["cases"] == len(CASES) and summary["flagged"] == 0 and summary["decoded"] == len(CASES) * len(S_VALUES) and summary["bad"] == 0
    assert summary["max_subsequences"] > 256 and summary["max_rounds"] >= 1
    # the host's linear pass against its bytewise restatement: unstuffed bytes and segment table of every case
    at = 0
    for name, d in CASES.items():
        f = H.parse(d)
        want_bytes, want_segs = H.unstuff_segments(d[f["scan"]:], f["dri"], f["mcux"] * f["mcuy"])
        nb, found, need = struct.unpack_from("<3I", dump, at)
        at += 12
        assert dump[at: at + nb] == want_bytes, name
        at += nb
        segs = [struct.unpack_from("<4I", dump, at + 16 * k) for k in range(found)]
        at += 16 * found
        assert found == need == len(want_segs) and segs == [tuple(s) for s in want_segs], name
    assert at == len(dump)
    assert sum(len(H.unstuff_segments(d[H.parse(d)["scan"]:], H.parse(d)["dri"], H.parse(d)["mcux"] * H.parse(d)["mcuy"])[1]) > 1 for d in CASES.values()) >= 4
    assert any(b"\xff\x00" in d[H.parse(d)["scan"]:] for d in CASES.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_damaged_files_end_flagged_or_equal_with_the_sanitizers_silent(program, tmp_path, name):
    variants = H.damaged(CASES[name])
    assert len(variants) == 202
    recs = [r for r in (pack_case(d, False) for _, d in variants) if r is not None]
    assert len(recs) >= 200
    summary, _ = run(program, tmp_path, recs)
    assert summary["cases"] == len(recs) and summary["bad"] == 0


def test_the_two_damaged_files_of_the_gpu_test(program, tmp_path):
    """Exactly the bytes tests/test_gpu_jpeg_huff.py runs on the GPU: clean under the sanitizers, and flagged at every S."""
    cut, bad = H.gpu_damaged_files()
    assert host_half(cut)[0] == -6 and host_half(bad)[0] == -1
    summary, _ = run(program, tmp_path, [pack_case(cut, False), pack_case(bad, False)])
    assert summary["cases"] == 2 and summary["flagged"] == 2 * len(S_VALUES) and summary["decoded"] == 0 and summary["bad"] == 0


def test_unstuffing_restatement_on_crafted_scans():
    """The marker rules of the linear pass, on bytes no encoder writes."""
    u = H.unstuff_segments
    assert u(b"\x12\xff\x00\x34\xff\xd9\x99", 0, 4) == (b"\x12\xff\x34", [(0, 24, 0, 4)])
    assert u(b"\x12\xff\xd0\x34", 0, 4) == (b"\x12", [(0, 8, 0, 4)])                       # RSTn without a restart interval ends the data
    assert u(b"\x12\xff\xd0\x34\xff\xd1\x56\xff\xd2\x78", 2, 5) == (b"\x12\x34\x56", [(0, 8, 0, 2), (1, 8, 2, 2), (2, 8, 4, 1)])      # ... what follows the last segment is not read
    assert u(b"\x12\xff", 0, 1) == (b"\x12", [(0, 8, 0, 1)])                              # a lone FF at the end of the file
    assert u(b"\x12\xff\xff\xd0", 3, 9) == (b"\x12", [(0, 8, 0, 3)])                      # FF FF is no data: fewer segments than the frame needs
    assert u(b"", 0, 1) == (b"", [(0, 0, 0, 1)])


def test_abi_is_10_and_the_four_symbols_exist():
    lib = B.load_library()
    assert lib.ctpn_abi_version() == 10
    for n in ("ctpn_decode_jpeg_batch_device", "ctpn_decode_jpeg_files_device", "ctpn_jpeg_entropy_decode_device", "ctpn_jpeg_entropy_device_stats"):
        assert hasattr(lib, n), n
    out = (C.c_longlong * 4)()
    assert lib.ctpn_jpeg_entropy_device_stats(None, out) == -1
    assert lib.ctpn_jpeg_entropy_decode_device(None, None, None, 0, 0, None, 0, None, None, None) == -1
