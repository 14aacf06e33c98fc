"""CPU: JPEG files of mixed sizes into one ragged device batch (include/ctpn_hip.h, ctpn_decode_jpeg_batch_ragged) before it reaches a GPU:
the kernels' per-thread source (csrc/jpeg_ragged_dev.h) under ASan + UBSan as a stand-alone program (tests/jpeg_ragged_host.cpp) against
Pillow's decode and the oracle's resize, the symbols and the argument errors that need no device, and demo_batch's planner."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import jpeg_ragged_cases as J

NAMES = ("ctpn_decode_jpeg_batch_ragged", "ctpn_decode_jpeg_files_ragged")


@pytest.fixture(scope="module")
def program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpeg_ragged_host") / "jpeg_ragged_host")
    # -ffp-contract=off as the kernels' unit is built
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(root, "tests", "jpeg_ragged_host.cpp")], check=True)
    return exe


def _entropy(data):
    """(layout8, qt, coefficients) of one file as ctpn_jpeg_entropy_decode fills them (the host half: no device)"""
    lib = B.load_library()
    keep, ptr, n = B._bytes_ptr(data)
    h, w = B.jpeg_probe(data)[:2]
    cap = int(lib.ctpn_jpeg_coef_capacity(h, w))
    coef = np.zeros((cap,), np.int16)
    qt = np.zeros((192,), np.uint16)
    l8 = np.zeros((8,), np.int32)
    B._check(lib.ctpn_jpeg_entropy_decode(ptr, n, coef.ctypes.data_as(C.POINTER(C.c_int16)), cap, qt.ctypes.data_as(C.POINTER(C.c_uint16)),
                                          l8.ctypes.data_as(C.POINTER(C.c_int))))
    count = 64 * (int(l8[4]) * int(l8[6]) + (2 * int(l8[5]) * int(l8[7]) if l8[2] == 3 else 0))
    assert count <= cap
    return l8, qt, coef[:count]


def test_the_set_is_what_its_table_says():
    """sizes as the probe reports them, the five layouts, the orientation, the restart interval; the expected heights from ctpn_resize_dims"""
    files = J.files()
    probes = [B.jpeg_probe(d) for d in files]
    assert [p[:2] for p in probes] == [tuple(s) for s in J.SIZES]
    assert [(p[2], p[3] & 0xff, (p[3] >> 8) + 1) for p in probes] == [(3, 2, 1), (1, 1, 1), (3, 1, 1), (3, 0x21, 1), (3, 0x12, 6)]
    assert b"\xff\xdd\x00\x04\x00\x03" in files[2]
    for (h, w), f, want in zip(J.SIZES, J.FACTORS, J.HEIGHTS):
        assert ((h, w) if f == 1.0 else B.resize_dims(h, w, f, f)) == (want, J.WC)


@pytest.mark.parametrize("order,hc", [((0, 1, 2, 3, 4), 96), ((4, 3, 2, 1, 0), 96), ((0, 1, 2, 3, 4), 112), ((3,), 16)])
def test_kernels_per_thread_source_under_sanitizers(program, tmp_path, order, hc):
    """Both kernels as loops over every thread index: the canvas equals, byte for byte, Pillow's decode (turned by the EXIF orientation)
    resized by oracle/resize_ref.py in a zero canvas; nothing from the sanitizers."""
    files = J.files()
    blob = struct.pack("<3i", len(order), hc, J.WC)
    for i in order:
        l8, qt, coef = _entropy(files[i])
        blob += l8.tobytes() + struct.pack("<di", J.FACTORS[i], coef.size) + qt.tobytes() + coef.tobytes()
    (tmp_path / "batch.bin").write_bytes(blob)
    r = subprocess.run([program, str(tmp_path / "batch.bin"), str(tmp_path / "canvas.out")], capture_output=True, text=True)
    assert r.stderr == "", r.stderr[-3000:]
    assert r.returncode == 0, r.stdout[-2000:]
    words = r.stdout.split()
    assert words[-1] == "ok" and int(words[1]) == len(order)
    if len(order) == 5:
        assert int(words[words.index("straddling") + 1]) >= 3      # IDCT workgroups that hold blocks of two images
    want, heights = J.expected(order, hc)
    raw = (tmp_path / "canvas.out").read_bytes()
    assert np.array_equal(np.frombuffer(raw[:4 * len(order)], np.int32), heights) and [J.HEIGHTS[i] for i in order] == list(heights)
    got = np.frombuffer(raw[4 * len(order):], np.uint8).reshape(want.shape)
    for k in range(len(order)):
        assert np.array_equal(got[k], want[k]), (order[k], np.argwhere(got[k] != want[k])[:4])
        assert not got[k, heights[k]:].any()


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (4, 3, 2, 1, 0)])
def test_beyond_range_files_through_the_kernels_source_under_sanitizers(program, tmp_path, order):
    """tests/jpeg_beyond_cases.py RAGGED -- five files of different layouts and heights whose coefficients leave the range an encoder reaches
    (wrapping products, 16-bit tables, row-0-only and column-0-only blocks) -- as one ragged batch at factor 1 through both kernels' per-thread
    source: IDCT workgroups hold blocks of two images and of both kinds, the block's zero-rows flag comes from its eight columns. The canvas
    equals Pillow's decode of each file and the committed vectors; nothing from ASan or UBSan (no signed overflow on the way)."""
    import jpeg_beyond_cases as BC
    import util_jpeg as U
    names = [BC.RAGGED[i] for i in order]
    files = [BC.cases()[n].data for n in names]
    want = [U.cv2_like_bgr(d) for d in files]
    assert {w.shape[1] for w in want} == {BC.RAGGED_WC} and len({w.shape[0] for w in want}) == 3
    blob = struct.pack("<3i", len(files), BC.RAGGED_HC, BC.RAGGED_WC)
    for d in files:
        l8, qt, coef = _entropy(d)
        blob += l8.tobytes() + struct.pack("<di", 1.0, coef.size) + qt.tobytes() + coef.tobytes()
    (tmp_path / "batch.bin").write_bytes(blob)
    r = subprocess.run([program, str(tmp_path / "batch.bin"), str(tmp_path / "canvas.out")], capture_output=True, text=True)
    assert r.stderr == "", r.stderr[-3000:]
    assert r.returncode == 0, r.stdout[-2000:]
    words = r.stdout.split()
    assert words[-1] == "ok" and int(words[words.index("straddling") + 1]) >= 1
    raw = (tmp_path / "canvas.out").read_bytes()
    assert list(np.frombuffer(raw[:4 * len(files)], np.int32)) == [w.shape[0] for w in want]
    got = np.frombuffer(raw[4 * len(files):], np.uint8).reshape(len(files), BC.RAGGED_HC, BC.RAGGED_WC, 3)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_beyond_cases.npz"))
    for k, n in enumerate(names):
        h = want[k].shape[0]
        assert np.array_equal(got[k, :h], want[k]), (n, np.argwhere(got[k, :h] != want[k])[:4])
        assert np.array_equal(got[k, :h], g["bgr_" + n]), n
        assert not got[k, h:].any()


def test_symbols_bindings_and_null_arguments(root):
    lib = B.load_library()
    declared = B._declare(C.CDLL(B.lib_path()))
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in declared and n + "(" in hdr
    assert hasattr(ctpn_amd.Context, "decode_jpeg_ragged")
    assert lib.ctpn_abi_version() == 10
    data = J.files()[0]
    keep, ptr, size = B._bytes_ptr(data)
    ptrs, sizes = (C.POINTER(C.c_uint8) * 1)(ptr), (C.c_size_t * 1)(size)
    fh, fw, fac, hts = (C.c_int * 1)(96), (C.c_int * 1)(82), (C.c_double * 1)(1.0), (C.c_int * 1)(0)
    out = C.c_void_p(0)
    paths = (C.c_char_p * 1)(b"/nonexistent.jpg")
    # no ctx, and every other pointer in turn
    assert lib.ctpn_decode_jpeg_batch_ragged(None, ptrs, sizes, 1, fh, fw, fac, 96, 82, 0, C.byref(out), hts) == -1
    assert lib.ctpn_decode_jpeg_files_ragged(None, paths, 1, fh, fw, fac, 96, 82, 0, C.byref(out), hts) == -1
    assert b"null pointer" in lib.ctpn_last_error()
    fake = C.c_void_p(1)      # never dereferenced: the null checks come first
    assert lib.ctpn_decode_jpeg_batch_ragged(fake, None, sizes, 1, fh, fw, fac, 96, 82, 0, C.byref(out), hts) == -1
    assert lib.ctpn_decode_jpeg_batch_ragged(fake, ptrs, sizes, 1, None, fw, fac, 96, 82, 0, C.byref(out), hts) == -1
    assert lib.ctpn_decode_jpeg_batch_ragged(fake, ptrs, sizes, 1, fh, fw, None, 96, 82, 0, C.byref(out), hts) == -1
    assert lib.ctpn_decode_jpeg_batch_ragged(fake, ptrs, sizes, 1, fh, fw, fac, 96, 82, 0, None, hts) == -1
    assert lib.ctpn_decode_jpeg_batch_ragged(fake, ptrs, sizes, 1, fh, fw, fac, 96, 82, 0, C.byref(out), None) == -1
    assert lib.ctpn_decode_jpeg_batch_ragged(fake, (C.POINTER(C.c_uint8) * 1)(), sizes, 1, fh, fw, fac, 96, 82, 0, C.byref(out), hts) == -1
    assert lib.ctpn_decode_jpeg_files_ragged(fake, (C.c_char_p * 1)(), 1, fh, fw, fac, 96, 82, 0, C.byref(out), hts) == -1


def test_resize_arithmetic_has_one_copy(root):
    """rs_coord / rs_short and the uint8 formula live in csrc/resize_pixel.h, which preprocess.hip and the ragged kernels include"""
    csrc = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    text = {n: open(os.path.join(csrc, n)).read() for n in ("resize_pixel.h", "preprocess.hip", "jpeg_ragged_dev.h", "jpeg.hip")}
    assert "void rs_coord(" in text["resize_pixel.h"] and "int rs_short(" in text["resize_pixel.h"] and "const int v = (((b0 *" in text["resize_pixel.h"]
    for n in ("preprocess.hip", "jpeg_ragged_dev.h"):
        assert '#include "resize_pixel.h"' in text[n] and "void rs_coord(" not in text[n] and "const int v = (((b0 *" not in text[n]
    assert "ragged" not in text["jpeg.hip"]      # the uniform path's two kernels are not touched


ENTRIES = [
    # name, file (h, w), layout (components, sampling | orientation << 8), factor, resized shape
    ("a.jpg", (1552, 1200), (3, 2), 0.5, (776, 600)),
    ("b.jpg", (800, 600), (3, 1), 1.0, (800, 600)),
    ("c.jpg", (2547, 1800), (1, 1), 1.0 / 3.0, (849, 600)),
    ("d.jpg", (1067, 600), (3, 0x21 | (5 << 8)), 1.0, (1067, 600)),      # (sizes are the turned image's, as the probe reports them)
    ("e.jpg", (600, 900), (3, 2), 1.0, (600, 900)),
    ("f.png", (800, 600), (-1, 0), 1.0, (800, 600)),
    ("g.bmp", (800, 600), (0, 0), 1.0, (800, 600)),
    ("h.jpg", (800, 600), (3, 1), 1.0, (800, 600)),
]


def test_planner_batches_jpeg_files_by_resized_shape():
    from ctpn_amd.ctpn.demo_batch import plan_device_jobs
    plain = plan_device_jobs(ENTRIES, 32)
    # without ragged: one job per file size, layout and orientation, as before
    assert sorted((j[1], tuple(j[4])) for j in plain) == [("host", ("g.bmp",)), ("jpg", ("a.jpg",)), ("jpg", ("b.jpg", "h.jpg")), ("jpg", ("c.jpg",)),
                                                         ("jpg", ("d.jpg",)), ("jpg", ("e.jpg",)), ("png", ("f.png",))]
    jobs = plan_device_jobs(ENTRIES, 32, ragged=True)
    assert sorted(n for j in jobs for n in j[4]) == sorted(e[0] for e in ENTRIES)                  # every image exactly once
    rag = [j for j in jobs if j[1] == "ragged"]
    assert len(rag) == 1
    (hc, wc), _, per, rs, members = rag[0]
    # the four page shapes of width 600 in one canvas, whatever their file sizes, layouts and orientations; the tallest first
    assert (hc, wc) == rs == (1067, 600) and members == ["d.jpg", "c.jpg", "b.jpg", "h.jpg", "a.jpg"]
    by_name = {e[0]: e for e in ENTRIES}
    assert per == [(by_name[n][1][0], by_name[n][1][1], by_name[n][3]) for n in members]
    # the landscape JPEG ends alone: the size-grouped path; PNG and Pillow files never join a ragged batch
    rest = {j[4][0]: j for j in jobs if j[1] != "ragged"}
    assert rest["e.jpg"][:4] == ((600, 900), "jpg", 1.0, (600, 900)) and rest["f.png"][1] == "png" and rest["g.bmp"][1] == "host"
    # batch 2: pairs; waste 0: equal resized shapes only
    assert [len(j[4]) for j in plan_device_jobs(ENTRIES, 2, ragged=True) if j[1] == "ragged"] == [2, 2]
    assert [j[4] for j in plan_device_jobs(ENTRIES, 32, ragged=True, waste=0.0) if j[1] == "ragged"] == [["b.jpg", "h.jpg"]]


def test_ragged_option_combinations():
    from ctpn_amd.ctpn.demo_batch import check_ragged_options
    for decode in ("host", "gpu", "gpu-entropy"):
        check_ragged_options(decode)                                              # the new combination is accepted
    for kw in ({"encode": "gpu"}, {"encode": "gpu-entropy"}, {"png_encode": "gpu"}, {"crops_dir": "crops"}):
        with pytest.raises(ValueError, match="uniform batches"):
            check_ragged_options("gpu", **kw)
    with pytest.raises(ValueError, match="process-pool"):
        check_ragged_options("host", decode_procs=2)
    with pytest.raises(ValueError, match="process-pool"):
        check_ragged_options("gpu", decode_pool=object())


def test_run_refuses_the_excluded_combinations_before_any_work(tmp_path):
    """demo_batch.run raises for ragged device decode with a library writer or crops -- before it touches the net (None here)"""
    from ctpn_amd.ctpn import demo_batch
    for kw in ({"encode": "gpu"}, {"png_encode": "gpu"}, {"crops_dir": str(tmp_path / "crops")}):
        with pytest.raises(ValueError, match="ragged device decode"):
            demo_batch.run(None, [], str(tmp_path / "out"), decode="gpu", ragged=True, **kw)
    with pytest.raises(ValueError, match="process-pool"):
        demo_batch.run(None, [], str(tmp_path / "out"), decode_procs=2, ragged=True)
