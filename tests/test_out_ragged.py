"""CPU: the ragged output stage (ctpn_write_annotated_files_ragged, ctpn_crop_lines_ragged, ctpn_write_line_crops_ragged), without a device.
  * the per-thread text of resize_linear_mixed_kernel -- csrc/resize_mixed_dev.h over csrc/resize_pixel.h -- compiled with g++ under ASan +
    UBSan as a stand-alone program (tests/resize_mixed_host.cpp) and run as a subprocess over the ragged canvas of tests/out_ragged_cases.py,
    as listed and reversed: every work item maps back to its (image, row, segment), each image's output equals oracle/resize_ref.py's of
    that image alone, the guard bytes around every destination block and the sentinel rows of the canvas are untouched;
  * crop_lines_kernel's text over the canvas (tests/crop_ragged_host.cpp, same sanitizers) against tests/crop_ref.py on the lone images;
  * the five new symbols, their bindings, ABI version 10; the argument errors that need no device; the demo option; one copy of each body."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_ref as R  # noqa: E402
import out_ragged_cases as OC  # noqa: E402

from ctpn_amd import _binding as B  # noqa: E402
from oracle import resize_ref  # noqa: E402

NEW_SYMBOLS = ("ctpn_write_annotated_files_ragged", "ctpn_write_annotated_files_ragged_device", "ctpn_crop_lines_ragged", "ctpn_write_line_crops_ragged",
               "ctpn_write_line_crops_ragged_device")
GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all"]


def build(root, tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(GXX + ["-o", exe, os.path.join(root, "tests", name + ".cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def resize_program(root, tmp_path_factory):
    return build(root, tmp_path_factory, "resize_mixed_host")


@pytest.fixture(scope="module")
def crop_program(root, tmp_path_factory):
    return build(root, tmp_path_factory, "crop_ragged_host")


def run_clean(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.stderr == "", r.stderr[-3000:]                       # the sanitizers are silent
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout.split()


@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_mixed_resize_text_under_sanitizers_equals_the_oracle_per_image(resize_program, tmp_path, order):
    idx = list(range(5)) if order == "listed" else list(range(5))[::-1]
    canvas, heights = OC.host_canvas(idx)
    scales = [OC.SCALES[i] for i in idx]
    dims = [resize_ref.out_dim(int(h), 1.0 / s) for h, s in zip(heights, scales)], [resize_ref.out_dim(OC.WC, 1.0 / s) for s in scales]
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(struct.pack("<iii", len(idx), OC.HC, OC.WC))
        f.write(np.asarray(heights, "<i4").tobytes() + np.asarray(dims[0], "<i4").tobytes() + np.asarray(dims[1], "<i4").tobytes())
        f.write(np.asarray(scales, "<f8").tobytes())
        f.write(canvas.tobytes())
    words = run_clean([resize_program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    want_items = sum(dh * ((dw + 255) // 256) for dh, dw in zip(*dims))
    assert words[-1] == "ok" and int(words[1]) == 5 and int(words[3]) == want_items, words
    assert sorted(zip(*dims)) == sorted([(96, 82), (160, 164), (74, 123), (8, 41), (33, 82)])      # no resize, 2 x up, non-dyadic, odd width down
    raw, at = np.fromfile(str(tmp_path / "out.bin"), np.uint8), 0
    for k, (dh, dw) in enumerate(zip(*dims)):
        pitch = (dw + 3) // 4 * 12
        block = raw[at: at + dh * pitch].reshape(dh, pitch)
        at += dh * pitch
        want = resize_ref.resize_linear(OC.lone(canvas, heights, k), 1.0 / scales[k], 1.0 / scales[k])      # (the sentinel rows are not part of it)
        assert want.shape == (dh, dw, 3)
        assert np.array_equal(block[:, : 3 * dw].reshape(dh, dw, 3), want), (order, k)
        assert not block[:, 3 * dw:].any()                      # the row padding: zeros, never part of a file
    assert at == raw.size


@pytest.mark.parametrize("crop_h", [8, OC.CROP_H])
def test_ragged_crop_text_under_sanitizers_equals_the_lone_images_crops(crop_program, tmp_path, crop_h):
    canvas, heights = OC.host_canvas()
    recs = OC.recs()
    img = [i for i, r in enumerate(recs) for _ in r]
    q = np.concatenate([r[:, :8] for r in recs if len(r)])
    wc = [R.width(rec, crop_h, OC.MAX_W) for r in recs for rec in r]
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(struct.pack("<7i", 5, OC.HC, OC.WC, len(img), crop_h, OC.MAX_W, OC.PAD))
        f.write(np.asarray(heights, "<i4").tobytes() + np.asarray(img, "<i4").tobytes() + np.asarray(wc, "<i4").tobytes() + np.ascontiguousarray(q, "<f8").tobytes())
        f.write(canvas.tobytes())
    words = run_clean([crop_program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    assert words[-1] == "ok" and int(words[1]) == len(img)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8).reshape(len(img), crop_h, OC.MAX_W, 3)
    want, want_w = R.crop_lines([OC.lone(canvas, heights, i) for i in range(5)], recs, crop_h, OC.MAX_W, OC.PAD)
    assert want_w.tolist() == wc and (crop_h != OC.CROP_H or (min(wc) == 1 and max(wc) == OC.MAX_W))
    assert np.array_equal(got, want)
    # the lines across and below an image's last row read that row, not the sentinel under it
    below = [k for k, (i, rec) in enumerate((i, rec) for i, r in enumerate(recs) for rec in r) if max(rec[5], rec[7]) > heights[i]]
    assert len(below) >= 3
    full = R.crop_lines(list(canvas), recs, crop_h, OC.MAX_W, OC.PAD)[0]      # the same lines over the whole slots: these DO read the sentinel
    assert all(not np.array_equal(full[k], want[k]) for k in below)


def test_the_five_symbols_exist_are_bound_and_the_abi_version_is_still_10(root):
    lib = B.load_library()
    assert lib.ctpn_abi_version() == 10
    declared = B._declare(C.CDLL(B.lib_path()))
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    assert "#define CTPN_ABI_VERSION 10" in hdr
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in declared and ("int    %s(" % name) in hdr, name
    assert declared[NEW_SYMBOLS[0]] == declared[NEW_SYMBOLS[1]] and declared[NEW_SYMBOLS[3]] == declared[NEW_SYMBOLS[4]]
    import inspect
    assert callable(B.Context.write_annotated_files_ragged)
    for name in ("crop_lines", "write_line_crops"):
        assert "heights" in inspect.signature(getattr(B.Context, name)).parameters
    from ctpn_amd.lib.utils import image as imutil
    assert callable(imutil.imwrite_annotated_ragged)


def annotated_args(n=2, hc=32, w=24, heights=(32, 16), scales=(1.0, 0.5), quality=95):
    canvas = np.zeros((n, hc, w, 3), np.uint8)
    hts, cnt, sc = np.asarray(heights, np.int32), np.zeros(n, np.int32), np.asarray(scales, np.float64)
    keep, paths = B._path_array(["a.jpg", "b.jpg"][:n])
    return (canvas, hts, cnt, sc, keep, paths), [canvas.ctypes.data_as(C.c_void_p), 0, n, hc, w, B._ptr(hts, C.c_int), None, 0, B._ptr(cnt, C.c_int), B._ptr(sc, C.c_double), paths,
                                                 quality]


@pytest.mark.parametrize("name", NEW_SYMBOLS[:2])
def test_annotated_ragged_checks_its_arguments_before_it_touches_a_device(name):
    """a null ctx stands behind every other check that needs no device; then a ctx that is never dereferenced: each call fails on the
    argument named, with its message and the image's index"""
    lib = B.load_library()
    fn = getattr(lib, name)
    err = lib.ctpn_last_error
    keep, args = annotated_args()
    assert fn(None, *args) == -1 and b"null pointer" in err() and name.encode() + b":" in err()
    fake = C.c_void_p(1)
    for k in (0, 5, 8, 9, 10):                                    # canvas, heights, line_counts, scales, paths
        bad = list(args)
        bad[k] = None
        assert fn(fake, *bad) == -1 and b"null pointer" in err(), k
    for n in (0, -2):
        bad = list(args)
        bad[2] = n
        assert fn(fake, *bad) == -1 and b"empty batch" in err()
    for h in (15, 33):
        keep, bad = annotated_args(heights=(32, h))
        assert fn(fake, *bad) == -1 and b"image 1: height %d outside 16 .. 32" % h in err(), h
    for s in (0.0, -1.0, float("nan"), float("inf")):
        keep, bad = annotated_args(scales=(s, 1.0))
        assert fn(fake, *bad) == -1 and b"image 0: the scale is not finite and positive" in err(), s
    for s in (1e-4, 1e9):                                         # 24 / 1e-4 = 240000 columns; 16 / 1e9 rounds to no rows
        keep, bad = annotated_args(scales=(1.0, s))
        assert fn(fake, *bad) == -1 and b"image 1: the resized image is empty or too large" in err(), s
    for q in (0, 101):
        keep, bad = annotated_args(quality=q)
        assert fn(fake, *bad) == -1 and b"quality must be 1 .. 100" in err()
    keep, bad = annotated_args()
    keep[2][1] = 1                                                # more lines than the capacity says
    assert fn(fake, *bad) == -1 and b"image 1: line count" in err()


@pytest.mark.parametrize("name", NEW_SYMBOLS[2:])
def test_ragged_crops_check_their_arguments_before_they_touch_a_device(name):
    lib = B.load_library()
    fn = getattr(lib, name)
    err = lib.ctpn_last_error
    total = C.c_int(-1)
    cnt, hts = np.zeros(2, np.int32), np.array([32, 16], np.int32)
    canvas = np.zeros((2, 32, 24, 3), np.uint8)
    px = canvas.ctypes.data_as(C.c_void_p)
    tail = (None, 0, 0, None, C.byref(total)) if name == "ctpn_crop_lines_ragged" else (95, None, None, C.byref(total))

    def call(ctx, n=2, heights=B._ptr(hts, C.c_int), crop_h=32, max_w=64, pad=0, tail=tail):
        return fn(ctx, px, 0, n, 32, 24, heights, None, 0, B._ptr(cnt, C.c_int), crop_h, max_w, pad, *tail)
    assert call(None) == -1 and total.value == 0 and b"null pointer" in err() and name.encode() + b":" in err()
    fake = C.c_void_p(1)
    assert call(fake, heights=None) == -1 and b"null pointer" in err()
    assert call(fake, tail=tail[:-1] + (None,)) == -1 and b"null pointer" in err()      # total_out is always written: never null
    assert call(fake, n=0) == -1 and b"empty batch" in err()
    for h in (15, 33):
        hts[1] = h
        total.value = -1
        assert call(fake) == -1 and total.value == 0 and b"image 1: height %d outside 16 .. 32" % h in err(), h
    hts[1] = 16
    for crop_h, max_w, pad in ((0, 64, 0), (257, 64, 0), (32, 6, 0), (32, 65536, 0), (32, 64, 256)):
        assert call(fake, crop_h=crop_h, max_w=max_w, pad=pad) == -1, (crop_h, max_w, pad)
    cnt[0] = 1                                                    # (the writers' quality stands behind the ctx's state: tests/test_gpu_out_ragged.py)
    assert call(fake) == -1 and b"line count" in err()


def test_demo_option_ragged_outputs(tmp_path):
    from ctpn_amd.ctpn import demo_batch
    chk = demo_batch.check_ragged_options
    for decode in ("gpu", "gpu-entropy"):
        for encode in ("host", "gpu", "gpu-entropy"):
            chk(decode=decode, encode=encode, crops_dir=str(tmp_path / "crops"), ragged_outputs=True)      # accepted
        with pytest.raises(ValueError, match="png_encode"):
            chk(decode=decode, png_encode="gpu", ragged_outputs=True)
        with pytest.raises(ValueError, match="ragged=True"):
            chk(decode=decode, encode="gpu", ragged_outputs=True, ragged=False)
        with pytest.raises(ValueError):                           # without the keyword: today's refusals
            chk(decode=decode, encode="gpu")
        with pytest.raises(ValueError):
            chk(decode=decode, crops_dir=str(tmp_path / "crops"))
    with pytest.raises(ValueError, match="decode="):
        chk(decode="host", ragged_outputs=True)
    # run raises before it touches the net (None here) or the disk
    with pytest.raises(ValueError, match="ragged=True"):
        demo_batch.run(None, [], str(tmp_path / "out"), decode="gpu", encode="gpu", ragged_outputs=True)
    with pytest.raises(ValueError, match="decode="):
        demo_batch.run(None, [], str(tmp_path / "out"), decode="host", ragged=True, ragged_outputs=True)
    with pytest.raises(ValueError, match="png_encode"):
        demo_batch.run(None, [], str(tmp_path / "out"), decode="gpu", png_encode="gpu", ragged=True, ragged_outputs=True)
    with pytest.raises(ValueError):
        demo_batch.run(None, [], str(tmp_path / "out"), decode="gpu", encode="gpu", ragged=True)
    assert not (tmp_path / "out").exists() and not (tmp_path / "crops").exists()
    ap = demo_batch.build_parser()
    assert ap.parse_args([]).ragged_outputs is False and ap.parse_args(["--ragged", "--ragged-outputs"]).ragged_outputs is True
    import inspect
    for fn in (demo_batch.run, demo_batch._run_gpu, chk):
        assert inspect.signature(fn).parameters["ragged_outputs"].default is False


def test_one_copy_of_the_drawing_body_and_of_the_resize_arithmetic(root):
    csrc = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    unit = open(os.path.join(csrc, "jpeg_enc.hip")).read()
    assert unit.count("for (int dy = -1; dy <= 1; ++dy)") == 1      # the stamp loop: one body ...
    assert unit.count("draw_boxes_image(") == 3                      # ... and its two callers
    for kernel in ("draw_boxes_kernel", "draw_boxes_ragged_kernel"):
        assert unit.count("void %s(" % kernel) == 1
    defs = re.compile(r"\b(?:void|int)\s+(rs_coord|rs_u8|rs_weights)\s*\(")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".h", ".hip", ".cpp")):
            found = defs.findall(open(os.path.join(csrc, name)).read())
            assert (sorted(found) == ["rs_coord", "rs_u8", "rs_weights"]) if name == "resize_pixel.h" else not found, name
    mixed = open(os.path.join(csrc, "resize_mixed_dev.h")).read()
    assert "rs_coord(" in mixed and "rs_u8(" in mixed and '#include "resize_pixel.h"' in mixed
    crop = open(os.path.join(csrc, "crop.hip")).read()
    assert crop.count("crop_quad(") == 1 and crop.count("void crop_lines_kernel(") == 1      # one crop kernel serves both forms
    mk = open(os.path.join(csrc, "Makefile")).read()
    nocontract = [ln for ln in mk.splitlines() if ln.startswith("NOCONTRACT_UNITS")][0]
    assert " resize_mixed" in nocontract and " resize_mixed " in mk.split("SRCS =")[1].splitlines()[0] and "resize_mixed_dev.h" in mk
