"""CPU: the text-line crops (ctpn_crop_lines) pinned without a GPU. The kernel's per-sample SOURCE TEXT (csrc/crop_pixel.h, what
crop_lines_kernel is built from) is compiled with g++ (tests/crop_host.cpp), driven like the kernel -- four output pixels per thread, three
dwords per store -- and compared bit for bit with the numpy restatement of the definition (tests/crop_ref.py); that restatement in turn is
held against an exact copy, the project's own resize (oracle/resize_ref.py) and float64 bilinear interpolation. The width function is checked
through the library's pure entry point, ctpn_line_crop_width."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_ref as R  # noqa: E402

from ctpn_amd import _binding as B  # noqa: E402
from oracle import resize_ref  # noqa: E402

SHAPES = [(48, 80), (33, 81)]        # (h, w); the second has row starts that are not dword-aligned (243 bytes per row)


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def box(x, y, ws, hs, slant=0.0, shear=0.0):
    """P0 top-left, P1 top-right, P2 bottom-left, P3 bottom-right; slant lowers the right end, shear moves the bottom edge sideways"""
    return [x, y, x + ws, y + slant, x + shear, y + hs, x + ws + shear, y + hs + slant, 0.9]


@pytest.fixture(scope="module")
def host(root, tmp_path_factory):
    """csrc/crop_pixel.h compiled with g++ (tests/crop_host.cpp): crops(img, recs, widths, crop_h, max_w, pad) as the kernel computes them"""
    so = str(tmp_path_factory.mktemp("crop_host") / "libcrop_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror", "-o", so, os.path.join(root, "tests", "crop_host.cpp")], check=True)
    lib = C.CDLL(so)

    def crops(img, recs, widths, crop_h, max_w, pad=0):
        img = np.ascontiguousarray(img, np.uint8)
        recs = np.ascontiguousarray(recs, np.float64).reshape(-1, 9)
        widths = np.ascontiguousarray(widths, np.int32)
        out = np.full((len(recs), crop_h, max_w, 3), 0x5A, np.uint8)
        assert lib.crop_lines_host(img.ctypes.data_as(C.c_void_p), img.shape[0], img.shape[1], recs.ctypes.data_as(C.c_void_p), widths.ctypes.data_as(C.c_void_p),
                                   len(recs), crop_h, max_w, pad, out.ctypes.data_as(C.c_void_p)) == 0
        return out

    def width(rec, crop_h, max_w):
        r = np.ascontiguousarray(rec, np.float64)
        return lib.crop_width_host(r.ctypes.data_as(C.c_void_p), crop_h, max_w)
    crops.width = width
    return crops


def quads(h, w):
    """axis-aligned boxes, slanted and sheared quadrilaterals, boxes partly and wholly outside the image (negative coordinates included)"""
    return [box(3.0, 5.0, 40.0, 12.0), box(10.25, 7.5, 33.3, 9.75), box(0.0, 0.0, float(w), float(h)),
            box(5.0, 4.0, 50.0, 14.0, slant=6.0), box(20.0, 20.0, 45.5, 10.0, slant=-7.25, shear=3.5), box(8.5, 2.0, 30.0, 20.0, shear=-4.0),
            box(-12.5, -6.0, 40.0, 16.0), box(w - 20.0, h - 9.0, 45.0, 18.0, slant=2.0), box(-30.0, 10.0, w + 60.0, 11.0),
            box(-200.0, -100.0, 60.0, 20.0), box(w + 7.0, 3.0, 25.0, 8.0, slant=1.0)]


@pytest.mark.parametrize("crop_h", [1, 8, 32])
@pytest.mark.parametrize("h,w", SHAPES)
def test_host_compiled_source_equals_the_restatement(host, h, w, crop_h):
    img = noise(h, w, h + crop_h)
    max_w = 64
    recs = quads(h, w)
    natural = [R.width(r, crop_h, max_w) for r in recs]
    assert [host.width(r, crop_h, max_w) for r in recs] == natural
    # every record at its own width, then at every width the row-tail stores care about
    jobs = list(zip(recs, natural)) + [(r, wc) for r in recs[:8] for wc in (1, 2, 3, 4, 5, max_w)]
    for pad in (0, 255):
        got = host(img, [r for r, _ in jobs], [wc for _, wc in jobs], crop_h, max_w, pad)
        for k, (r, wc) in enumerate(jobs):
            want, _ = R.crop_line(img, r, crop_h, max_w, pad, wc)
            assert np.array_equal(got[k], want), (k, r, wc, pad)
            assert (got[k][:, wc:] == pad).all()


def test_a_squeezed_line_fills_max_w(host):
    """a line whose natural width exceeds max_w is squeezed to it: the whole quadrilateral is sampled, not its first max_w columns"""
    h, w = SHAPES[0]
    img = noise(h, w, 9)
    rec = box(2.0, 10.0, 76.0, 8.0, slant=1.5)              # 8 rows high, 76 wide: 304 columns at crop_h = 32
    for max_w in (16, 64):
        assert R.width(rec, 32, max_w) == max_w == host.width(rec, 32, max_w)
        got = host(img, [rec], [max_w], 32, max_w)[0]
        assert np.array_equal(got, R.crop_line(img, rec, 32, max_w)[0])
        X, _ = R.positions(rec, max_w, 32)
        assert X.min() < 4.0 and X.max() > 75.0             # from one end of the line to the other


@pytest.mark.parametrize("h,w", SHAPES)
def test_an_integer_box_at_its_own_size_is_an_exact_copy(host, h, w):
    """corners [x, y, x + ws, y + hs], crop_h = hs: Wc = ws, every sample falls on a pixel with weight 1, and the formula gives the pixel back"""
    img = noise(h, w, 3)
    for (x, y, ws, hs) in [(0, 0, w if w % 4 == 0 else w - 1, h), (5, 3, 20, 8), (w - 13, h - 7, 12, 7), (17, 11, 1, 1), (2, 2, 37, 29)]:
        max_w = (ws + 3) // 4 * 4
        rec = box(float(x), float(y), float(ws), float(hs))
        assert host.width(rec, hs, max_w) == ws
        got = host(img, [rec], [ws], hs, max_w, 7)[0]
        assert np.array_equal(got[:, :ws], img[y:y + hs, x:x + ws]), (x, y, ws, hs)
        assert (got[:, ws:] == 7).all()
        assert np.array_equal(R.crop_line(img, rec, hs, max_w, 7)[0], got)


@pytest.mark.parametrize("h,w", SHAPES)
def test_twice_the_size_equals_the_projects_resize_inside(host, h, w):
    """an integer box at least 2 pixels inside the image, crop_h = 2 hs: away from the crop's edge (where only the clamp differs: the crop
    reads the pixels around the box, the resize of the slice replicates the slice's border) it is cv2.resize(slice, fx = 2, fy = 2)"""
    img = noise(h, w, 4)
    for (x, y, ws, hs) in [(2, 2, w - 4, h - 4), (7, 5, 21, 9), (30, 12, 16, 16)]:
        rec = box(float(x), float(y), float(ws), float(hs))
        max_w = (2 * ws + 3) // 4 * 4
        assert host.width(rec, 2 * hs, max_w) == 2 * ws
        got = host(img, [rec], [2 * ws], 2 * hs, max_w)[0][:, :2 * ws]
        want = resize_ref.resize_linear(np.ascontiguousarray(img[y:y + hs, x:x + ws]), 2, 2)
        assert want.shape == got.shape
        assert np.array_equal(got[2:-2, 2:-2], want[2:-2, 2:-2]), (x, y, ws, hs)
        assert not np.array_equal(got, want)                # (the edge does differ on noise: the test is not vacuous about what it skips)


def test_at_most_one_grey_level_from_exact_bilinear(host):
    """an oracle that shares nothing with the fixed-point formula: rint of the float64 bilinear value. The 11-bit weights and the two
    truncating shifts cost less than one level before rounding (0.776 measured with this arithmetic in oracle/resize_ref.py at seven scale
    factors on 40 x 56 noise), so at most 1 after it."""
    worst = 0
    for h, w in SHAPES:
        img = noise(h, w, 5)
        for crop_h in (8, 32):
            for rec in quads(h, w):
                wc = R.width(rec, crop_h, 64)
                got = host(img, [rec], [wc], crop_h, 64)[0][:, :wc].astype(np.int64)
                X, Y = R.positions(rec, wc, crop_h)
                want = np.rint(R.bilinear_exact(img, X, Y)).astype(np.int64)
                worst = max(worst, int(np.abs(got - want).max()))
    print("max |crop - rint(exact bilinear)| = %d grey levels" % worst)
    assert worst <= 1


def lib_width(rec, crop_h, max_w):
    r = np.ascontiguousarray(rec, np.float64)
    out = C.c_int(-7)
    B._check(B.load_library().ctpn_line_crop_width(B._ptr(r, C.c_double), crop_h, max_w, C.byref(out)))
    return out.value


def test_width_equals_the_formula():
    rng = np.random.default_rng(11)
    for k in range(1000):
        q = rng.uniform(-50, 400, 8) if k % 3 else np.array(box(*rng.uniform(0, 300, 2), rng.uniform(0.1, 500), rng.uniform(0.1, 40), rng.uniform(-9, 9))[:8])
        rec = list(q) + [0.9]
        crop_h, max_w = int(rng.integers(1, 257)), int(rng.integers(1, 300)) * 4
        assert lib_width(rec, crop_h, max_w) == R.width(rec, crop_h, max_w) == B.line_crop_width(rec, crop_h, max_w), rec
    # degenerate quadrilaterals: no height (hlen counts as 1), no size at all (width 1)
    assert lib_width([10, 5, 30, 5, 10, 5, 30, 5, 1], 16, 512) == 320
    assert lib_width([10, 5, 30, 5, 10, 5.5, 30, 5.5, 1], 16, 512) == 320      # half a pixel high: still 1
    assert lib_width([7, 7, 7, 7, 7, 7, 7, 7, 1], 32, 512) == 1
    # ties go to the even neighbour: crop_h * wlen / hlen = 0.5, 1.5, 2.5, 3.5, 4.5 (the first then clamped to 1)
    assert [lib_width(box(0.0, 0.0, float(wl), 2.0), 1, 64) for wl in (1, 3, 5, 7, 9)] == [1, 2, 2, 4, 4]
    assert [R.width(box(0.0, 0.0, float(wl), 2.0), 1, 64) for wl in (1, 3, 5, 7, 9)] == [1, 2, 2, 4, 4]
    # squeezed
    assert lib_width(box(0.0, 0.0, 1000.0, 10.0), 32, 512) == 512 and lib_width(box(0.0, 0.0, 1e300, 10.0), 32, 512) == 512


def test_abi_is_still_10_and_the_symbols_exist():
    lib = B.load_library()
    assert lib.ctpn_abi_version() == 10
    for name in ("ctpn_line_crop_width", "ctpn_crop_lines"):
        assert hasattr(lib, name)


def test_argument_errors():
    lib = B.load_library()
    rec = np.array(box(3.0, 4.0, 50.0, 10.0), np.float64)
    p, out = B._ptr(rec, C.c_double), C.c_int(-7)
    assert lib.ctpn_line_crop_width(p, 32, 512, C.byref(out)) == 0 and out.value == 160
    assert lib.ctpn_line_crop_width(None, 32, 512, C.byref(out)) == -1
    assert lib.ctpn_line_crop_width(p, 32, 512, None) == -1
    for crop_h in (0, -1, 257):
        assert lib.ctpn_line_crop_width(p, crop_h, 512, C.byref(out)) == -1 and b"crop_h" in lib.ctpn_last_error()
    for max_w in (0, 3, 6, 510, 65536, 65538):
        assert lib.ctpn_line_crop_width(p, 32, max_w, C.byref(out)) == -1 and b"max_w" in lib.ctpn_last_error()
    assert lib.ctpn_line_crop_width(p, 1, 4, C.byref(out)) == 0 and lib.ctpn_line_crop_width(p, 256, 65532, C.byref(out)) == 0
    for k in range(8):
        for v in (np.nan, np.inf, -np.inf):
            bad = rec.copy()
            bad[k] = v
            assert lib.ctpn_line_crop_width(B._ptr(bad, C.c_double), 32, 512, C.byref(out)) == -1 and b"finite" in lib.ctpn_last_error()
    bad = rec.copy()
    bad[8] = np.nan                                        # the score is not a coordinate
    assert lib.ctpn_line_crop_width(B._ptr(bad, C.c_double), 32, 512, C.byref(out)) == 0
    # the ctx entry point checks its arguments before it touches a device, and always writes the total
    total, cnt = C.c_int(5), np.array([1], np.int32)
    assert lib.ctpn_crop_lines(None, None, 0, 1, 8, 8, p, 1, B._ptr(cnt, C.c_int), 32, 512, 0, None, 0, 0, None, C.byref(total)) == -1
    assert total.value == 0
