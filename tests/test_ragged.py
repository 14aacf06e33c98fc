"""CPU: ragged batches (images of one width and different heights in one call; include/ctpn_hip.h, ctpn_forward_ragged) before they reach a
GPU: the pure entry point and the symbols, the definition restated on the oracle (tests/ragged_ref.py), the kernels' per-thread source
(csrc/ragged_dev.h) under ASan + UBSan as a stand-alone program (tests/ragged_host.cpp), and demo_batch's planner."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
from oracle import network as N
import ragged_ref as R

NAMES = ("ctpn_ragged_valid_rows", "ctpn_forward_ragged", "ctpn_detect_ragged", "ctpn_detect_submit_ragged")


def test_valid_rows_is_the_shift_and_the_pool_chain():
    lib = B.load_library()
    for h in range(16, 1301):
        for level in range(5):
            assert lib.ctpn_ragged_valid_rows(h, level) == h >> level == B.ragged_valid_rows(h, level)
    # ... which is the row count the oracle's VALID pools leave
    for h in (16, 17, 31, 33, 49, 80, 95, 96, 776, 849, 1067):
        x = np.zeros((1, h, 16, 1), np.float32)
        for level in range(1, 5):
            x = N.maxpool2x2(x)
            assert x.shape[1] == lib.ctpn_ragged_valid_rows(h, level)
    for bad in ((-1, 0), (16, -1), (16, 5)):
        assert lib.ctpn_ragged_valid_rows(*bad) == -1
    with pytest.raises(ValueError):
        B.ragged_valid_rows(16, 5)


def test_symbols_bindings_and_null_arguments(root):
    lib = B.load_library()
    declared = B._declare(C.CDLL(B.lib_path()))
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in declared and n + "(" in hdr
    assert hasattr(ctpn_amd.Context, "forward_ragged") and hasattr(ctpn_amd.Context, "detect_ragged") and hasattr(ctpn_amd.Context, "ragged_valid_rows")
    hts = np.array([16], np.int32)
    img = np.zeros((1, 16, 16, 3), np.uint8)
    assert lib.ctpn_forward_ragged(None, img.ctypes.data_as(C.c_void_p), 0, 1, 16, 16, hts.ctypes.data_as(C.POINTER(C.c_int))) == -1
    assert lib.ctpn_detect_submit_ragged(None, img.ctypes.data_as(C.c_void_p), 0, 1, 16, 16, hts.ctypes.data_as(C.POINTER(C.c_int)), None, 0) == -1
    assert lib.ctpn_detect_ragged(None, img.ctypes.data_as(C.c_void_p), 0, 1, 16, 16, hts.ctypes.data_as(C.POINTER(C.c_int)), None, 0, None, 0, None, None, None) == -1
    assert lib.ctpn_abi_version() == 10


def test_masked_canvas_equals_the_lone_images_on_the_oracle(arena):
    """The definition, on the CPU: the masked canvas, cropped to every image's valid rows, is the oracle on that image alone; the
    canvas run as it is (random bytes below the images) is not. Measured: masked 1.4e-6 - 1.7e-6 on rpn_cls_prob_reshape and 3.8e-7 -
    4.2e-7 on rpn_bbox_pred over runs of this machine (torch's conv blocking differs by shape and thread count, nothing else does);
    unmasked 0.26 - 0.60 on rpn_cls_prob_reshape. The bounds are ten times the first measurement (1.4e-6, 3.8e-7); the unmasked canvas must
    miss them by three orders."""
    w = ctpn_amd.arena_views(arena)
    ims = R.images()
    canvas, heights = R.canvas_of(ims, R.HC)
    assert canvas.shape == (5, 96, 82, 3) and tuple(heights) == R.HEIGHTS
    keep = {"pool4", "rpn_conv/3x3"}
    masked = R.forward(canvas, heights, w, keep=keep)
    plain = R.forward(canvas, heights, w, keep=keep, mask=False)
    for i, im in enumerate(ims):
        lone = N.forward(im[None], w, keep=keep)
        hf = heights[i] >> 4
        for name, bound in (("rpn_cls_prob_reshape", 1.4e-5), ("rpn_bbox_pred", 3.8e-6)):
            assert lone[name].shape[1] == hf
            err = float(np.abs(masked[name][i, :hf] - lone[name][0]).max())
            print("image %d (h %d) %s: masked %.2e" % (i, heights[i], name, err))
            assert err <= bound, (i, name, err)
        for name in ("pool4", "rpn_conv/3x3"):
            assert lone[name].shape[1] == hf and not masked[name][i, hf:].any()
        if heights[i] < R.HC:
            err = float(np.abs(plain["rpn_cls_prob_reshape"][i, :hf] - lone["rpn_cls_prob_reshape"][0]).max())
            print("image %d (h %d): unmasked %.2e" % (i, heights[i], err))
            assert err > 1.4e-2, (i, err)


@pytest.fixture(scope="module")
def program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ragged_host") / "ragged_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(root, "tests", "ragged_host.cpp")], check=True)
    return exe


@pytest.mark.parametrize("shape,heights", [((5, 96, 82), R.HEIGHTS), ((3, 7, 5), (7, 3, 1)), ((2, 16, 16), (16, 16))])
def test_kernels_per_thread_source_under_sanitizers(program, tmp_path, shape, heights):
    """Both kernels as loops over thread indices. The mask cases (2-, 4-, 8- and 12-byte pixels, five levels, heights equal to the canvas,
    valid rows 0) are checked byte by byte inside the program; the blob's bits are compared with numpy's here (3 x 7 x 5 x 3 = 315
    floats: the last thread holds three)."""
    n, hc, w = shape
    canvas = np.random.default_rng(n).integers(0, 256, (n, hc, w, 3), dtype=np.uint8)
    with open(tmp_path / "canvas.bin", "wb") as f:
        f.write(struct.pack("<3i", n, hc, w) + np.asarray(heights, np.int32).tobytes() + canvas.tobytes())
    r = subprocess.run([program, str(tmp_path / "canvas.bin"), str(tmp_path / "blob.out")], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.splitlines()[-1] == "cases 304 ok"
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("mask ")]
    assert len(lines) == 304 and any(int(t[-1]) == 0 for t in lines) and any(int(t[-1]) > 0 for t in lines)
    want = N.image_blob(canvas)
    for i, h in enumerate(heights):
        want[i, h:] = 0.0
    got = np.fromfile(tmp_path / "blob.out", np.float32).reshape(want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _check_plan(shapes, max_batch, waste):
    from ctpn_amd.ctpn.demo_batch import plan_ragged_batches
    batches, alone = plan_ragged_batches(shapes, max_batch, waste)
    seen = sorted(i for _, m in batches for i in m) + sorted(alone)
    assert sorted(seen) == list(range(len(shapes)))                                    # every image exactly once
    for (hc, w), members in batches:
        assert 2 <= len(members) <= max_batch
        assert all(shapes[i][1] == w for i in members)                                 # one width
        hs = [shapes[i][0] for i in members]
        assert hc == max(hs)
        assert sum(hc - h for h in hs) <= waste * len(hs) * hc                         # the padded share
    return batches, alone


def test_planner():
    rng = np.random.default_rng(0)
    pages = [(int(h), 600) for h in rng.choice([776, 800, 849, 1067], 50)] + [(600, int(w)) for w in rng.choice([450, 800, 900], 20)] + [(333, 601)]
    for waste in (0.0, 0.1, 0.25, 0.5):
        for mb in (1, 2, 4, 32):
            batches, alone = _check_plan(pages, mb, waste)
            assert 70 in alone                                                         # the only image of its width
            assert (mb == 1) == (not batches)
    # equal heights form plain batches whatever waste is; nothing is padded at waste 0
    same = [(600, 900)] * 70
    batches, alone = _check_plan(same, 32, 0.0)
    assert [len(m) for _, m in batches] == [32, 32, 6] and not alone and all(s == (600, 900) for s, _ in batches)
    batches, _ = _check_plan(pages, 32, 0.0)
    assert all(len({pages[i] for i in m}) == 1 for _, m in batches)
    # one of each page shape pads 776 of 4 x 1067 rows, 18 %: one batch at the default; at 0.1 the 9:16 page stays alone (10.2 % with A4)
    four = [(776, 600), (849, 600), (800, 600), (1067, 600)]
    assert _check_plan(four, 32, 0.25) == ([((1067, 600), [3, 1, 2, 0])], [])
    assert _check_plan(four, 32, 0.1) == ([((849, 600), [1, 2, 0])], [3])
    with pytest.raises(ValueError):
        _check_plan(same, 0, 0.25)


def test_im_list_to_canvas():
    from ctpn_amd.lib.utils.blob import im_list_to_canvas
    ims = R.images()
    canvas, heights = im_list_to_canvas(ims)
    assert canvas.shape == (5, 96, 82, 3) and canvas.dtype == np.uint8 and heights.dtype == np.int32 and tuple(heights) == R.HEIGHTS
    for i, im in enumerate(ims):
        assert np.array_equal(canvas[i, :im.shape[0]], im) and not canvas[i, im.shape[0]:].any()
    with pytest.raises(ValueError):
        im_list_to_canvas([ims[0], ims[1][:, :80]])
