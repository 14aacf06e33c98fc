"""CPU: pages in tiles (ctpn_page_plan, ctpn_page_merge, ctpn_page_text_lines on the host connector) -- what of the page path needs no device:
  * the plan, exhaustively per axis (every L in 16 .. 400, T in {32, 64, 96}, V in {0, 32}): the tiles cover the axis, the owned ranges
    partition it, origins are multiples of 16, the last valid extent exceeds V; 2-D plans against tests/page_ref.py; the argument errors;
  * the merge against the restatement on generated rois: fractional y, centres exactly on an own bound from either side, columns at own_x0
    and own_x1 - 16, a page width that is no multiple of 16 (the clip then makes a box thinner than min_size), capacity overflow;
  * the seam scene: a row of column boxes across a 64 x 352 page, reported by every tile that sees it -> exactly one box per page column, and
    one text line with the bytes ctpn_text_lines gives for the same set built in page coordinates;
  * the two device texts -- csrc/page_dev.h (the cut's per-thread body) and csrc/nms_column_dev.h (the page NMS's per-column body) -- compiled
    with g++ under ASan + UBSan as a stand-alone program (tests/page_host.cpp) and run as a subprocess: tiles equal the restatement's byte
    for byte, keep lists equal the restatement's and oracle/nms_ref.c's, from exact-size heap blocks;
  * the five symbols in header, library and binding; ABI version 10; no device: CTPN_ERR_NODEVICE, not a CPU fallback."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_cases as K  # noqa: E402
import page_ref as R  # noqa: E402

import ctpn_amd  # noqa: E402
from ctpn_amd import _binding as B  # noqa: E402
from oracle import cnms  # noqa: E402

NEW_SYMBOLS = ("ctpn_page_plan", "ctpn_page_cut", "ctpn_page_merge", "ctpn_page_nms", "ctpn_page_text_lines")
GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-pthread"]
i32p = C.POINTER(C.c_int)


# ---- the plan ----
def test_every_axis_is_covered_partitioned_and_on_the_grid():
    lib = B.load_library()
    for T in (32, 64, 96):
        for V in (0, 32):
            if V > T // 2:      # (32, 32): an overlap above half the tile is an argument error, below
                continue
            for L in range(16, 401):
                # one axis through the library: a page L x 16 .. (the other axis is one tile)
                tiles, grid = B.page_plan(L, 16, T, 96, V)
                assert grid[1] == 1 and np.array_equal(tiles[:, [1, 3, 6, 7]], np.tile([0, 16, 0, 16], (grid[0], 1)))
                o, v, a, b = tiles[:, 0], tiles[:, 2], tiles[:, 4], tiles[:, 5]
                assert [tuple(x) for x in np.stack([o, v, a, b], 1).tolist()] == R.axis(L, T, V), (L, T, V)
                assert (o % 16 == 0).all() and o[0] == 0 and (v >= 1).all() and (v <= T).all() and (o + v <= L).all()
                covered = np.zeros(L, bool)
                owned = np.zeros(L, np.int32)
                for j in range(len(o)):
                    covered[o[j]:o[j] + v[j]] = True
                    assert o[j] <= a[j] < b[j] <= o[j] + v[j], (L, T, V, j)      # a tile sees all it owns
                    owned[a[j]:b[j]] += 1
                assert covered.all() and (owned == 1).all(), (L, T, V)
                assert a[0] == 0 and b[-1] == L and (a[1:] == b[:-1]).all() and (b[:-1] % 16 == 0).all()
                assert v[-1] > V or len(o) == 1, (L, T, V)
                assert (v[:-1] == T).all()
    assert lib.ctpn_abi_version() == 10


@pytest.mark.parametrize("shape", [(100, 203, 64, 96, 32), (64, 96, 64, 96, 32), (40, 50, 64, 96, 32), (64, 352, 64, 96, 32), (399, 400, 96, 64, 0),
                                   (3508, 2480, 608, 912, 128), (16384, 16384, 608, 912, 288), (16, 16, 16, 16, 0)])
def test_plans_equal_the_restatement(shape):
    tiles, grid = B.page_plan(*shape)
    want, wgrid = R.plan(*shape)
    assert grid == wgrid and np.array_equal(tiles, want)
    h, w = shape[:2]
    own = np.zeros((h, w), np.uint8) if h * w <= 1 << 20 else None
    area = 0
    for oy, ox, vh, vw, y0, y1, x0, x1 in tiles.tolist():
        area += (y1 - y0) * (x1 - x0)
        assert oy <= y0 < y1 <= oy + vh <= h and ox <= x0 < x1 <= ox + vw <= w and oy % 16 == 0 and ox % 16 == 0
        if own is not None:
            own[y0:y1, x0:x1] += 1
    assert area == h * w and (own is None or (own == 1).all())      # the owned rectangles partition the page


def test_plan_argument_errors_and_capacity():
    lib = B.load_library()
    cnt = C.c_int(-1)
    bad = [(15, 100, 64, 96, 32), (100, 16385, 64, 96, 32), (100, 100, 60, 96, 32), (100, 100, 64, 100, 32), (100, 100, 64, 96, 16), (100, 100, 64, 96, 64),
           (100, 100, 64, 96, -32), (100, 100, 0, 96, 0), (100, 100, 32, 32, 32)]
    for args in bad:
        assert lib.ctpn_page_plan(*args, None, 0, C.byref(cnt), None) == -1, args
        assert not R.plan_ok(*args)
    assert lib.ctpn_page_plan(100, 203, 64, 96, 32, None, 0, None, None) == -1
    tiles = np.full((9, 8), -7, np.int32)
    assert lib.ctpn_page_plan(100, 203, 64, 96, 32, tiles.ctypes.data_as(i32p), 8, C.byref(cnt), None) == B.CTPN_ERR_CAPACITY
    assert cnt.value == 9 and (tiles == -7).all()
    assert lib.ctpn_page_plan(100, 203, 64, 96, 32, None, 0, C.byref(cnt), None) == 0 and cnt.value == 9      # sizing


# ---- the merge ----
def merge_case():
    """rois on a 100 x 203 page (tile 64 x 96, overlap 32: 3 x 3 tiles; the page's last column is 11 px wide)"""
    page_h, page_w = 100, 203
    tiles, _ = R.plan(page_h, page_w, K.TILE_H, K.TILE_W, K.OVERLAP)
    rng = np.random.default_rng(11)
    cap = 64
    rois = np.zeros((len(tiles), cap, 5), np.float32)
    counts = np.zeros(len(tiles), np.int32)
    for t, (oy, ox, vh, vw, y0, y1, x0, x1) in enumerate(tiles.tolist()):
        rows = []
        # centres exactly on both own bounds, and one float to either side of each
        for bound in (y0 - oy, y1 - oy):
            for cy in (np.float32(bound), np.nextafter(np.float32(bound), np.float32(-1e9)), np.nextafter(np.float32(bound), np.float32(1e9))):
                half = np.float32(9.25)
                rows.append((0.95, x0 - ox, max(cy - half, 0), x0 - ox + 15, cy + half if cy - half >= 0 else 2 * cy))
        # the first and the last owned column, and their outer neighbours
        for col in (x0, x1 - 16 if x1 % 16 == 0 else (x1 // 16) * 16, x0 - 16, x1 if x1 % 16 == 0 else (x1 // 16 + 1) * 16):
            if 0 <= col - ox and col - ox + 15 < K.TILE_W:
                rows.append((0.9, col - ox, (y0 + y1) / 2 - oy - 10.5, col - ox + 15, (y0 + y1) / 2 - oy + 9.75))
        # random fractional boxes on every column of the tile
        for _ in range(cap - len(rows)):
            c = int(rng.integers(0, K.TILE_W // 16))
            ya = np.round(rng.uniform(0, K.TILE_H - 20) * 8) / 8
            rows.append((rng.uniform(0.5, 1.0), 16 * c, ya, 16 * c + 15, min(ya + np.round(rng.uniform(8, 30) * 8) / 8, K.TILE_H - 1)))
        rois[t, :len(rows)] = np.array(rows, np.float32)
        counts[t] = len(rows)
    return (page_h, page_w), tiles, rois, counts


@pytest.mark.parametrize("min_size", [8.0, 16.0, 0.0])
def test_merge_equals_the_restatement(min_size):
    (page_h, page_w), tiles, rois, counts = merge_case()
    got = B.page_merge(tiles, rois, counts, page_h, page_w, min_size)
    want = R.merge(tiles, rois, counts, page_h, page_w, min_size)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    boxes, scores, src = got
    assert 0 < len(boxes) < counts.sum()                                                       # some kept, some dropped
    assert (boxes[:, 2] <= page_w - 1).all() and (boxes[:, 3] <= page_h - 1).all()
    assert (np.diff(src) > 0).all()                                                            # tile order, then roi order
    # ownership: every kept box lies in its tile's owned columns, with its centre in the owned rows
    for b, s in zip(boxes, src):
        oy, ox, vh, vw, y0, y1, x0, x1 = tiles[s // rois.shape[1]].tolist()
        assert x0 <= int(b[0]) < x1
    # the page's last column (192 .. 202) is 11 px wide after the clip: kept at min_size 8 and 0, dropped at 16
    thin = boxes[:, 0] == 192
    assert thin.any() == (min_size < 16.0) and (boxes[thin, 2] == 202).all()


def test_merge_capacity_overflow_and_argument_errors():
    (page_h, page_w), tiles, rois, counts = merge_case()
    lib = B.load_library()
    want = R.merge(tiles, rois, counts, page_h, page_w, 8.0)
    m = len(want[0])
    f32p = C.POINTER(C.c_float)
    boxes, scores, src = np.full((m - 1, 4), -1, np.float32), np.full(m - 1, -1, np.float32), np.full(m - 1, -1, np.int32)
    cnt = C.c_int(0)
    args = (tiles.ctypes.data_as(i32p), len(tiles), rois.ctypes.data_as(f32p), rois.shape[1], counts.ctypes.data_as(i32p), page_h, page_w, C.c_float(8.0))
    rc = lib.ctpn_page_merge(*args, boxes.ctypes.data_as(f32p), scores.ctypes.data_as(f32p), src.ctypes.data_as(i32p), m - 1, C.byref(cnt))
    assert rc == B.CTPN_ERR_CAPACITY and cnt.value == m
    assert np.array_equal(boxes, want[0][:m - 1]) and np.array_equal(src, want[2][:m - 1])      # what fits is written
    assert lib.ctpn_page_merge(*args, None, None, None, 0, C.byref(cnt)) == B.CTPN_ERR_CAPACITY and cnt.value == m      # sizing
    big = counts.copy()
    big[3] = rois.shape[1] + 1
    assert lib.ctpn_page_merge(args[0], args[1], args[2], args[3], big.ctypes.data_as(i32p), page_h, page_w, C.c_float(8.0), None, None, None, 0, C.byref(cnt)) == -1
    assert lib.ctpn_page_merge(*args, None, None, None, 0, None) == -1


# ---- the seam ----
def test_a_line_across_four_seams_is_one_line():
    (page_h, page_w), rois, counts, page_boxes, page_scores = K.seam_scene()
    tiles, grid = B.page_plan(page_h, page_w, K.TILE_H, K.TILE_W, K.OVERLAP)
    assert grid == (1, 5) and counts.sum() > len(page_boxes)                                   # the overlaps report their columns twice
    boxes, scores, src = B.page_merge(tiles, rois, counts, page_h, page_w, 8.0)
    assert len(boxes) == page_w // 16 and sorted(boxes[:, 0].tolist()) == [16.0 * c for c in range(page_w // 16)]      # one box per page column
    order = np.argsort(boxes[:, 0])
    assert np.array_equal(boxes[order], page_boxes) and np.array_equal(scores[order], page_scores)
    assert len(set(page_scores.tolist())) == len(page_scores) and page_scores.min() > 0.9
    for mode in "HO":
        for form in (0, 1):
            got = B.page_text_lines(boxes, scores, (page_h, page_w), mode=mode, device_id=-1, nms_form=form)
            want = B.text_lines(page_boxes, page_scores, (page_h, page_w), mode=mode, device_id=-1)
            assert got.shape == (1, 9) and got.tobytes() == want.tobytes(), (mode, form)


def test_page_text_lines_is_text_lines_cfg_on_the_host_and_checks_its_arguments():
    b = K.column_boxes(5, 400, 20, span=300.0)
    lib = B.load_library()
    for mode in "HO":
        for cfg in (None, {"MAX_HORIZONTAL_GAP": 20, "TEXT_PROPOSALS_NMS_THRESH": 0.3}):
            want = B.text_lines(b[:, :4], b[:, 4], (300, 320), mode=mode, device_id=-1, config=cfg)
            assert len(want) > 0
            for form in (0, 1):
                assert B.page_text_lines(b[:, :4], b[:, 4], (300, 320), mode=mode, device_id=-1, config=cfg, nms_form=form).tobytes() == want.tobytes()
    cnt = C.c_int(3)
    assert lib.ctpn_page_text_lines(None, None, 0, 100, 100, 0, -1, None, 2, None, 0, C.byref(cnt)) == -1      # nms_form
    assert lib.ctpn_page_text_lines(None, None, 0, 100, 100, 9, -1, None, 0, None, 0, C.byref(cnt)) == -1      # mode
    assert lib.ctpn_page_text_lines(None, None, 0, 100, 100, 0, -1, None, 1, None, 0, C.byref(cnt)) == 0 and cnt.value == 0
    assert lib.ctpn_page_text_lines(None, None, 0, 100, 100, 0, -1, None, 1, None, 0, None) == -1


# ---- the device texts under the sanitizers ----
@pytest.fixture(scope="module")
def page_program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("page_host") / "page_host")
    subprocess.run(GXX + ["-o", exe, os.path.join(root, "tests", "page_host.cpp")], check=True)
    return exe


def run_program(exe, what, tmp_path, payload):
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(payload)
    r = subprocess.run([exe, what, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.stderr == "", r.stderr[-3000:]                                                    # the sanitizers are silent
    assert r.returncode == 0, r.stdout[-2000:]
    return np.fromfile(str(tmp_path / "out.bin"), np.uint8)


@pytest.mark.parametrize("shape", [(64, 96), (100, 203), (40, 50)])
@pytest.mark.parametrize("extra", [0, 5])
def test_cut_text_under_sanitizers_equals_the_restatement(page_program, tmp_path, shape, extra):
    h, w = shape
    page = np.random.default_rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    tiles, _ = R.plan(h, w, K.TILE_H, K.TILE_W, K.OVERLAP)
    buf, view = K.pitched(page, extra, 0)
    assert buf.size == (h - 1) * (3 * w + extra) + 3 * w                                       # exactly to the last pixel's last byte
    payload = struct.pack("<iiiiiq", h, w, len(tiles), K.TILE_H, K.TILE_W, 3 * w + extra) + tiles.tobytes() + buf.tobytes()
    got = run_program(page_program, "cut", tmp_path, payload)
    want = R.cut(page, tiles, K.TILE_H, K.TILE_W)
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want)             # no 0xCD left: every byte was written


def nms_cases():
    yield "empty", np.zeros((0, 5), np.float32), 0.2, 128
    for r in (1, 63, 64, 65):
        yield "r%d_one_column" % r, K.column_boxes(r, r, 1, span=120.0), 0.2, 128
        yield "r%d_two_columns" % r, K.column_boxes(100 + r, r, 2, span=80.0), 0.7, 128
    yield "crowd300_lds64", K.column_boxes(3, 340, 4, span=3000.0, crowd=(2, 300), heights=(8.0, 12.0)), 0.2, 64
    yield "crowd300_lds128", K.column_boxes(3, 340, 4, span=3000.0, crowd=(2, 300), heights=(8.0, 12.0)), 0.2, 128
    yield "equal_scores", K.column_boxes(9, 200, 3, span=200.0, equal_scores=8), 0.2, 128
    yield "r1000_1024_columns", K.column_boxes(21, 1000, 1024, span=60.0), 0.2, 128
    for thr in (0.2, 0.7):
        yield "threshold_pairs_%g" % thr, K.threshold_pairs(thr)[0], thr, 128


@pytest.mark.parametrize("case", list(nms_cases()), ids=lambda c: c[0])
def test_column_nms_text_under_sanitizers_equals_restatement_and_oracle(page_program, tmp_path, case):
    name, b, thr, kcap = case
    payload = struct.pack("<iif", len(b), kcap, thr) + np.ascontiguousarray(b[:, :4]).tobytes()
    out = run_program(page_program, "nms", tmp_path, payload).view(np.int32)
    keep = out[1:]
    assert out[0] == len(keep)
    assert keep.tolist() == R.nms(b, thr).tolist(), name
    assert keep.tolist() == cnms.nms(b, thr) if len(b) else len(keep) == 0, name              # oracle/nms_ref.c, predicate 1; ties by index
    if name.startswith("crowd300"):
        col = (b[keep, 0] == 32).sum()
        assert col > 128 and (b[:, 0] == 32).sum() >= 300                                      # more kept boxes than either LDS capacity: the spill slice serves
    if name.startswith("threshold_pairs"):
        _, survives = K.threshold_pairs(thr)
        assert [2 * k + 1 in keep for k in range(3)] == survives == [True, True, False]


def test_the_cases_reach_the_shapes_the_texts_can_go_wrong_at():
    names = [c[0] for c in nms_cases()]
    assert len(set(names)) == len(names)
    b = dict((c[0], c[1]) for c in nms_cases())
    assert (b["r1000_1024_columns"][:, 0] == 16 * 1023).any()
    assert len(set(b["equal_scores"][:, 4].tolist())) == 25
    for thr in (0.2, 0.7):
        rows, _ = K.threshold_pairs(thr)
        ious = [K.iou32(rows[2 * k], rows[2 * k + 1]) for k in range(3)]
        t = np.float32(thr)
        assert ious == [np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))]


def test_header_rules_and_build_flags(root):
    src = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    for name, includes in (("page_dev.h", {"stddef.h", "stdint.h"}), ("nms_column_dev.h", set())):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(src, name)).read())
        assert "hip/" not in code and set(re.findall(r'#include\s+[<"]([^>"]+)[>"]', code)) == includes, name
    nms = open(os.path.join(src, "nms.hip")).read()
    assert nms.count("nms_kept_suppress(") == 2 and nms.count("nms_resolve_chunk(") == 2 and "nms_column_greedy(" in nms      # callers only: the one copy is the header's
    body = open(os.path.join(src, "nms_column_dev.h")).read()
    assert len(re.findall(r"NMS_DEV bool nms_kept_suppress\(|NMS_DEV unsigned long long nms_resolve_chunk\(", body)) == 2
    mk = open(os.path.join(src, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()
    assert "page" in srcs and "api_page" in srcs and "page_dev.h" in mk and "nms_column_dev.h" in mk
    unit = re.sub(r"//[^\n]*", "", open(os.path.join(src, "api_page.hip")).read())
    assert "ctpn_ctx" not in unit and "getenv" not in unit and "hipDeviceSynchronize" not in unit


def test_symbols_in_header_library_and_binding(root):
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    lib = B.load_library()
    declared = B._declare(C.CDLL(B.lib_path()))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, hdr) and hasattr(lib, s) and s in declared, s
    assert lib.ctpn_abi_version() == 10 and "#define CTPN_ABI_VERSION 10" in hdr      # additive
    assert declared["ctpn_page_nms"] == declared["ctpn_nms"]
    assert [len(declared[s][1]) for s in NEW_SYMBOLS] == [9, 14, 13, 7, 12]
    for name in ("page_plan", "page_cut", "page_merge", "page_nms_sorted", "page_text_lines"):
        assert callable(getattr(B, name))
    assert callable(ctpn_amd.detect_page)


def test_page_nms_domain_is_checked_before_the_device():
    good = K.column_boxes(1, 50, 8)
    for row, col, val in ((7, 2, good[7, 0] + 17.0), (7, 0, -1.0), (7, 0, 16.0 * 1024), (7, 2, good[7, 0] - 1.0), (7, 1, np.nan)):
        bad = good.copy()
        bad[row, col] = val
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.page_nms_sorted(bad, 0.2, 0)
        assert e.value.code == -1, (col, val)
    with pytest.raises(ctpn_amd.CtpnError) as e:
        B.page_nms_sorted(good, 0.05, 0)
    assert e.value.code == -1
    thin = good.copy()                                                                          # two neighbouring columns, both with a box under 10 px
    thin[0, :4] = (32.0, 5.0, 38.0, 30.0)
    thin[1, :4] = (48.0, 5.0, 56.0, 30.0)
    with pytest.raises(ctpn_amd.CtpnError) as e:
        B.page_nms_sorted(thin, 0.2, 0)
    assert e.value.code == -1
    assert B.page_nms_sorted(np.zeros((0, 5), np.float32), 0.2, 0).shape == (0,)


def test_no_device_is_an_error_not_a_cpu_fallback():
    if B.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(ctpn_amd.CtpnError) as e:
        B.page_nms_sorted(K.column_boxes(1, 50, 8), 0.2, 0)
    assert e.value.code == -5 and "no CPU fallback" in str(e.value) and "ctpn_page_nms" in str(e.value)
    tiles, _ = B.page_plan(100, 203, 64, 96, 32)
    with pytest.raises(ctpn_amd.CtpnError) as e:
        B.page_cut(np.zeros((100, 203, 3), np.uint8), tiles, 0, 9, 64, 96)
    assert e.value.code == -5 and "ctpn_page_cut" in str(e.value)


# ---- Python: the default form, the command line ----
def test_default_nms_form_follows_the_measurement_and_the_domain(root):
    import json
    from ctpn_amd import page as PG

    class Params:
        def __init__(self, thr):
            self.thr = thr

        def get_param(self, name):
            assert name == "TEXT_PROPOSALS_NMS_THRESH"
            return self.thr
    prof = json.load(open(os.path.join(root, "profiles", "page_throughput.json")))
    faster = 1 if prof["tail_ms_form1"] < prof["tail_ms_form0"] else 0
    assert PG.DEFAULT_NMS_FORM == faster == prof["default_nms_form"] and prof["tail_equal"] and prof["nms_equal"]
    assert PG.default_nms_form(Params(0.2)) == PG.DEFAULT_NMS_FORM and PG.default_nms_form(Params(0.1)) == PG.DEFAULT_NMS_FORM
    assert PG.default_nms_form(Params(0.05)) == 0                                              # below ctpn_page_nms's domain: the form that takes anything


def test_demo_page_command_line(tmp_path):
    from ctpn_amd.ctpn import demo_page
    a = demo_page.build_parser().parse_args(["--input", "x.png"])
    assert (a.factor, tuple(a.tile), a.batch, a.overlap, a.mode, a.nms_form, a.annotate) == (1.0, (608, 912), 32, 128, "H", None, False)
    a = demo_page.build_parser().parse_args(["--input", "d", "--factor", "0.5", "--nms-form", "0", "--annotate", "--mode", "O", "--tile", "64", "96"])
    assert (a.factor, a.nms_form, a.annotate, a.mode, a.tile) == (0.5, 0, True, "O", [64, 96])
    with pytest.raises(SystemExit):
        demo_page.build_parser().parse_args(["--input", "d", "--nms-form", "2"])
    (tmp_path / "b.jpg").write_bytes(b"")
    (tmp_path / "a.png").write_bytes(b"")
    (tmp_path / "notes.txt").write_bytes(b"")
    assert [os.path.basename(p) for p in demo_page.page_names(str(tmp_path))] == ["a.png", "b.jpg"]
    assert demo_page.page_names(str(tmp_path / "b.jpg")) == [str(tmp_path / "b.jpg")]
