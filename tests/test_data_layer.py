"""CPU: the training data layer (include/ctpn_hip_data_layer.h: ctpn_split_labels, ctpn_train_page, ctpn_train_boxes; ctpn_amd.data_layer) before it
reaches a GPU. Every comparison is bit for bit.

  * tests/data_layer_ref.py, the numpy restatement, is held first: against the strips the reference's own split_label.py wrote and the
    indices its RoIDataLayer served (tests/golden/data_layer.npz, written by tools/make_data_layer_golden.py), the quirk table row by row,
    and the flip against a literal numpy uint16 evaluation, wrap and clamp included;
  * csrc/data_layer_dev.h, the kernels' per-thread text, compiled with g++ -ffp-contract=off under ASan + UBSan as a stand-alone program
    (tests/data_layer_host.cpp) and run over exact-size heap blocks: split, page and box bodies equal the restatement and
    oracle/resize_ref.py; five mutants each fail that comparison;
  * DataLayer's order under device-free stubs; the label parser's errors; the symbols in header, library and binding, the ABI still 10;
    bad arguments refused before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ctpn_amd
import data_layer_ref as R
from data_layer_cases import PAGE_CASES, big_label_set, label_set
from ctpn_amd import _binding as B
from ctpn_amd import data_layer as DL
from oracle import resize_ref

GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all"]
NEW = ("ctpn_split_labels", "ctpn_train_page", "ctpn_train_boxes")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "text-detection-ctpn_amd", "csrc")
# (xmin, xmax) -> the (x1, x2) strips: the table of include/ctpn_hip_data_layer.h
QUIRKS = [((5, 100), [(5, 15), (16, 31), (32, 47), (48, 63), (64, 79), (80, 95), (96, 100)]), ((3, 17), [(3, 15), (16, 17)]), ((16, 33), [(16, 31), (32, 33)]),
          ((31, 48), [(32, 48)]), ((3, 10), [(3, 15)]), ((3, 15), [(3, 15)]), ((3, 16), [(3, 15)]), ((16, 32), [(16, 31)]), ((15, 16), []), ((7, 7), [])]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "data_layer.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("data_layer_host") / "data_layer_host")
    subprocess.run(GXX + ["-I", CSRC, os.path.join(HERE, "data_layer_host.cpp"), "-o", exe], check=True)
    return exe


# ---- the restatement against the reference's recorded results
def test_the_restatement_equals_the_references_strips(golden):
    dims, quads, offs, want, want_offs = label_set(golden)
    assert quads.shape[0] >= 40 and dims.shape[0] >= 4
    got, got_offs, _ = R.split_labels(dims, quads, offs)
    assert got_offs.tolist() == want_offs.tolist()
    assert got.tobytes() == want.tobytes()
    for p in range(dims.shape[0]):      # the sizes and factors the reference's script worked with are split_label_dims'
        f, (rh, rw) = ctpn_amd.split_label_dims(int(dims[p, 0]), int(dims[p, 1]))
        assert (rh, rw) == (int(dims[p, 2]), int(dims[p, 3])) and f == float(golden["factors"][p])


def test_the_fixture_covers_the_quirk_table(golden):
    """page_a is 600 x 1024 at factor 1: a rectangle's x1, x2 are xmin, xmax exactly, and its first lines are the table's rows"""
    got = golden["strips_page_a"]
    k = 0
    for (xmin, xmax), strips in QUIRKS[:-1]:
        assert [(int(r[0]), int(r[2])) for r in got[k: k + len(strips)]] == strips, (xmin, xmax)
        k += len(strips)
    assert golden["strips_page_e"][:, 2].tolist() == [15, 15] and int(golden["page_dims"][4, 3]) == 12      # x2 = 15 on a page 12 wide


@pytest.mark.parametrize("span,strips", QUIRKS)
def test_the_strip_rule_row_by_row(span, strips):
    assert R.strips_x(*span) == strips


def test_the_restatement_equals_the_references_order(golden):
    assert bool(golden["order_from_reference"])
    for n in (1, 2, 3, 8):
        assert [i for i, _ in R.order(n, 3, 40)] == golden["order_%d" % n].tolist(), n
    # the last entry of every permutation is never served: in 7-long runs of a length-8 order no index repeats
    inds = [i for i, _ in R.order(8, 3, 70)]
    assert all(len(set(inds[k: k + 7])) == 7 for k in range(0, 70, 7))
    # more than one scale: the draw comes after the index and moves the generator
    assert [i for i, _ in R.order(8, 3, 40, n_scales=2)] != inds[:40]


def test_the_flip_equals_a_literal_uint16_evaluation():
    rs = np.random.RandomState(5)
    boxes = rs.randint(0, 1300, size=(200, 4)).astype(np.uint16)
    boxes[:, 2] = np.maximum(boxes[:, 0], boxes[:, 2])
    boxes[:4] = [[3, 20, 15, 90], [6, 0, 15, 9], [0, 0, 11, 5], [0, 0, 65535, 1]]      # x2 = 15 on a page 12 wide: the wrap, then the clamp
    for width in (12, 1200, 65535):
        lit = boxes.copy()
        oldx1, oldx2 = lit[:, 0].copy(), lit[:, 2].copy()
        with np.errstate(over="ignore"):
            lit[:, 0] = np.uint16(width) - oldx2 - np.uint16(1)
            lit[:, 2] = np.uint16(width) - oldx1 - np.uint16(1)
        assert lit.dtype == np.uint16
        for b in range(len(lit)):
            if lit[b][2] < lit[b][0]:
                lit[b][0] = 0
        got = R.flip_boxes(boxes, width)
        assert got.dtype == np.uint16 and np.array_equal(got, lit), width
    wrapped = R.flip_boxes(boxes[:1], 12)
    assert wrapped.tolist() == [[0, 20, 8, 90]]      # x1' = 12 - 15 - 1 wraps to 65532 > x2' = 8, so x1' = 0
    out = R.train_boxes(boxes[:4].astype(np.float32), 12, True, 1000.0 / 1200.0)
    assert out.dtype == np.float32 and out[0].tolist() == [0.0, float(np.float32(20 * (1000.0 / 1200.0))), float(np.float32(8 * (1000.0 / 1200.0))), 75.0, 1.0]


# ---- the kernels' text on the host
def run_split(exe, dims, quads, offs, tmp, mutant=0):
    src, dst = os.path.join(tmp, "split_in.bin"), os.path.join(tmp, "split_out.bin")
    pages, nq = int(np.asarray(dims).reshape(-1, 4).shape[0]), int(np.asarray(quads).reshape(-1, 8).shape[0])
    with open(src, "wb") as f:
        f.write(np.array([pages, nq], np.int32).tobytes())
        f.write(np.ascontiguousarray(dims, np.int32).tobytes())
        f.write(np.ascontiguousarray(offs, np.int32).tobytes())
        f.write(np.ascontiguousarray(quads, np.float64).tobytes())
    r = subprocess.run([exe, "split", src, dst] + ([str(mutant)] if mutant else []), stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    raw = np.fromfile(dst, np.int32)
    total = int(raw[0])
    poffs, scan = raw[1: 2 + pages], raw[2 + pages: 3 + pages + nq]
    strips = raw[3 + pages + nq:].view(np.float32).reshape(total, 4)
    return strips, poffs, scan


def run_page(exe, img, factor, flip, tmp, offset=0, pad=0, mutant=0):
    """img goes in with rows 3 w + pad bytes apart, `offset` bytes into its heap block"""
    src, dst = os.path.join(tmp, "page_in.bin"), os.path.join(tmp, "page_out.bin")
    h, w = img.shape[:2]
    pitch = 3 * w + pad
    oh, ow = (resize_ref.out_dim(h, factor), resize_ref.out_dim(w, factor)) if (factor > 0 and factor != 1) else (h, w)
    rows = np.full((h, pitch), 0xA5, np.uint8)
    rows[:, : 3 * w] = img.reshape(h, 3 * w)
    with open(src, "wb") as f:
        f.write(np.array([h, w, pitch, offset, int(flip), oh, ow, 0], np.int32).tobytes())
        f.write(np.array([factor], np.float64).tobytes())
        f.write(rows.reshape(-1)[: (h - 1) * pitch + 3 * w].tobytes())
    r = subprocess.run([exe, "page", src, dst] + ([str(mutant)] if mutant else []), stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    raw = open(dst, "rb").read()
    n = oh * ow * 3
    return np.frombuffer(raw[:n], np.uint8).reshape(oh, ow, 3), np.frombuffer(raw[n:], np.float32).reshape(oh, ow, 3)


def run_boxes(exe, strips, width, flip, scale, tmp, mutant=0):
    src, dst = os.path.join(tmp, "boxes_in.bin"), os.path.join(tmp, "boxes_out.bin")
    s = np.ascontiguousarray(strips, np.float32).reshape(-1, 4)
    with open(src, "wb") as f:
        f.write(np.array([s.shape[0], width, int(flip), 0], np.int32).tobytes())
        f.write(np.array([scale], np.float64).tobytes())
        f.write(s.tobytes())
    r = subprocess.run([exe, "boxes", src, dst] + ([str(mutant)] if mutant else []), stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    raw = open(dst, "rb").read()
    return int(np.frombuffer(raw[:4], np.int32)[0]), np.frombuffer(raw[4:], np.float32).reshape(-1, 5)


def test_split_body_equals_the_restatement(program, golden, tmp_path):
    dims, quads, offs, want, want_offs = label_set(golden)
    got, poffs, scan = run_split(program, dims, quads, offs, str(tmp_path))
    assert poffs.tolist() == want_offs.tolist() and got.tobytes() == want.tobytes()
    assert scan.tolist() == R.split_labels(dims, quads, offs)[2].tolist()
    dims2, quads2, offs2 = big_label_set(golden)
    want2 = R.split_labels(dims2, quads2, offs2)
    got2 = run_split(program, dims2, quads2, offs2, str(tmp_path))
    assert want2[0].shape[0] > 2048 and want2[2][-1] == want2[2][-2]
    assert got2[0].tobytes() == want2[0].tobytes() and got2[1].tolist() == want2[1].tolist() and got2[2].tolist() == want2[2].tolist()


@pytest.mark.parametrize("h,w,factor", PAGE_CASES)
def test_page_body_equals_resize_then_mirror(program, h, w, factor, tmp_path):
    img = np.random.RandomState(h * 100 + w).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    for flip in (0, 1):
        want_img, want_blob = R.train_page(img, factor, flip)
        for offset in range(4):
            got_img, got_blob = run_page(program, img, factor, flip, str(tmp_path), offset=offset, pad=1)
            assert got_img.tobytes() == want_img.tobytes(), (flip, offset)
            assert got_blob.tobytes() == want_blob.tobytes(), (flip, offset)
    if factor == 0.5:      # factor <= 0 means no resize, like 1
        assert run_page(program, img, 0.0, 1, str(tmp_path))[0].tobytes() == np.ascontiguousarray(img[:, ::-1]).tobytes()


def test_box_body_equals_the_restatement(program, tmp_path):
    rs = np.random.RandomState(3)
    strips = rs.randint(0, 1200, size=(1000, 4)).astype(np.float32)
    strips[:3] = [[3, 20, 15, 90], [0, 0, 65535, 65535], [1184, 5, 1199, 599]]
    for width, flip, scale in ((12, 1, 1.0), (1200, 1, 1000.0 / 1200.0), (1200, 0, 1000.0 / 1200.0), (933, 1, 0.7779)):
        ok, got = run_boxes(program, strips, width, flip, scale, str(tmp_path))
        assert ok == 1 and got.tobytes() == R.train_boxes(strips, width, flip, scale).tobytes(), (width, flip, scale)
    assert run_boxes(program, strips[:0], 12, 1, 1.0, str(tmp_path))[1].shape == (0, 5)
    for bad in (-1.0, 65536.0, np.nan):
        s = strips[:5].copy()
        s[3, 2] = bad
        assert run_boxes(program, s, 1200, 1, 1.0, str(tmp_path))[0] == 0


def test_mutants_fail_the_comparison(program, golden, tmp_path):
    """1 the input mirrored instead of the output, 2 `<= xmax` in the strip walk, 3 a signed flip without the wrap, 4 multiply before dividing in
    the scaling, 5 an unstable tie order: each changes bytes the unmutated program shares with the restatement"""
    tmp = str(tmp_path)
    # 1: at 31 x 45 by 1.37 the float32 sample positions of column dx and of its mirror image are not mirror images, so the two orders differ
    # -- shown first with oracle/resize_ref.py alone
    img = np.random.RandomState(3145).randint(0, 256, size=(31, 45, 3)).astype(np.uint8)
    after = np.flip(resize_ref.resize_linear(img, 1.37, 1.37), axis=1)
    before = resize_ref.resize_linear(np.ascontiguousarray(np.flip(img, axis=1)), 1.37, 1.37)
    assert after.shape == before.shape and not np.array_equal(after, before)
    good, bad = run_page(program, img, 1.37, 1, tmp)[0], run_page(program, img, 1.37, 1, tmp, mutant=1)[0]
    assert good.tobytes() == np.ascontiguousarray(after).tobytes() and bad.tobytes() == before.tobytes()
    # 2, 4, 5 on the fixture: the reference's own strips kill them
    dims, quads, offs, want, want_offs = label_set(golden)
    assert run_split(program, dims, quads, offs, tmp)[0].tobytes() == want.tobytes()
    for mutant in (2, 4, 5):
        got, poffs, _ = run_split(program, dims, quads, offs, tmp, mutant)
        assert poffs.tolist() != want_offs.tolist() or got.tobytes() != want.tobytes(), mutant
    # 3: x2 = 15 on a page 12 wide
    strips = np.array([[3, 20, 15, 90], [0, 1, 5, 9]], np.float32)
    want_b = R.train_boxes(strips, 12, True, 1.0)
    assert run_boxes(program, strips, 12, 1, 1.0, tmp)[1].tobytes() == want_b.tobytes()
    assert run_boxes(program, strips, 12, 1, 1.0, tmp, mutant=3)[1].tobytes() != want_b.tobytes()


# ---- the layer's order, device-free
class FakeStrips(object):
    def __getitem__(self, key):
        return ("strips", key.start, key.stop)


@pytest.fixture
def stubbed(monkeypatch):
    """DataLayer with its three device calls and its file reads replaced: what is left is the order, the factors and the bookkeeping"""
    from ctpn_amd.lib.utils import image as imutil
    sizes = {"a.png": (600, 1024), "b.png": (900, 1400), "c.png": (500, 1500), "d.png": (375, 500)}
    calls = []
    monkeypatch.setattr(imutil, "image_size", lambda p: sizes[os.path.basename(p)])

    def imread(p):
        h, w = sizes[os.path.basename(p)]
        return np.zeros((h, w, 3), np.uint8)
    monkeypatch.setattr(imutil, "imread", imread)

    def split_labels(dims, quads, offs, device_id=0, on_device=False):
        calls.append(("split", np.array(dims), np.array(offs)))
        return FakeStrips(), np.arange(len(offs), dtype=np.int32) * 10

    def train_page(image, factor, flip=False, device_id=0, want_blob=True):
        calls.append(("page", tuple(image.shape[:2]), factor, bool(flip), want_blob))
        h, w = image.shape[:2]
        oh, ow = B.resize_dims(h, w, factor, factor) if factor != 1.0 else (h, w)
        return np.zeros((oh, ow, 3), np.uint8), (np.zeros((oh, ow, 3), np.float32) if want_blob else None)

    def train_boxes(strips, page_width, flip=False, scale=1.0, device_id=0):
        calls.append(("boxes", strips, page_width, bool(flip), scale))
        return np.zeros((10, 5), np.float32)
    monkeypatch.setattr(DL, "split_labels", split_labels)
    monkeypatch.setattr(DL, "train_page", train_page)
    monkeypatch.setattr(DL, "train_boxes", train_boxes)
    return sorted(sizes), calls


@pytest.mark.parametrize("pages,flipped,length", [(1, False, 1), (1, True, 2), (3, False, 3), (4, True, 8)])
@pytest.mark.parametrize("prefetch", [False, True])
def test_the_layers_order_is_the_references(stubbed, golden, pages, flipped, length, prefetch):
    names, calls = stubbed
    quads = [np.zeros((2, 8))] * pages
    with DL.DataLayer(0, names[:pages], quads, flipped=flipped, seed=3, prefetch=prefetch) as layer:
        recs = [layer.next() for _ in range(40)]
    want = golden["order_%d" % length].tolist()
    assert [r.page + (pages if r.flipped else 0) for r in recs] == want
    assert [c[0] for c in calls].count("split") == 1      # the label database is built once, at construction
    boxes = [c for c in calls if c[0] == "boxes"]
    for r, c in zip(recs, boxes):      # the page's slice of the resident strips, its resized width, its flip, the second factor
        assert c[1] == ("strips", 10 * r.page, 10 * r.page + 10) and c[3] == r.flipped and c[4] == r.im_scale
        assert c[2] == int(layer.page_dims[r.page, 3])


def test_the_layers_second_pass_follows_prep_im_for_blob(stubbed):
    names, calls = stubbed
    with DL.DataLayer(0, names, [np.zeros((1, 8))] * 4, flipped=True, seed=3, prefetch=False) as layer:
        assert layer.page_dims.tolist() == [[600, 1024, 600, 1024], [900, 1400, 600, 933], [500, 1500, 400, 1200], [375, 500, 600, 800]]
        assert layer.max_shape() == (600, 1000)
        del calls[:]
        recs = [layer.next() for _ in range(14)]
    pages = [c for c in calls if c[0] == "page"]
    k = 0
    for r in recs:
        first = pages[k]
        assert first[1] == tuple(layer.page_dims[r.page, :2]) and first[2] == layer.factors[r.page] and first[3] == r.flipped
        if r.page in (0, 2):      # 600 x 1024 -> the long side is capped at 1000; 400 x 1200 -> 600 / 400 = 1.5 would give 1800: capped too
            second = pages[k + 1]
            assert first[4] is False and second[1] == tuple(layer.page_dims[r.page, 2:]) and second[3] is False and second[4] is True
            assert r.im_scale == 1000.0 / max(layer.page_dims[r.page, 2:]) and second[2] == r.im_scale
            k += 2
        else:
            assert first[4] is True and r.im_scale == 1.0
            k += 1
        assert r.hw == layer.page_shape(r.page)
    assert k == len(pages) and {r.page for r in recs} == {0, 1, 2, 3}


def test_the_label_parsers_errors_name_the_file_and_the_line(tmp_path):
    p = tmp_path / "gt_page_1.txt"
    p.write_text("﻿377,117,463,117,465,130,378,130,Genaxis Theatre\n\n 1.5,2,3,4,5,6,7,8 \n", encoding="utf-8")
    q = DL.read_quads(str(p))
    assert q.dtype == np.float64 and q.tolist() == [[377, 117, 463, 117, 465, 130, 378, 130], [1.5, 2, 3, 4, 5, 6, 7, 8]]
    for text, line in (("1,2,3,4,5,6,7,8\n1,2,3,4,5,6,7\n", 2), ("1,2,3,4,5,6,7,8\n\n1,2,x,4,5,6,7,8\n", 3), ("1,2,3,4,5,6,7,nan\n", 1)):
        p.write_text(text)
        with pytest.raises(ValueError, match=re.escape("%s:%d:" % (str(p), line))):
            DL.read_quads(str(p))
    assert DL.quad_label_path(str(tmp_path), "/x/page_1.jpg") == str(p) and DL.quad_label_path(str(tmp_path), "/x/page_2.jpg") is None


# ---- the ABI
def test_the_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctpn_hip_data_layer.h")).read()
    assert '#include "ctpn_hip_data_layer.h"' in open(os.path.join(ROOT, "include", "ctpn_hip_train.h")).read()      # they come with the training-side header
    lib = ctpn_amd.load_library()
    sig = B._declare_data_layer(lib)
    assert sorted(sig) == sorted(NEW) and not set(sig) & (set(B._declare(lib)) | set(B._declare_train(lib)))
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(lib, name) is not None and name in sig
    assert lib.ctpn_abi_version() == 10
    assert re.search(r"#define\s+CTPN_ABI_VERSION\s+10\b", open(os.path.join(ROOT, "include", "ctpn_hip.h")).read())
    for name in ("split_labels", "split_label_dims", "train_page", "train_boxes", "DataLayer"):
        assert hasattr(ctpn_amd, name)


def test_bad_arguments_are_refused_before_any_device_work():
    lib = ctpn_amd.load_library()
    i32p = C.POINTER(C.c_int)
    dims = np.array([[600, 800, 600, 800]], np.int32)
    offs, soffs = np.array([0, 1], np.int32), np.zeros(2, np.int32)
    quads = np.zeros((1, 8), np.float64)
    strips = np.zeros((8, 4), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    split = lambda pages=1, d=dims, q=quads, o=offs, on=0, s=strips, cap=8, so=soffs: lib.ctpn_split_labels(      # noqa: E731
        0, pages, None if d is None else d.ctypes.data_as(i32p), None if q is None else p(q), None if o is None else o.ctypes.data_as(i32p), on,
        None if s is None else p(s), cap, None if so is None else so.ctypes.data_as(i32p), None)
    assert split(pages=0) == -1 and split(d=None) == -1 and split(o=None) == -1 and split(so=None) == -1 and split(q=None) == -1
    assert split(on=2) == -1 and split(cap=-1) == -1 and split(s=None) == -1
    assert split(o=np.array([1, 1], np.int32)) == -1 and split(o=np.array([0, -1], np.int32)) == -1
    assert split(d=np.array([[600, 800, 0, 800]], np.int32)) == -1 and split(d=np.array([[600, 800, 600, 65536]], np.int32)) == -1
    img, out, blob = np.zeros((20, 32, 3), np.uint8), np.zeros((20, 32, 3), np.uint8), np.zeros((20 * 32 * 3 + 1,), np.float32)
    page = lambda im=img, on=0, h=20, w=32, pitch=96, f=1.0, flip=0, o=out, b=None, oh=20, ow=32: lib.ctpn_train_page(      # noqa: E731
        0, None if im is None else p(im), on, h, w, pitch, f, flip, None if o is None else p(o), b, oh, ow)
    assert page(im=None) == -1 and page(o=None) == -1 and page(h=0) == -1 and page(w=0) == -1 and page(pitch=95) == -1
    assert page(on=2) == -1 and page(flip=2) == -1 and page(oh=21) == -1 and page(f=0.5) == -1 and page(f=0.5, oh=10, ow=17) == -1
    assert page(f=float("inf")) == -1 and page(b=C.c_void_p(blob.ctypes.data + 2)) == -1
    boxes = lambda s=strips, g=8, w=100, flip=0, scale=1.0, on=0, o=np.zeros((8, 5), np.float32): lib.ctpn_train_boxes(      # noqa: E731
        0, None if s is None else p(s), g, w, flip, scale, on, None if o is None else p(o))
    assert boxes(g=-1) == -1 and boxes(w=0) == -1 and boxes(w=65536) == -1 and boxes(flip=2) == -1 and boxes(on=2) == -1
    assert boxes(scale=float("nan")) == -1 and boxes(s=None) == -1 and boxes(o=None) == -1
    bad = strips.copy()
    bad[5, 2] = 65536.0
    assert boxes(s=bad) == -1 and b"uint16" in lib.ctpn_last_error()
    # well-formed calls get as far as the device: without one the answer is CTPN_ERR_NODEVICE, never a host fallback
    if lib.ctpn_device_count() <= 0:
        assert split() == -5 and page() == -5 and boxes() == -5
