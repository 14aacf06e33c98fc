"""GPU: the training data layer (include/ctpn_hip_data_layer.h: ctpn_split_labels, ctpn_train_page, ctpn_train_boxes; ctpn_amd.DataLayer,
Trainer.step_record, ctpn/train_net.py --data-layer) against tests/data_layer_ref.py and oracle/resize_ref.py, which tests/test_data_layer.py
holds on the CPU. Every comparison is bit for bit.

  * split_labels: the fixture's pages, an empty page between two others, a page of 301 quads (two workgroups of the count kernel, strips
    past one 2048-wide run of the scan), host and device arrays, the probe, CTPN_ERR_CAPACITY one strip short with canaries untouched;
  * train_page: the five shapes of data_layer_cases.PAGE_CASES x flip x host / device source; a device source at pointer offsets 1 .. 3 with
    pitch 3 w + 1; outputs at a 4-byte-only alignment (and image_out at an odd address); canaries after both outputs;
  * train_boxes: G = 0, 1, 1000, the uint16 wrap, two scales, host and device arrays, a strip outside uint16 on the device;
  * DataLayer: prefetch on equals prefetch off; records equal a host composition (imread, ctpn_resize, np.flip, the restatement), with
    and without the second pass; a Momentum Trainer.step_record run equals Trainer.step fed the host composition's arrays; pages of sizes
    A, B, A on one ctx equal the same pages on a fresh ctx per size; nothing is left live after close();
  * train_net.main --data-layer in process, twice; the same folder without the flag still stops at the one-size message.

The folder's four pages resize to 48 x 80 and 32 x 80 (files of 96 x 160 and 64 x 160 under a 48 / 80 rule, the second by its cap). One
rule -- the short side to a target, the long side capped -- cannot give 48 x 80 and 32 x 48 at once, so the second size differs from the
first in its height alone; the feature maps are 3 x 5 and 2 x 5."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ctpn_amd
import data_layer_ref as R
from ctpn_amd import _binding as B
from ctpn_amd import data_layer as DL
from ctpn_amd import solver as S
from conv_grad_cases import net_cfg
from data_layer_cases import PAGE_CASES, big_label_set, label_set

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 1234.5


def live():
    out = (C.c_longlong * 4)()
    B.load_library().ctpn_debug_live_resources(out)
    return list(out)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "data_layer.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- split_labels
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("which", ["fixture", "big"])
def test_split_labels_equals_the_restatement(golden, which, on_device):
    if which == "fixture":
        dims, quads, offs, want, want_offs = label_set(golden)
        ref = R.split_labels(dims, quads, offs)
        assert ref[0].tobytes() == want.tobytes() and ref[1].tolist() == want_offs.tolist()
    else:
        dims, quads, offs = big_label_set(golden)
        ref = R.split_labels(dims, quads, offs)
        assert ref[0].shape[0] > 2048 and quads.shape[0] > 256 and ref[1][1] == ref[1][2]
    before = live()
    strips, soffs, qso = ctpn_amd.split_labels(dims, quads, offs, 0, on_device=on_device, want_quad_offsets=True)
    if on_device:
        assert strips.device == torch.device(DEV) and qso.device == torch.device(DEV)
        strips, qso = strips.cpu().numpy(), qso.cpu().numpy()
    assert soffs.tolist() == ref[1].tolist() and qso.tolist() == ref[2].tolist()
    assert strips.dtype == np.float32 and strips.tobytes() == ref[0].tobytes()
    assert live() == before


def test_split_labels_probe_and_capacity(golden):
    dims, quads, offs, want, want_offs = label_set(golden)
    lib = B.load_library()
    i32p = C.POINTER(C.c_int)
    total = int(want_offs[-1])
    for on_device in (0, 1):
        soffs = np.full(len(offs), -1, np.int32)
        buf = torch.full((total + 2, 4), CANARY, dtype=torch.float32, device=DEV) if on_device else np.full((total + 2, 4), CANARY, np.float32)
        q = torch.from_numpy(quads).to(DEV) if on_device else quads
        pq = C.c_void_p(q.data_ptr()) if on_device else q.ctypes.data_as(C.c_void_p)
        pb = C.c_void_p(buf.data_ptr()) if on_device else buf.ctypes.data_as(C.c_void_p)
        host = lambda: buf.cpu().numpy() if on_device else buf      # noqa: E731
        call = lambda p, cap: lib.ctpn_split_labels(0, len(dims), np.ascontiguousarray(dims, np.int32).ctypes.data_as(i32p), pq, offs.ctypes.data_as(i32p),      # noqa: E731
                                                    on_device, p, cap, soffs.ctypes.data_as(i32p), None)
        torch.cuda.synchronize()
        assert call(pb, 0) == 0 and soffs.tolist() == want_offs.tolist() and (host() == CANARY).all()      # the probe: offsets, nothing else
        assert call(None, 0) == 0
        soffs[:] = -1
        assert call(pb, total - 1) == -4 and soffs.tolist() == want_offs.tolist() and (host() == CANARY).all()      # one strip short
        assert call(pb, total) == 0
        back = host()
        assert back[:total].tobytes() == want.tobytes() and (back[total:] == CANARY).all()
    # no quads at all: offsets of zeros, no strips
    strips, soffs = ctpn_amd.split_labels(dims[:2], np.zeros((0, 8)), [0, 0, 0], 0)
    assert strips.shape == (0, 4) and soffs.tolist() == [0, 0, 0]


# ---- train_page
def page_call(src_ptr, on_device, h, w, pitch, factor, flip, oh, ow, img_off=0, blob_off=0, want_blob=True):
    """ctpn_train_page into canaried device buffers, the outputs img_off / blob_off bytes into them -> (image, blob, both tails)"""
    n = oh * ow * 3
    ibuf = torch.full((img_off + n + 32,), 0x5A, dtype=torch.uint8, device=DEV)
    bbuf = torch.full((blob_off // 4 + n + 8,), CANARY, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    rc = B.load_library().ctpn_train_page(0, C.c_void_p(src_ptr), on_device, h, w, pitch, factor, flip, C.c_void_p(ibuf.data_ptr() + img_off),
                                          C.c_void_p(bbuf.data_ptr() + blob_off) if want_blob else None, oh, ow)
    B._check(rc)
    ib, bb = ibuf.cpu().numpy(), bbuf.cpu().numpy()
    assert (ib[:img_off] == 0x5A).all() and (ib[img_off + n:] == 0x5A).all(), "bytes outside image_out were written"
    assert (bb[: blob_off // 4] == CANARY).all() and (bb[blob_off // 4 + n:] == CANARY).all(), "floats outside blob_out were written"
    if not want_blob:
        assert (bb == CANARY).all()
    return ib[img_off: img_off + n].reshape(oh, ow, 3), bb[blob_off // 4: blob_off // 4 + n].reshape(oh, ow, 3)


@pytest.mark.parametrize("h,w,factor", PAGE_CASES)
def test_train_page_equals_resize_then_mirror(h, w, factor):
    img = np.random.RandomState(h * 100 + w).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    oh, ow = B.resize_dims(h, w, factor, factor) if factor != 1.0 else (h, w)
    plain = ctpn_amd._binding.resize_linear(img, factor, factor) if factor != 1.0 else img      # ctpn_resize
    before = live()
    for flip in (0, 1):
        want_img, want_blob = R.train_page(img, factor, flip)
        assert want_img.tobytes() == np.ascontiguousarray(np.flip(plain, axis=1) if flip else plain).tobytes()      # np.flip(ctpn_resize(...))
        # the host source; the Python wrapper
        got_img, got_blob = page_call(img.ctypes.data, 0, h, w, 3 * w, factor, flip, oh, ow)
        assert got_img.tobytes() == want_img.tobytes() and got_blob.tobytes() == want_blob.tobytes(), flip
        t_img, t_blob = ctpn_amd.train_page(img, factor, bool(flip), 0)
        assert t_img.device == torch.device(DEV) and t_img.cpu().numpy().tobytes() == want_img.tobytes() and t_blob.cpu().numpy().tobytes() == want_blob.tobytes()
        # the device source, dense and then at pointer offsets 1 .. 3 with rows 3 w + 1 bytes apart
        dense = torch.from_numpy(img).to(DEV)
        d_img, d_blob = ctpn_amd.train_page(dense, factor, bool(flip), 0)
        assert d_img.cpu().numpy().tobytes() == want_img.tobytes() and d_blob.cpu().numpy().tobytes() == want_blob.tobytes()
        pitch = 3 * w + 1
        rows = np.full((h, pitch), 0xA5, np.uint8)
        rows[:, : 3 * w] = img.reshape(h, 3 * w)
        for off in (1, 2, 3):
            block = torch.zeros((off + h * pitch,), dtype=torch.uint8, device=DEV)
            block[off:] = torch.from_numpy(rows.reshape(-1)).to(DEV)
            got_img, got_blob = page_call(block.data_ptr() + off, 1, h, w, pitch, factor, flip, oh, ow, img_off=4 * off, blob_off=4 * off)
            assert got_img.tobytes() == want_img.tobytes() and got_blob.tobytes() == want_blob.tobytes(), (flip, off)
        # the host source with that pitch; image_out at an odd address; no blob
        got_img, _ = page_call(rows.ctypes.data, 0, h, w, pitch, factor, flip, oh, ow, img_off=1 + 2 * flip, want_blob=False)
        assert got_img.tobytes() == want_img.tobytes()
    del dense, block, t_img, t_blob, d_img, d_blob
    assert live() == before
    lib = B.load_library()
    out = torch.zeros((oh + 1, ow, 3), dtype=torch.uint8, device=DEV)
    assert lib.ctpn_train_page(0, C.c_void_p(img.ctypes.data), 0, h, w, 3 * w, factor, 0, C.c_void_p(out.data_ptr()), None, oh + 1, ow) == -1


# ---- train_boxes
@pytest.mark.parametrize("g", [0, 1, 1000])
def test_train_boxes_equals_the_restatement(g):
    rs = np.random.RandomState(g)
    strips = rs.randint(0, 1200, size=(g, 4)).astype(np.float32)
    if g:
        strips[0] = [3, 20, 15, 90]      # x2 = 15 on a page 12 wide
    for width, flip, scale in ((12, True, 1.0), (12, True, 1000.0 / 1200.0), (1200, True, 1000.0 / 1200.0), (1200, False, 1.0), (1200, False, 1000.0 / 1200.0)):
        want = R.train_boxes(strips, width, flip, scale)
        got = ctpn_amd.train_boxes(strips, width, flip, scale, 0)
        assert got.dtype == np.float32 and got.shape == (g, 5) and got.tobytes() == want.tobytes(), (width, flip, scale)
        dev = ctpn_amd.train_boxes(torch.from_numpy(strips).to(DEV), width, flip, scale, 0)
        assert dev.device == torch.device(DEV) and tuple(dev.shape) == (g, 5) and dev.cpu().numpy().tobytes() == want.tobytes(), (width, flip, scale)
    if g == 1:
        assert ctpn_amd.train_boxes(strips, 12, True, 1.0, 0).tolist() == [[0.0, 20.0, 8.0, 90.0, 1.0]]      # wrapped, then clamped
    if g == 1000:      # device strips cannot be read before the device work: the kernel finds the value and leaves that row alone
        bad = strips.copy()
        bad[700, 2] = 65536.0
        out = torch.full((g, 5), CANARY, dtype=torch.float32, device=DEV)
        t = torch.from_numpy(bad).to(DEV)
        torch.cuda.synchronize()
        lib = B.load_library()
        assert lib.ctpn_train_boxes(0, C.c_void_p(t.data_ptr()), g, 1200, 1, 1.0, 1, C.c_void_p(out.data_ptr())) == -1
        assert b"uint16" in lib.ctpn_last_error() and (out[700].cpu().numpy() == CANARY).all()
        with pytest.raises(ctpn_amd.CtpnError):
            ctpn_amd.train_boxes(bad, 1200, True, 1.0, 0)


# ---- DataLayer and Trainer
RULE = dict(label_scale=48, label_max_size=80, scales=(48,), max_size=80)
SIZES = [(96, 160), (64, 160), (96, 160), (64, 160)]


def folder_quads(h, w, k):
    """two text rows of page k in file coordinates: a rectangle and a slanted quadrilateral given from another corner"""
    a = [0.125 * w + k, 0.2 * h, 0.75 * w, 0.2 * h + 1, 0.75 * w + 2, 0.45 * h, 0.125 * w, 0.45 * h]
    b = [0.9 * w, 0.85 * h, 0.3 * w + k, 0.8 * h, 0.3 * w, 0.6 * h, 0.9 * w + 1.5, 0.62 * h]
    return np.array([a, b], np.float64)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """IMAGES, LABELS: four synthetic PNG pages of two sizes; LABELS holds gt_<stem>.txt quadrilaterals and, for the run without the data
    layer, <stem>.txt strips in the older format"""
    from PIL import Image
    d = tmp_path_factory.mktemp("data_layer_folder")
    (d / "images").mkdir()
    (d / "labels").mkdir()
    paths, quads = [], []
    for k, (h, w) in enumerate(SIZES):
        img = ctpn_amd.weights.synthetic_images(1, h, w, 40 + k)[0]
        p = d / "images" / ("page_%d.png" % k)
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(str(p))
        q = folder_quads(h, w, k)
        (d / "labels" / ("gt_page_%d.txt" % k)).write_text("".join(",".join(repr(float(v)) for v in row) + ",text\n" for row in q))
        (d / "labels" / ("page_%d.txt" % k)).write_text("text\t16\t10\t31\t30\n")
        paths.append(str(p))
        quads.append(q)
    return d, paths, quads


def host_record(path, quads, flip, rule, scale_ind=0):
    """the host composition of one record: imread, ctpn_resize, np.flip, the restatement -> (image, blob, gt, im_scale)"""
    from ctpn_amd.lib.utils import image as imutil
    img = imutil.imread(path)
    h, w = img.shape[:2]
    f, (rh, rw) = ctpn_amd.split_label_dims(h, w, rule["label_scale"], rule["label_max_size"])
    page = B.resize_linear(img, f, f) if f != 1.0 else img
    assert page.shape[:2] == (rh, rw)
    if flip:
        page = np.ascontiguousarray(np.flip(page, axis=1))
    second = DL.prep_scale(rh, rw, rule["scales"][scale_ind], rule["max_size"])
    if second != 1.0:
        page = B.resize_linear(page, second, second)
    blob = (page.astype(np.float64) - R.PIXEL_MEANS).astype(np.float32)
    strips = R.split_labels([[h, w, rh, rw]], quads, [0, len(quads)])[0]
    return page, blob, R.train_boxes(strips, rw, flip, second), second


def fetch(rec):
    return (rec.image_dev.cpu().numpy(), rec.blob_dev.cpu().numpy(), rec.gt_dev.cpu().numpy(), rec.hw, rec.page, rec.flipped, rec.im_scale)


@pytest.mark.parametrize("max_size", [80, 64])
def test_records_equal_the_host_composition_with_and_without_prefetch(folder, max_size):
    """max_size 64: prep_im_for_blob's rule gives 0.8 on every page (80 wide), so each record takes the second pass"""
    _, paths, quads = folder
    rule = dict(RULE, max_size=max_size)
    before = live()
    got = {}
    for prefetch in (False, True):
        with ctpn_amd.DataLayer(0, paths, quads, flipped=True, seed=3, prefetch=prefetch, **rule) as layer:
            assert layer.max_shape() == ((48, 80) if max_size == 80 else (38, 64))
            got[prefetch] = [fetch(layer.next()) for _ in range(10)]
            with pytest.raises(ValueError):
                ctpn_amd.DataLayer(0, paths, quads[:3])
        with pytest.raises(ValueError, match="closed"):
            layer.next()
    assert live() == before
    want_order = R.order(8, 3, 10)
    assert {r[5] for r in got[False]} == {False, True} and len({r[3] for r in got[False]}) == 2
    for k, (a, b) in enumerate(zip(got[False], got[True])):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:], k
        assert a[4] + (4 if a[5] else 0) == want_order[k][0]
        img, blob, gt, second = host_record(paths[a[4]], quads[a[4]], a[5], rule)
        assert a[3] == img.shape[:2] and a[6] == second and (second == 1.0) == (max_size == 80)
        assert a[0].tobytes() == img.tobytes() and a[1].tobytes() == blob.tobytes(), k
        assert gt.shape[0] > 0 and a[2].tobytes() == gt.tobytes(), k


def momentum():
    hyper = S.solver_defaults("Momentum")
    hyper[0] = 1e-3
    return hyper


def test_step_record_equals_step_on_the_host_composition(folder):
    _, paths, quads = folder
    arena = ctpn_amd.make_synthetic_arena(0)
    before = live()
    with ctpn_amd.Context(0, 1, 48, 80, "fp32", options={"keep_acts": 1}) as ctx, ctpn_amd.Context(0, 1, 48, 80, "fp32", options={"keep_acts": 1}) as ref_ctx:
        tr = ctpn_amd.Trainer(ctx, arena, "Momentum", momentum(), 0.0005, "conv1_1", cfg=net_cfg())
        ref = ctpn_amd.Trainer(ref_ctx, arena, "Momentum", momentum(), 0.0005, "conv1_1", cfg=net_cfg())
        shapes = set()
        with ctpn_amd.DataLayer(0, paths, quads, flipped=True, seed=3, **RULE) as layer:
            for k in range(12):
                rec = layer.next()
                got = tr.step_record(rec, seed=k)
                img, _, gt, _ = host_record(paths[rec.page], quads[rec.page], rec.flipped, RULE)
                want = ref.step(img[None], [gt], seed=k)
                assert got == want and np.isfinite(got["model_loss"]), k
                shapes.add(rec.hw)
        assert shapes == {(48, 80), (32, 80)}
        assert tr.arena().tobytes() == ref.arena().tobytes() and tr.s1.cpu().numpy().tobytes() == ref.s1.cpu().numpy().tobytes()
        assert tr.arena().tobytes() != arena.tobytes()
        del tr, ref
    assert live() == before


def test_sizes_a_b_a_on_one_ctx_equal_a_fresh_ctx_per_size(folder, tmp_path):
    """the ctx's capacity is the largest page; a forward at a smaller size leaves nothing behind that the next, larger one reads"""
    _, paths, quads = folder
    arena = ctpn_amd.make_synthetic_arena(0)
    recs = {}
    with ctpn_amd.DataLayer(0, paths, quads, flipped=False, seed=3, prefetch=False, **RULE) as layer:
        while not {0, 1, 2} <= set(recs):
            r = layer.next()
            recs.setdefault(r.page, r)
    run = [recs[0], recs[1], recs[2]]
    assert [r.hw for r in run] == [(48, 80), (32, 80), (48, 80)]
    with ctpn_amd.Context(0, 1, 48, 80, "fp32", options={"keep_acts": 1}) as ctx:
        tr = ctpn_amd.Trainer(ctx, arena, "Momentum", momentum(), 0.0005, "conv1_1", cfg=net_cfg())
        got = [tr.step_record(r, seed=k) for k, r in enumerate(run)]
        end = (tr.arena(), tr.s1.cpu().numpy())
        del tr
    snap = str(tmp_path / "snap.npz")
    want = []
    for k, r in enumerate(run):
        with ctpn_amd.Context(0, 1, r.hw[0], r.hw[1], "fp32", options={"keep_acts": 1}) as ctx:
            tr = ctpn_amd.Trainer.restore(ctx, snap) if k else ctpn_amd.Trainer(ctx, arena, "Momentum", momentum(), 0.0005, "conv1_1", cfg=net_cfg())
            want.append(tr.step_record(r, seed=k))
            tr.snapshot(snap)
            fresh = (tr.arena(), tr.s1.cpu().numpy())
            del tr
    assert got == want
    assert end[0].tobytes() == fresh[0].tobytes() and end[1].tobytes() == fresh[1].tobytes()


# ---- the command line
@pytest.fixture
def small_rule(monkeypatch, root):
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg
    monkeypatch.setattr(TextLineCfg, "SCALE", 48)
    monkeypatch.setattr(TextLineCfg, "MAX_SCALE", 80)
    monkeypatch.chdir(os.path.join(root, "text-detection-ctpn_amd"))
    saved_train, saved_prec = dict(cfg.TRAIN), cfg.TEST.PRECISION
    cfg.TRAIN.SCALES, cfg.TRAIN.MAX_SIZE = (48,), 80
    yield
    cfg.TRAIN.update(saved_train)      # cfg is one object for the whole process: leave it as it was found
    cfg.TEST.PRECISION = saved_prec


def test_train_net_with_the_data_layer(folder, small_rule, capsys):
    from ctpn_amd.ctpn import train_net as TN
    d, paths, quads = folder
    lines = []
    for _ in range(2):
        TN.main([str(d / "images"), str(d / "labels"), "--data-layer", "--steps", "6", "--synthetic", "1"])
        lines.append([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")])
    assert lines[0] == lines[1] and len(lines[0]) == 6
    recs = [json.loads(ln) for ln in lines[0]]
    want = R.order(8, 3, 6)
    for k, r in enumerate(recs):
        assert set(ctpn_amd.train.RECORD_FIELDS) | {"page", "flipped", "h", "w"} <= set(r) and r["step"] == k
        assert r["page"] + (4 if r["flipped"] else 0) == want[k][0]
        assert (r["h"], r["w"]) == ((48, 80) if r["page"] % 2 == 0 else (32, 80))
        assert all(np.isfinite(r[f]) for f in ctpn_amd.train.RECORD_FIELDS)
    # --no-flip and another seed: another order, no mirrored page
    TN.main([str(d / "images"), str(d / "labels"), "--data-layer", "--steps", "3", "--synthetic", "1", "--no-flip", "--shuffle-seed", "5", "--no-prefetch"])
    other = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [r["page"] for r in other] == [i for i, _ in R.order(4, 5, 3)] and not any(r["flipped"] for r in other)


def test_train_net_without_the_flag_still_wants_one_size(folder, small_rule):
    from ctpn_amd.ctpn import train_net as TN
    d, _, _ = folder
    with pytest.raises(SystemExit, match="one size per run"):
        TN.main([str(d / "images"), str(d / "labels"), "--steps", "1", "--synthetic", "1"])
