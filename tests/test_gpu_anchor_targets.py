"""GPU: ctpn_bbox_overlaps, ctpn_anchor_targets and ctpn_rpn_loss against tests/anchor_target_ref.py and tests/golden/anchor_targets.npz, at the
bounds tests/test_anchor_targets.py states (labels, weights, max_overlap, argmax, stats and dx / dy exact; dw / dh within 1 float32 ulp; losses
within relative 1e-10; d_heads within 1 float32 ulp of autograd's gradient; counts exact). The shapes are the smallest at which the kernels
can go wrong: every side of the LDS chunk C = 256, maps whose anchor count is no multiple of a wave or a workgroup, one anchor more than the
sampling workgroup's 1024 threads.
The smallest anchor is 16 x 12 (generate_anchors with the reference's + 1 convention), so the exact threshold hit is built on the 16 x 16 anchor:
a 16 x 32 box around it overlaps it by 256 / 512 = 0.5 exactly, and that anchor is not its column's maximum (which is foreground whatever the
thresholds)."""
import numpy as np
import pytest

import anchor_target_ref as R
import ctpn_amd
import test_anchor_targets as T

pytestmark = pytest.mark.gpu
C = 256      # TG_CHUNK of csrc/targets_dev.h


def cfg12(**kw):
    c = np.array(R.DEFAULT_CFG, np.float64)
    names = {"neg": 0, "pos": 1, "clobber": 2, "fg_fraction": 3, "batch": 4, "dc_hi": 5, "preclude": 6}
    for k, v in kw.items():
        c[names[k]] = v
    return c


def as_dict(t, i=0):
    return {k: np.asarray(getattr(t, k))[i] for k in t._fields if getattr(t, k) is not None}


def device_targets(hf, wf, im_info, gt, hard=None, dc=None, cfg=None, seed=0):
    t = ctpn_amd.anchor_targets(hf, wf, [im_info], [gt], None if hard is None else [hard], None if dc is None else [dc], cfg, seed, stages=True)
    return as_dict(t)


def random_boxes(rng, n, hi=300.0, integer=True):
    b = rng.integers(0, int(hi), (n, 4)).astype(np.float64)
    b[:, 2:] = b[:, :2] + rng.integers(0, 60, (n, 2))
    return b if integer else b * 0.7324


def test_bbox_overlaps_both_forms_bit_equal():
    rng = np.random.default_rng(0)
    special_b = np.array([[0, 0, 15, 15], [0, 0, 15, 15], [16, 0, 31, 15], [15, 0, 30, 15], [0.5, 0.25, 10.75, 3.125]], np.float64)
    special_q = np.array([[0, 0, 15, 15], [15, 15, 20, 20], [16, 16, 20, 20], [0, 0, 7, 10], [-5, -5, -1, -1]], np.float64)
    for n in (1, 63, 64, 65, 257):
        for k in (1, C - 1, C, C + 1, 2 * C + 1):
            b = np.vstack([special_b, random_boxes(rng, n // 2), random_boxes(rng, n, integer=False)])[:n]
            q = np.vstack([special_q, b[: min(n, 3)], random_boxes(rng, k // 2), random_boxes(rng, k, integer=False)])[:k] if k > 1 else b[:1]
            # (identical boxes, one-pixel touches and misses, non-integer coordinates among them)
            for fn, inter in ((ctpn_amd.bbox_overlaps, False), (ctpn_amd.bbox_intersections, True)):
                got = fn(b, q)
                assert got.shape == (n, k) and got.dtype == np.float64
                assert np.array_equal(got.view(np.int64), R.overlaps(b, q, inter).view(np.int64)), (n, k, inter)
    o = ctpn_amd.bbox_overlaps(special_b, special_q)
    assert o[0, 0] == 1.0 and o[0, 1] == 1.0 / 291.0 and o[0, 2] == 0.0 and o[0, 3] == 88.0 / 256.0
    from ctpn_amd.lib.utils import bbox as X
    assert np.array_equal(X.bbox_overlaps(special_b, special_q), o) and X.bbox_intersections(special_b, special_q)[0, 3] == 1.0
    assert ctpn_amd.bbox_overlaps(np.zeros((0, 4)), special_q).shape == (0, 5)


@pytest.mark.parametrize("name", T.SCENES)
def test_anchor_targets_on_the_fixture_scenes(golden_dir, name):
    golden = np.load(golden_dir + "/anchor_targets.npz")
    s = T.scene(golden, name)
    for batch, seed in ((0, 0), (None, 12345)):
        cfg = s["cfg12"].copy()
        if batch is not None:
            cfg[4] = batch
        got = device_targets(s["hf"], s["wf"], s["im_info"], s["gt"], s["hard"], s["dontcare"], cfg, seed)
        T.check_targets({k: v.reshape(-1) if v.ndim == 3 else v for k, v in got.items()}, T.restated(golden, name, batch, seed), name)
    # ... and against the reference's own arrays
    assert np.array_equal(got["labels_presample"].reshape(-1), s["labels_presample"].astype(np.float32))
    if "bbox_targets" in s:
        T.check_targets_against(got["bbox_targets"], s["bbox_targets"], name)


def strips(rng, G, hf, wf):
    x = rng.integers(0, max(wf - 1, 1), G) * 16
    y = rng.integers(0, max(hf * 16 - 20, 1), G)
    h = rng.integers(8, 60, G)
    return np.stack([x, y, x + 15, y + h, np.ones(G)], axis=1).astype(np.float32)


@pytest.mark.parametrize("hf,wf", [(1, 1), (5, 13), (6, 8), (12, 20), (7, 9), (11, 10)])      # 630 anchors: no multiple of 64; 1100: one past 1024
def test_synthetic_maps_and_box_counts(hf, wf):
    rng = np.random.default_rng(hf * 100 + wf)
    im = np.array([hf * 16, wf * 16, 1], np.float32)
    for G in (0, 1, 64, 65, C + 1):
        gt = strips(rng, G, hf, wf)
        hard = (rng.random(G) < 0.1).astype(np.int32)
        for cfg, seed in ((cfg12(batch=0), 0), (cfg12(batch=40), 7)):
            got = device_targets(hf, wf, im, gt, hard, None, cfg, seed)
            T.check_targets({k: v.reshape(-1) if v.ndim == 3 else v for k, v in got.items()}, R.anchor_targets(hf, wf, im, gt, hard, None, cfg, seed), (hf, wf, G))


def test_batch_of_three_equals_three_lone_calls():
    rng = np.random.default_rng(3)
    hf, wf = 6, 8
    info = np.array([[96, 128, 1], [90, 128, 1], [96, 120, 1]], np.float32)
    gts = [strips(rng, 5, hf, wf), np.zeros((0, 5), np.float32), strips(rng, C + 1, hf, wf)]
    hard = [np.array([0, 1, 0, 0, 0], np.int32), np.zeros(0, np.int32), (rng.random(C + 1) < 0.05).astype(np.int32)]
    dc = [np.zeros((0, 4), np.float32), np.array([[0, 0, 40, 40]], np.float32), np.zeros((0, 4), np.float32)]
    cfg = cfg12(batch=0)
    both = ctpn_amd.anchor_targets(hf, wf, info, gts, hard, dc, cfg, 5, stages=True)
    for i in range(3):
        lone = ctpn_amd.anchor_targets(hf, wf, info[i:i + 1], gts[i:i + 1], hard[i:i + 1], dc[i:i + 1], cfg, 5, stages=True)
        for k in both._fields:
            assert np.asarray(getattr(both, k))[i].tobytes() == np.asarray(getattr(lone, k))[0].tobytes(), (i, k)
    # with sampling the key holds the image's index in the call: image i of a batch is the restatement's image i
    cfg = cfg12(batch=30)
    both = ctpn_amd.anchor_targets(hf, wf, info, gts, hard, dc, cfg, 5, stages=True)
    for i in range(3):
        want = R.anchor_targets(hf, wf, info[i], gts[i], hard[i], dc[i], cfg, 5, image=i)
        T.check_targets({k: v.reshape(-1) if v.ndim == 3 else v for k, v in as_dict(both, i).items()}, want, i)


def test_ties_and_exact_thresholds():
    im = np.array([48, 48, 1], np.float32)
    cell = (1 * 3 + 1) * 10
    # two identical boxes: the first wins the argmax; a box equal to an anchor: IoU 1.0
    gt = np.array([[16, 16, 31, 31, 1], [16, 16, 31, 31, 1]], np.float32)
    got = device_targets(3, 3, im, gt, cfg=cfg12(batch=0))
    assert got["max_overlap"].reshape(-1)[cell + 1] == 1.0 and np.all(got["argmax"].reshape(-1)[got["argmax"].reshape(-1) >= 0] == 0)
    # a 16 x 32 box around the 16 x 16 anchor: 256 / 512 = 0.5 exactly, and the column's maximum is another anchor (16 x 34: 512 / 544)
    gt = np.array([[16, 8, 31, 39, 1]], np.float32)
    for cfg, want in ((cfg12(batch=0, pos=0.5), 1.0), (cfg12(batch=0, neg=0.5), -1.0), (cfg12(batch=0, neg=np.nextafter(0.5, 1)), 0.0), (cfg12(batch=0), -1.0),
                      (cfg12(batch=0, pos=np.nextafter(0.5, 1), neg=0.1), -1.0)):
        got = device_targets(3, 3, im, gt, cfg=cfg)
        assert got["max_overlap"].reshape(-1)[cell + 1] == 0.5 and got["max_overlap"].reshape(-1)[cell + 3] == 512.0 / 544.0
        assert got["labels"].reshape(-1)[cell + 1] == want, (cfg, want)
        assert got["labels"].reshape(-1)[cell + 3] == 1.0
        T.check_targets({k: v.reshape(-1) if v.ndim == 3 else v for k, v in got.items()}, R.anchor_targets(3, 3, im, gt, None, None, cfg, 0), "threshold")
    # an 8 x 12 box inside the 16 x 12 anchor: 96 / 192 = 0.5 exactly, here the column's maximum: foreground under every threshold
    got = device_targets(3, 3, im, np.array([[16, 18, 23, 29, 1]], np.float32), cfg=cfg12(batch=0))
    assert got["max_overlap"].reshape(-1)[cell] == 0.5 and got["labels"].reshape(-1)[cell] == 1.0


def test_zero_overlap_box_hard_box_and_dontcare_sums():
    im = np.array([48, 48, 1], np.float32)
    cfg = cfg12(batch=0)
    inside = R.anchor_targets(3, 3, im, np.zeros((0, 5), np.float32), cfg=cfg)["labels_presample"] == 0
    near, far = [16, 16, 31, 31, 1], [200, 200, 215, 230, 1]
    # a box that overlaps no inside anchor: column maximum 0, every inside anchor with overlap 0 to it -- all of them -- is foreground
    got = device_targets(3, 3, im, np.array([near, far], np.float32), cfg=cfg)
    assert np.all(got["labels"].reshape(-1)[inside] == 1.0) and got["stats"][1] == inside.sum() and got["stats"][2] == 0
    # ... and as a hard box it disables the first inside anchor, at overlap 0
    got = device_targets(3, 3, im, np.array([near, far], np.float32), np.array([0, 1], np.int32), cfg=cfg)
    first = np.nonzero(inside)[0][0]
    assert got["labels"].reshape(-1)[first] == -1.0 and got["stats"][5] == 1 and got["stats"][1] == inside.sum() - 1
    T.check_targets({k: v.reshape(-1) if v.ndim == 3 else v for k, v in got.items()},
                    R.anchor_targets(3, 3, im, np.array([near, far], np.float32), np.array([0, 1], np.int32), None, cfg, 0), "far hard")
    # dontcare: the 16 x 16 anchor of the middle cell covered by exactly 0.5 (one area; two quarters) stays, by 144 / 256 it goes
    a = (1 * 3 + 1) * 10 + 1
    for dc, want in (([[16, 16, 31, 23]], 1.0), ([[16, 16, 31, 19], [16, 20, 31, 23]], 1.0), ([[16, 16, 31, 24]], -1.0), ([[16, 16, 31, 19], [16, 20, 31, 24]], -1.0)):
        dc = np.array(dc, np.float32)
        got = device_targets(3, 3, im, np.array([near], np.float32), None, dc, cfg)
        assert got["labels"].reshape(-1)[a] == want, dc
        T.check_targets({k: v.reshape(-1) if v.ndim == 3 else v for k, v in got.items()}, R.anchor_targets(3, 3, im, np.array([near], np.float32), None, dc, cfg, 0), "dc")


def test_settings_no_fixture_scene_moves():
    """CLOBBER on the zero-overlap box (the column-maximum foreground is clobbered where the overlap is below NEGATIVE), FG_FRACTION 0 (every fg
    anchor disabled) and 0.25, DONTCARE_AREA_INTERSECTION_HI 0.75 and 0.9 on an area that covers a column of anchors by 13 / 16"""
    im = np.array([96, 128, 1], np.float32)
    three = np.array([[16, 20, 31, 50, 1], [32, 22, 47, 52, 1], [48, 24, 63, 54, 1]], np.float32)
    far4 = np.vstack([three, [[200, 200, 215, 230, 1]]]).astype(np.float32)
    dc = np.array([[0, 0, 60, 95]], np.float32)
    seen = {}
    for what, gt, dcs, cfg in (("clobber", far4, None, cfg12(clobber=1, batch=0)), ("no clobber", far4, None, cfg12(batch=0)),
                               ("clobber sampled", far4, None, cfg12(clobber=1, batch=50)),
                               ("fraction 0", three, None, cfg12(fg_fraction=0.0, batch=20)), ("fraction 0.25", far4, None, cfg12(fg_fraction=0.25, batch=40)),
                               ("dc_hi 0.75", three, dc, cfg12(dc_hi=0.75, batch=0)), ("dc_hi 0.9", three, dc, cfg12(dc_hi=0.9, batch=0))):
        got = device_targets(6, 8, im, gt, None, dcs, cfg, 9)
        T.check_targets({k: v.reshape(-1) if v.ndim == 3 else v for k, v in got.items()}, R.anchor_targets(6, 8, im, gt, None, dcs, cfg, 9), what)
        seen[what] = got
    inside = seen["no clobber"]["stats"][0]
    assert seen["no clobber"]["stats"][1] == inside and seen["no clobber"]["stats"][2] == 0
    assert list(seen["clobber"]["stats"][1:3]) == [35, 173]                     # what the reference gives (tests/golden, scene "clobber")
    assert list(seen["fraction 0"]["stats"][1:5]) == [6, 173, 0, 20]
    assert seen["fraction 0.25"]["stats"][3] == 10 and seen["fraction 0.25"]["stats"][4] == 0
    assert seen["dc_hi 0.75"]["stats"][5] > seen["dc_hi 0.9"]["stats"][5] > 0


def test_sampling(golden_dir):
    golden = np.load(golden_dir + "/anchor_targets.npz")
    s = T.scene(golden, "rows_sampled")
    pre = T.restated(golden, "rows_sampled", 0)["labels"].astype(np.float32)
    seen = []
    for seed in (0, 1, 0xDEADBEEFCAFEF00D):
        got = device_targets(s["hf"], s["wf"], s["im_info"], s["gt"], cfg=s["cfg12"], seed=seed)
        lab = got["labels"].reshape(-1)
        assert (lab == 1).sum() == 150 and (lab == 0).sum() == 150 and list(got["stats"][1:5]) == [160, 520, 150, 150]
        changed = lab != pre
        assert np.all(lab[changed] == -1) and np.all(pre[changed] >= 0)      # disabled only, and only labelled anchors
        assert lab.tobytes() == T.restated(golden, "rows_sampled", None, seed)["labels"].astype(np.float32).tobytes()
        assert np.array_equal(got["labels_presample"].reshape(-1), pre)
        seen.append(lab)
    assert not np.array_equal(seen[0], seen[1])
    c0 = s["cfg12"].copy()
    c0[4] = 0
    got = device_targets(s["hf"], s["wf"], s["im_info"], s["gt"], cfg=c0, seed=1)
    assert got["labels"].tobytes() == got["labels_presample"].tobytes() == pre.tobytes()


@pytest.mark.parametrize("name", T.SCENES)
def test_rpn_loss_on_the_references_arrays(golden_dir, name):
    golden = np.load(golden_dir + "/anchor_targets.npz")
    s = T.scene(golden, name)
    hf, wf = s["hf"], s["wf"]
    tgt = s["bbox_targets"] if "bbox_targets" in s else T.restated(golden, name, 0)["bbox_targets"]
    t = {"labels": s["labels"], "bbox_targets": tgt, "inside_weights": s["inside_weights"], "outside_weights": s["outside_weights"]}
    for ld in (60, 64):
        heads = T.seeded_heads(hf * wf, ld, 11)
        r = ctpn_amd.rpn_loss(heads.reshape(1, hf, wf, ld), s["labels"].astype(np.float32).reshape(1, hf, wf, 10), tgt.reshape(1, hf, wf, 40),
                              s["inside_weights"].reshape(1, hf, wf, 40), s["outside_weights"].reshape(1, hf, wf, 40), want_grad=True)
        T.check_loss(r.losses[0], r.counts[0], r.d_heads[0].reshape(hf * wf, ld), heads, t, name)


def edge_loss_case():
    """a 2 x 1 map: 20 anchors with the logit pairs and box deltas where the loss's arithmetic can go wrong"""
    heads = np.zeros((2, 64), np.float32)
    pairs = [(0, 0), (80, -80), (-80, 80), (1e4, -1e4), (-1e4, 1e4), (3, 3), (-1e4, -1e4), (1e4, 1e4), (0.5, -0.25), (-7, 2)]
    for a, (bg, fg) in enumerate(pairs):
        heads[0, 40 + 2 * a], heads[0, 41 + 2 * a] = bg, fg
        heads[1, 40 + 2 * a], heads[1, 41 + 2 * a] = fg, bg
    ninth = np.float32(1.0 / 9.0)                                   # rounds up: |x| >= 1/9 in double, the linear branch
    below = np.nextafter(ninth, np.float32(0))                      # the quadratic branch
    heads[0, 0:4] = [ninth, below, -ninth, -below]                  # anchors 0 and 2 are foreground: their outside weights are 1
    heads[0, 8:12] = [0.0, 1e-30, 5.0, -5.0]
    heads[1, :40] = np.linspace(-0.3, 0.3, 40, dtype=np.float32)
    heads[:, 60:] = np.nan
    labels = np.array([1, 0, 1, 0, 1, 0, 1, -1, 0, 1] + [1, 1, 0, 0, 1, -1, 0, 1, 1, 0], np.float32)
    targets = np.zeros((20, 4), np.float32)
    targets[10:] = np.float32(0.05)
    inside = np.ones((20, 4), np.float32)
    inside[10:] = [0, 1, 0, 1]
    outside = np.tile((labels == 1).astype(np.float32)[:, None], (1, 4))
    return heads, labels, targets, inside, outside


def test_rpn_loss_edge_cases():
    heads, labels, targets, inside, outside = edge_loss_case()
    t = {"labels": labels, "bbox_targets": targets, "inside_weights": inside, "outside_weights": outside}
    shp = lambda a, c: a.reshape(1, 2, 1, c)      # noqa: E731
    for ld in (64, 60):
        h = np.ascontiguousarray(heads[:, :ld])
        r = ctpn_amd.rpn_loss(shp(h, ld), shp(labels, 10), shp(targets, 40), shp(inside, 40), shp(outside, 40), want_grad=True)
        assert np.all(np.isfinite(r.losses)) and np.all(np.isfinite(r.d_heads))
        T.check_loss(r.losses[0], r.counts[0], r.d_heads[0].reshape(2, ld), h, t, ld)
        again = ctpn_amd.rpn_loss(shp(h, ld), shp(labels, 10), shp(targets, 40), shp(inside, 40), shp(outside, 40), want_grad=True)
        assert again.losses.tobytes() == r.losses.tobytes() and again.d_heads.tobytes() == r.d_heads.tobytes()
    # every label -1: cross entropy 0.0 by decision, no kept anchor, a zero gradient
    none = np.full(20, -1, np.float32)
    r = ctpn_amd.rpn_loss(shp(heads, 64), shp(none, 10), shp(targets, 40), shp(inside, 40), shp(outside, 40), want_grad=True)
    assert r.losses.tolist() == [[0.0, 0.0, 0.0]] and r.counts.tolist() == [[0, 0]] and np.all(r.d_heads == 0)
    # a batch of three equals three lone calls in bytes
    rng = np.random.default_rng(4)
    hs = np.stack([heads, np.roll(heads, 1, axis=0), T.seeded_heads(2, 64, 5)])
    ls = np.stack([labels, none, np.roll(labels, 3)])
    ts = np.stack([targets, targets, (rng.standard_normal((20, 4)) * 0.2).astype(np.float32)])
    ws = np.stack([outside, outside, np.tile((ls[2] == 1).astype(np.float32)[:, None], (1, 4))])
    ins = np.stack([inside] * 3)
    b = lambda a, c: np.ascontiguousarray(a).reshape(3, 2, 1, c)      # noqa: E731
    both = ctpn_amd.rpn_loss(b(hs, 64), b(ls, 10), b(ts, 40), b(ins, 40), b(ws, 40), want_grad=True)
    for i in range(3):
        lone = ctpn_amd.rpn_loss(shp(hs[i], 64), shp(ls[i], 10), shp(ts[i], 40), shp(ins[i], 40), shp(ws[i], 40), want_grad=True)
        assert lone.losses.tobytes() == both.losses[i].tobytes() and lone.counts.tobytes() == both.counts[i].tobytes()
        assert lone.d_heads.tobytes() == both.d_heads[i].tobytes()


def test_on_device_form_equals_the_host_form(golden_dir):
    import torch
    golden = np.load(golden_dir + "/anchor_targets.npz")
    dev = torch.device("cuda", 0)
    names = ("rows_sampled", "two_dontcare_hard", "three")
    ss = [T.scene(golden, n) for n in names[:2]]
    hf, wf = 12, 20
    info = np.stack([s["im_info"] for s in ss])
    gts = [s["gt"] for s in ss]
    hard = [np.zeros(len(ss[0]["gt"]), np.int32), ss[1]["hard"]]
    dcs = [np.zeros((0, 4), np.float32), ss[1]["dontcare"]]
    host = ctpn_amd.anchor_targets(hf, wf, info, gts, hard, dcs, None, 3, stages=True)
    offs = np.cumsum([0] + [len(g) for g in gts]).astype(np.int32)
    dco = np.cumsum([0] + [len(d) for d in dcs]).astype(np.int32)
    on = ctpn_amd.anchor_targets(hf, wf, info, torch.from_numpy(np.concatenate(gts)).to(dev), torch.from_numpy(np.concatenate(hard)).to(dev),
                                 torch.from_numpy(np.concatenate(dcs)).to(dev), None, 3, stages=True, gt_offsets=offs, dc_offsets=dco)
    for k in host._fields:
        if k != "stats":
            assert getattr(on, k).is_cuda
            assert getattr(on, k).cpu().numpy().tobytes() == getattr(host, k).tobytes(), k
    assert np.array_equal(on.stats, host.stats)
    # chained into the loss without touching the host
    heads = np.stack([T.seeded_heads(hf * wf, 64, 1), T.seeded_heads(hf * wf, 64, 2)]).reshape(2, hf, wf, 64)
    lh = ctpn_amd.rpn_loss(heads, host.labels, host.bbox_targets, host.inside_weights, host.outside_weights, want_grad=True)
    ld = ctpn_amd.rpn_loss(torch.from_numpy(heads).to(dev), on.labels, on.bbox_targets, on.inside_weights, on.outside_weights, want_grad=True)
    assert ld.d_heads.is_cuda and ld.losses.tobytes() == lh.losses.tobytes() and ld.counts.tobytes() == lh.counts.tobytes()
    assert ld.d_heads.cpu().numpy().tobytes() == lh.d_heads.tobytes()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_score_pages_equals_the_restatement_on_the_ctxs_heads(prec):
    from util import stress_arena
    imgs = ctpn_amd.weights.synthetic_images(2, 64, 96, 5)
    gts = [np.array([[16, 10, 31, 40], [32, 12, 47, 42], [48, 8, 63, 38]], np.float32), np.array([[0, 20, 15, 50, 1]], np.float32)]
    cfg = cfg12(batch=0)
    with ctpn_amd.Context(0, 2, 64, 96, prec) as ctx:
        ctx.load_weights(stress_arena("biased"))
        got = ctpn_amd.score_pages(ctx, imgs, gts, cfg=cfg)
        heads = ctx.get_tensor("heads")
    assert heads.shape == (2, 4, 6, 60) and len(got) == 2
    for i in range(2):
        g5 = np.concatenate([gts[i][:, :4], np.ones((len(gts[i]), 1), np.float32)], axis=1)
        t = R.anchor_targets(4, 6, [64, 96, 1], g5, cfg=cfg)
        ce, box, model, K, F = R.rpn_loss(heads[i].reshape(24, 60), t["labels"], t["bbox_targets"], t["inside_weights"], t["outside_weights"])
        assert (got[i]["kept"], got[i]["fg"]) == (K, F) and K > 0 and F > 0
        for key, want in (("rpn_cross_entropy", ce), ("rpn_loss_box", box), ("model_loss", model)):
            assert abs(got[i][key] - want) <= 1e-10 * abs(want), (key, got[i][key], want)
        assert [got[i]["stats"][k] for k in ctpn_amd.targets.STAT_NAMES] == t["stats"].tolist()


def test_mirror_anchor_target_layer_returns_the_references_shapes(golden_dir):
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.rpn_msr.anchor_target_layer_tf import anchor_target_layer, train_cfg12
    golden = np.load(golden_dir + "/anchor_targets.npz")
    s = T.scene(golden, "rows_sampled")
    score = np.zeros((1, 12, 20, 20), np.float32)
    saved = cfg.TRAIN
    cfg.TRAIN = type(saved)(dict(saved))      # a copy to edit; the original goes back whole
    try:
        cfg.TRAIN.RPN_BATCHSIZE, cfg.TRAIN.RPN_BBOX_INSIDE_WEIGHTS = 300, [0, 1, 0, 1]
        outs = []
        for _ in range(2):
            np.random.seed(4)
            outs.append(anchor_target_layer(score, s["gt"], None, None, s["im_info"][None]))
        assert np.array_equal(train_cfg12(), s["cfg12"])
    finally:
        cfg.TRAIN = saved
    labels, tgt, win, wout = outs[0]
    assert labels.shape == (1, 12, 20, 10) and tgt.shape == win.shape == wout.shape == (1, 12, 20, 40)
    assert all(a.dtype == np.float32 for a in outs[0]) and all(np.array_equal(a, b) for a, b in zip(*outs))
    assert (labels == 1).sum() == 150 and (labels == 0).sum() == 150
    assert np.array_equal(labels.reshape(-1) != -1, (s["labels_presample"] != -1) & (labels.reshape(-1) != -1))
    T.check_targets_against(tgt, s["bbox_targets"], "mirror")


def test_score_pages_command_line(tmp_path, monkeypatch, capsys, root):
    """ctpn/score_pages.py on one PNG file and its label file, in process: the JSON line is score_pages' result for the resized image and
    the scaled boxes"""
    import json
    import os
    from PIL import Image
    from ctpn_amd.ctpn import demo as D
    from ctpn_amd.ctpn import score_pages as S
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg
    from ctpn_amd.lib.utils import image as imutil
    rng = np.random.default_rng(8)
    img = rng.integers(0, 255, (60, 90, 3), dtype=np.uint8)
    (tmp_path / "images").mkdir()
    (tmp_path / "labels").mkdir()
    Image.fromarray(img[:, :, ::-1]).save(str(tmp_path / "images" / "page_1.png"))
    (tmp_path / "labels" / "page_1.txt").write_text("text\t16\t20\t31\t50\ntext\t32\t22\t47\t52\n")
    monkeypatch.chdir(os.path.join(root, "text-detection-ctpn_amd"))
    S.main([str(tmp_path / "images"), str(tmp_path / "labels"), "--synthetic", "0", "--precision", "bf16"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    got = json.loads(lines[0])
    big, f = D.resize_im(imutil.imread(str(tmp_path / "images" / "page_1.png")), scale=TextLineCfg.SCALE, max_scale=TextLineCfg.MAX_SCALE)
    assert got["image"] == "page_1.png" and got["scale"] == f and got["stats"]["fg_presample"] == got["stats"]["fg"] == got["fg"] > 0
    cfg = cfg12(batch=0)
    with ctpn_amd.Context(0, 1, big.shape[0], big.shape[1], "bf16") as ctx:
        ctx.load_weights(ctpn_amd.make_synthetic_arena(0))
        want = ctpn_amd.score_pages(ctx, big[None], [S.scale_boxes([[16, 20, 31, 50], [32, 22, 47, 52]], f)], cfg=cfg)[0]
    for k in ("rpn_cross_entropy", "rpn_loss_box", "model_loss", "kept", "fg", "stats"):
        assert got[k] == want[k], k
