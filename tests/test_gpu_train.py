"""GPU: the training step that stays on the device (include/ctpn_hip_train.h: ctpn_get_tensor_device; include/ctpn_hip.h, "the solver step"; ctpn_amd.solver,
ctpn_amd.train, ctpn/train_net.py), against tests/solver_ref.py, which tests/test_solver.py holds on the CPU.

  * get_tensor_device equals get_tensor in bytes: every name, four precisions, two shapes, a ragged forward, the refusals and the probe;
    between a submit and its collect it reads the batch in flight and changes neither batch;
  * solver_step, three solvers x three consecutive steps, counts at every seam of the plan, base pointers at every 4-byte alignment:
    exact dyadic data equals the restatement bit for bit (out2 too: every sum is exact, whatever its order); on random data out2[0] lies
    within count 2^-53 out2[0] of the restatement's sum (the a priori bound of a double sum of non-negative terms in any order) and the
    vectors equal the restatement evaluated with the device's own out2[0], bit for bit;
  * network_gradients_device equals network_gradients in bytes; a Momentum Trainer equals finetune.run_steps in bytes; Adam and RMS
    Trainers step by step against network_gradients + the restatement; snapshot / restore; train_net.py in process."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import conv_grad_cases as K
import ctpn_amd
import solver_ref as R
from ctpn_amd import _binding as B
from ctpn_amd import solver as S
from util import stress_arena

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SOLVER_NAMES = ["Momentum", "Adam", "RMS"]
BLOCK = 1024      # block_floats of every count up to 2048 x 1024


def live():
    out = (C.c_longlong * 4)()
    B.load_library().ctpn_debug_live_resources(out)
    return list(out)


# ---- get_tensor_device
NAMES = ["conv1_1", "conv1_2", "pool1", "conv2_1", "conv2_2", "pool2", "conv3_1", "conv3_2", "conv3_3", "pool3", "conv4_1", "conv4_2", "conv4_3", "pool4",
         "conv5_1", "conv5_2", "conv5_3", "rpn_conv/3x3", "lstm_pre", "lstm_out", "lstm_o", "heads", "rpn_cls_prob_reshape", "rpn_bbox_pred"]


@pytest.mark.parametrize("prec", ["fp32", "split", "bf16", "fp16"])
@pytest.mark.parametrize("nhw", [(1, 48, 80), (2, 32, 48)])
def test_get_tensor_device_equals_get_tensor_in_bytes(prec, nhw):
    n, h, w = nhw
    img = ctpn_amd.weights.synthetic_images(n, h, w, 5)
    before = live()
    with ctpn_amd.Context(0, n, h, w, prec, options={"keep_acts": 1}) as ctx:
        ctx.load_weights(stress_arena("biased"))
        ctx.forward(img)
        ctx.proposals(np.array([[h, w, 1.0]] * n, np.float32))
        for name in NAMES:
            want = ctx.get_tensor(name)
            got = ctx.get_tensor_device(name)
            assert got.device == torch.device(DEV) and tuple(got.shape) == want.shape, name
            assert got.cpu().numpy().tobytes() == want.tobytes(), (prec, name)
        # an output at a 4-byte alignment takes the kernel's other store form
        want = ctx.get_tensor("conv5_3")
        buf = torch.zeros(want.size + 3, dtype=torch.float32, device=DEV)
        shape = (C.c_int * 4)()
        B._check(ctx._lib.ctpn_get_tensor_device(ctx._h, b"conv5_3", C.c_void_p(buf.data_ptr() + 4), want.size, shape))
        back = buf.cpu().numpy()
        assert back[1: 1 + want.size].tobytes() == want.tobytes() and back[0] == 0 and back[-2:].tolist() == [0, 0]
    assert live() == before


def test_get_tensor_device_after_a_ragged_forward():
    hc, w, heights = 48, 64, [48, 32]
    canvas = ctpn_amd.weights.synthetic_images(2, hc, w, 9)
    canvas[1, 32:] = 0
    with ctpn_amd.Context(0, 2, hc, w, "bf16", options={"keep_acts": 1}) as ctx:
        ctx.load_weights(stress_arena("biased"))
        ctx.forward_ragged(canvas, heights)
        for name in NAMES[:-2]:
            want = ctx.get_tensor(name)
            assert ctx.get_tensor_device(name).cpu().numpy().tobytes() == want.tobytes(), name


def test_get_tensor_device_refusals_and_the_capacity_probe():
    img = ctpn_amd.weights.synthetic_images(1, 48, 80, 5)
    lib = B.load_library()
    buf = torch.full((64,), 7.0, dtype=torch.float32, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    with ctpn_amd.Context(0, 1, 48, 80, "bf16") as ctx:      # keep_acts = 0
        shape = (C.c_int * 4)()
        assert lib.ctpn_get_tensor_device(ctx._h, b"heads", p, 64, shape) == -3      # no forward yet
        ctx.load_weights(stress_arena("biased"))
        ctx.forward(img)
        for name in ("conv1_1", "conv1_2", "lstm_o", "rpn_cls_prob_reshape", "rpn_bbox_pred"):
            hrc = lib.ctpn_get_tensor(ctx._h, name.encode(), np.zeros(64, np.float32).ctypes.data_as(C.POINTER(C.c_float)), 64, shape)
            assert lib.ctpn_get_tensor_device(ctx._h, name.encode(), p, 64, shape) == hrc == -3, name
            with pytest.raises(ctpn_amd.CtpnError):
                ctx.get_tensor_device(name)
        assert lib.ctpn_get_tensor_device(ctx._h, b"no_such", p, 64, shape) == -1
        assert lib.ctpn_get_tensor_device(ctx._h, b"heads", None, 64, shape) == -1
        assert lib.ctpn_get_tensor_device(ctx._h, b"heads", p, 0, shape) == -4 and list(shape) == [1, 3, 5, 60]      # the probe
        assert (buf == 7.0).all()
        assert ctx.get_tensor_device("conv5_3").cpu().numpy().tobytes() == ctx.get_tensor("conv5_3").tobytes()


def test_get_tensor_device_between_a_submit_and_its_collect():
    """One batch in flight, then two: the most recent forward is the last submit's, get_tensor_device gives its tensors -- the bytes of a
    fresh ctx's forward of that image -- and every collect gives the lines and rois of a synchronous detect."""
    h, w = 48, 80
    imgs = ctpn_amd.weights.synthetic_images(2, h, w, 21)
    a, b = imgs[:1], imgs[1:]
    fresh = {}
    with ctpn_amd.Context(0, 1, h, w, "bf16") as ctx:
        ctx.load_weights(stress_arena("biased"))
        for key, im in (("a", a), ("b", b)):
            lines, rois = ctx.detect(im, want_rois=True)
            ctx.forward(im)
            fresh[key] = (lines, rois, ctx.get_tensor("heads"), ctx.get_tensor("rpn_conv/3x3"))

    def same(got, key):
        lines, rois = got
        return all(np.array_equal(p, q) for p, q in zip(lines, fresh[key][0])) and all(np.array_equal(p, q) for p, q in zip(rois, fresh[key][1])) and \
            len(lines) == len(fresh[key][0])

    def read(ctx, key):
        return all(ctx.get_tensor_device(name).cpu().numpy().tobytes() == fresh[key][k].tobytes() for k, name in ((2, "heads"), (3, "rpn_conv/3x3")))
    before = live()
    with ctpn_amd.Context(0, 1, h, w, "bf16") as ctx:
        ctx.load_weights(stress_arena("biased"))
        ctx.detect_submit(a, slot=0)
        assert read(ctx, "a") and read(ctx, "a")
        assert same(ctx.detect_collect(0, want_rois=True), "a")
        ctx.detect_submit(a, slot=0)
        ctx.detect_submit(b, slot=1)
        assert read(ctx, "b")
        assert same(ctx.detect_collect(0, want_rois=True), "a") and same(ctx.detect_collect(1, want_rois=True), "b")
        assert read(ctx, "b")
    assert live() == before


# ---- solver_step
def dyadic(count, seed):
    """multiples of 2^-6 of magnitude <= 1: with decay 0 or 2^-11 the first step's ge is exact and both of its sums are exact in double
    whatever their order (ge^2 is a multiple of 2^-34 below 2, over at most 2053 elements); later steps round, identically on both sides"""
    rng = np.random.default_rng(seed)
    return [(rng.integers(-64, 65, count) / 64.0).astype(np.float32) for _ in range(2)]


def segments(count, decay):
    if count < 3:
        return np.array([count], np.int64), np.array([decay], np.float32)
    cuts = sorted(set([count // 3, count // 3 + 1, (2 * count) // 3, count]))      # a boundary inside a quad, a one-element segment
    return np.array(cuts, np.int64), np.array([decay if i % 2 == 0 else 0.0 for i in range(len(cuts))], np.float32)


def dev_vec(a, offset):
    """a copy of `a` on the device whose first float lies `offset` floats past a 16-byte boundary"""
    buf = torch.zeros(a.shape[0] + 4, dtype=torch.float32, device=DEV)
    v = buf[offset: offset + a.shape[0]]
    v.copy_(torch.from_numpy(a))
    return v


def run_three(solver, count, w, g, decay, hyper, offset, on_device=True):
    """three steps on the device next to three of the restatement fed the device's own out2[0]; every vector compared after every step"""
    code = S.SOLVERS[solver]
    seg_end, seg_decay = segments(count, decay)
    s1, s2 = np.full(count, hyper[5], np.float32), np.full(count, hyper[6], np.float32)
    rw, r1, r2 = w.copy(), s1.copy(), s2.copy()
    if on_device:
        dw, dg, d1, d2 = (dev_vec(a, offset) for a in (w, g, s1, s2))
    else:
        dw, dg, d1, d2 = w.copy(), g.copy(), s1.copy(), s2.copy()
    outs = []
    for t in (1, 2, 3):
        out2 = ctpn_amd.solver_step(solver, dw, dg, d1, None if code == 0 else d2, hyper, t, seg_end, seg_decay)
        rw, r1, rr2, ref2 = R.step(code, rw, g, r1, None if code == 0 else r2, seg_end, seg_decay, hyper, t, sumsq=out2[0])
        r2 = r2 if rr2 is None else rr2
        back = [v.cpu().numpy() if on_device else v for v in (dw, d1, d2)]
        assert back[0].tobytes() == rw.tobytes() and back[1].tobytes() == r1.tobytes() and back[2].tobytes() == r2.tobytes(), (solver, count, t, offset)
        outs.append((out2, ref2))
    return outs, (rw, r1, r2)


COUNTS = [1, 3, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 5]


@pytest.mark.parametrize("solver", SOLVER_NAMES)
def test_solver_step_on_exact_dyadic_data(solver):
    assert all(S.solver_plan(c)[0] == BLOCK for c in COUNTS)
    hyper = S.solver_defaults(solver)
    hyper[0] = 2.0 ** -7
    hyper[1] = 0.5
    if solver == "RMS":
        hyper[2] = 0.25
    for count in COUNTS:
        for offset in range(4):
            for decay, clip in ((0.0, 1e30), (2.0 ** -11, 2.0 ** -3)):
                w, g = dyadic(count, 100 * count + offset)
                hyper[4] = clip
                outs, _ = run_three(solver, count, w, g, decay, hyper, offset)
                if count >= BLOCK - 1:
                    assert (np.sqrt(outs[0][0][0]) > clip) == (clip < 1)      # the clip active and inactive
                for out2, ref2 in outs:
                    assert out2[0] == ref2[0] and out2[1] == ref2[1], (solver, count, offset, out2, ref2)
                    assert decay > 0 or out2[1] == 0


@pytest.mark.parametrize("solver", SOLVER_NAMES)
def test_solver_step_on_random_data_and_the_real_decay_table(solver):
    rng = np.random.default_rng(3)
    hyper = S.solver_defaults(solver)
    for count, offset in ((2 * BLOCK + 5, 1), (ctpn_amd.WEIGHT_FLOATS, 0)):
        w = (rng.standard_normal(count) * 0.05).astype(np.float32)
        g = (rng.standard_normal(count) * (0.01 if count > 5000 else 1.0)).astype(np.float32)      # 17.9 M floats: norm 42 > 10, the clip is active
        if count == ctpn_amd.WEIGHT_FLOATS:
            seg_end, seg_decay = S.decay_table("conv1_1", 0.0005)
            code = S.SOLVERS[solver]
            dw, dg = dev_vec(w, offset), dev_vec(g, offset)
            d1, d2 = dev_vec(np.full(count, hyper[5], np.float32), offset), dev_vec(np.zeros(count, np.float32), offset)
            r1, r2, rw = np.full(count, hyper[5], np.float32), np.zeros(count, np.float32), w
            for t in (1, 2, 3):
                out2 = ctpn_amd.solver_step(solver, dw, dg, d1, None if code == 0 else d2, hyper, t, seg_end, seg_decay)
                rw, r1, rr2, ref2 = R.step(code, rw, g, r1, None if code == 0 else r2, seg_end, seg_decay, hyper, t, sumsq=out2[0])
                r2 = r2 if rr2 is None else rr2
                assert abs(out2[0] - ref2[0]) <= count * 2.0 ** -53 * out2[0] and abs(out2[1] - ref2[1]) <= count * 2.0 ** -53 * out2[1]
                assert np.sqrt(out2[0]) > hyper[4] and out2[1] > 0
                for got, want in ((dw, rw), (d1, r1), (d2, r2)):
                    assert got.cpu().numpy().tobytes() == want.tobytes(), (solver, t, offset)
                if t == 1:
                    first = (out2, dw.clone(), d1.clone(), d2.clone())
            # the same bytes on a second call
            ew, e1, e2 = dev_vec(w, 0), dev_vec(np.full(count, hyper[5], np.float32), 0), dev_vec(np.zeros(count, np.float32), 0)
            again = ctpn_amd.solver_step(solver, ew, dg, e1, None if code == 0 else e2, hyper, 1, seg_end, seg_decay)
            assert again == first[0] and torch.equal(ew, first[1]) and torch.equal(e1, first[2]) and torch.equal(e2, first[3])
        else:
            outs, _ = run_three(solver, count, w, g, 0.0005, hyper, offset)
            for out2, ref2 in outs:
                assert abs(out2[0] - ref2[0]) <= count * 2.0 ** -53 * out2[0]
            host, _ = run_three(solver, count, w, g, 0.0005, hyper, 0, on_device=False)      # host arrays: the same call, the same bytes
            assert [o[0] for o in host] == [o[0] for o in outs]


def test_solver_step_refuses_a_nan_gradient_and_bad_arguments():
    count = 2 * BLOCK + 5
    w, g = dyadic(count, 1)
    g[BLOCK + 3] = np.nan
    before = live()
    for solver in SOLVER_NAMES:
        hyper = S.solver_defaults(solver)
        dw, dg, d1, d2 = (dev_vec(a, 2) for a in (w, g, np.ones(count, np.float32), np.ones(count, np.float32)))
        with pytest.raises(ctpn_amd.CtpnError, match="not finite"):
            ctpn_amd.solver_step(solver, dw, dg, d1, d2, hyper, 1)
        assert dw.cpu().numpy().tobytes() == w.tobytes() and (d1 == 1).all() and (d2 == 1).all()
        hw, h1, h2 = w.copy(), np.ones(count, np.float32), np.ones(count, np.float32)
        with pytest.raises(ctpn_amd.CtpnError, match="not finite"):
            ctpn_amd.solver_step(solver, hw, g, h1, h2, hyper, 1)
        assert hw.tobytes() == w.tobytes() and (h1 == 1).all() and (h2 == 1).all()
    g[BLOCK + 3] = 0
    hyper = S.solver_defaults("Adam")
    ones = np.ones(count, np.float32)
    with pytest.raises(ctpn_amd.CtpnError):
        ctpn_amd.solver_step("Adam", w.copy(), g, ones.copy(), ones.copy(), hyper, 0)                                  # t is 1-based
    with pytest.raises(ctpn_amd.CtpnError):
        ctpn_amd.solver_step("Adam", w.copy(), g, ones.copy(), ones.copy(), hyper, 1, [count - 1], [0.0])              # segments end at count
    with pytest.raises(ctpn_amd.CtpnError):
        ctpn_amd.solver_step("Adam", w.copy(), g, ones.copy(), ones.copy(), hyper, 1, [5, 5, count], [0.0, 0.0, 0.0])  # ascending
    with pytest.raises(ValueError):
        ctpn_amd.solver_step("Adam", w.copy(), g, ones.copy(), None, hyper, 1)
    assert live() == before


# ---- the resident gradient and the Trainer
H, W = K.FT_H, K.FT_W


def trained_names(from_layer):
    first = S.trained_offset(from_layer)
    return [name for name, _, off in ctpn_amd.MANIFEST if off >= first]


def flat(grads, from_layer):
    return np.concatenate([grads[name].reshape(-1) for name in trained_names(from_layer)])


def test_network_gradients_device_equals_network_gradients_in_bytes():
    arena = stress_arena("biased")
    img, gts = K.net_page(48, 80)
    before = live()
    with ctpn_amd.Context(0, 1, 48, 80, "fp32", options={"keep_acts": 1}) as ctx:
        ctx.load_weights(arena)
        arena_dev = torch.from_numpy(arena).to(DEV)
        for from_layer in ("conv1_1", "rpn_conv/3x3"):
            losses, grads = ctpn_amd.network_gradients(ctx, img, gts, cfg=K.net_cfg(), from_layer=from_layer)
            dl, dg = ctpn_amd.network_gradients_device(ctx, img, gts, cfg=K.net_cfg(), arena_dev=arena_dev, from_layer=from_layer)
            assert dg.device == torch.device(DEV) and dl == losses
            assert dg.cpu().numpy().tobytes() == flat(grads, from_layer).tobytes(), from_layer
    with ctpn_amd.Context(0, 1, 48, 80, "fp32") as ctx:
        ctx.load_weights(arena)
        with pytest.raises(ValueError, match="keep_acts"):
            ctpn_amd.network_gradients_device(ctx, img, gts, cfg=K.net_cfg(), arena_dev=arena_dev)
    del arena_dev, dg
    assert live() == before


def test_momentum_trainer_equals_finetune_run_steps_in_bytes(monkeypatch):
    """decay 0 and a clip norm of 1e30 on both sides: the host loop's norm comes from numpy's pairwise sum, the device's from the plan's
    order, and with the clip out of reach neither enters the update"""
    from ctpn_amd.ctpn import finetune as FT
    monkeypatch.setattr(FT, "CLIP_NORM", 1e30)
    arena = ctpn_amd.make_synthetic_arena(0)
    img, gts = K.net_page(H, W)
    pages = [(img[0], gts[0])]
    with ctpn_amd.Context(0, 1, H, W, "fp32", options={"keep_acts": 1}) as ctx:
        want, recs = FT.run_steps(lambda h, w: ctx, arena, pages, K.FT_STEPS, K.FT_LR, K.FT_MOMENTUM, cfg=K.net_cfg())
        hyper = S.solver_defaults("Momentum")
        hyper[0], hyper[1], hyper[4] = K.FT_LR, K.FT_MOMENTUM, 1e30
        tr = ctpn_amd.Trainer(ctx, arena, "Momentum", hyper, 0.0, "conv1_1", cfg=K.net_cfg())
        mine = [tr.step(img, gts, seed=k) for k in range(K.FT_STEPS)]
        got = tr.arena()
    assert [r["model_loss"] for r in mine] == [r["model_loss"] for r in recs]
    assert all(r["reg_loss"] == 0 and r["total_loss"] == r["model_loss"] for r in mine)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("solver", ["Adam", "RMS"])
def test_adam_and_rms_trainers_step_by_step_against_the_restatement(solver, tmp_path):
    arena = ctpn_amd.make_synthetic_arena(0)
    img, gts = K.net_page(H, W)
    from_layer = "conv5_3"
    first = S.trained_offset(from_layer)
    seg_end, seg_decay = S.decay_table(from_layer, 0.0005)
    hyper = S.solver_defaults(solver)
    hyper[0] = 1e-4
    code = S.SOLVERS[solver]
    before = live()
    with ctpn_amd.Context(0, 1, H, W, "fp32", options={"keep_acts": 1}) as ctx:
        tr = ctpn_amd.Trainer(ctx, arena, solver, hyper, 0.0005, from_layer, cfg=K.net_cfg())
        w = arena[first:].copy()
        s1, s2 = np.full(w.shape[0], hyper[5], np.float32), np.zeros(w.shape[0], np.float32)
        with ctpn_amd.Context(0, 1, H, W, "fp32", options={"keep_acts": 1}) as ref_ctx:
            for k in range(2):
                full = np.concatenate([arena[:first], w])
                ref_ctx.load_weights(full)
                losses, grads = ctpn_amd.network_gradients(ref_ctx, img, gts, cfg=K.net_cfg(), seed=k, from_layer=from_layer)
                rec = tr.step(img, gts, seed=k)
                assert set(ctpn_amd.train.RECORD_FIELDS) <= set(rec) and rec["step"] == k and rec["lr"] == hyper[0]
                g = flat(grads, from_layer)
                w, s1, s2, ref2 = R.step(code, w, g, s1, s2, seg_end, seg_decay, hyper, k + 1, sumsq=rec["sumsq"])
                assert abs(rec["sumsq"] - ref2[0]) <= w.shape[0] * 2.0 ** -53 * rec["sumsq"]
                assert abs(rec["reg_loss"] - ref2[1]) <= w.shape[0] * 2.0 ** -53 * rec["reg_loss"] and rec["reg_loss"] > 0
                assert rec["model_loss"] == losses[0]["model_loss"] and rec["total_loss"] == rec["model_loss"] + rec["reg_loss"]
                assert rec["grad_norm"] == float(np.sqrt(rec["sumsq"]))
                assert tr.arena()[first:].tobytes() == w.tobytes() and tr.arena()[:first].tobytes() == arena[:first].tobytes()
                assert tr.s1.cpu().numpy().tobytes() == s1.tobytes() and tr.s2.cpu().numpy().tobytes() == s2.tobytes()
        # snapshot after 2 steps, then 2 more, equals restore, then 2 more
        snap = str(tmp_path / "snap.npz")
        tr.snapshot(snap)
        a = [tr.step(img, gts, seed=k) for k in (2, 3)]
        end = (tr.arena(), tr.s1.cpu().numpy(), tr.s2.cpu().numpy())
        del tr
        tr2 = ctpn_amd.Trainer.restore(ctx, snap)
        assert tr2.iter == 2 and tr2.solver == solver and tr2.from_layer == from_layer
        b = [tr2.step(img, gts, seed=k) for k in (2, 3)]
        assert a == b
        assert tr2.arena().tobytes() == end[0].tobytes() and tr2.s1.cpu().numpy().tobytes() == end[1].tobytes() and tr2.s2.cpu().numpy().tobytes() == end[2].tobytes()
        del tr2
    assert live() == before


def test_the_schedule_moves_momentums_rate_alone():
    arena = ctpn_amd.make_synthetic_arena(0)
    img, gts = K.net_page(H, W)
    with ctpn_amd.Context(0, 1, H, W, "fp32", options={"keep_acts": 1}) as ctx:
        for solver, want in (("Momentum", [1e-3, 1e-3, float(np.float32(np.float64(np.float32(1e-3)) * 0.1))]), ("Adam", [1e-3] * 3)):
            tr = ctpn_amd.Trainer(ctx, arena, solver, None, 0.0005, "rpn_conv/3x3", stepsize=2, gamma=0.1, cfg=K.net_cfg())
            got = [tr.step(img, gts, seed=k)["lr"] for k in range(3)]
            assert got == [float(np.float32(v)) if solver == "Momentum" else v for v in want], (solver, got)


# ---- the command line
@pytest.fixture
def page_dir(tmp_path, monkeypatch, root):
    from PIL import Image
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg
    img, gts = K.net_page(H, W)
    (tmp_path / "images").mkdir()
    (tmp_path / "labels").mkdir()
    Image.fromarray(img[0][:, :, ::-1]).save(str(tmp_path / "images" / "page_1.png"))
    (tmp_path / "labels" / "page_1.txt").write_text("".join("text\t%d\t%d\t%d\t%d\n" % tuple(b) for b in gts[0]))
    monkeypatch.setattr(TextLineCfg, "SCALE", H)
    monkeypatch.setattr(TextLineCfg, "MAX_SCALE", W)
    monkeypatch.chdir(os.path.join(root, "text-detection-ctpn_amd"))
    saved_train, saved_prec = dict(cfg.TRAIN), cfg.TEST.PRECISION
    yield tmp_path
    cfg.TRAIN.update(saved_train)      # cfg is one object for the whole process: leave it as it was found
    cfg.TEST.PRECISION = saved_prec


def test_train_net_momentum_lowers_the_loss(page_dir, capsys):
    from ctpn_amd.ctpn import train_net as TN
    out = str(page_dir / "run")
    TN.main([str(page_dir / "images"), str(page_dir / "labels"), "--synthetic", "0", "--steps", str(K.FT_STEPS), "--solver", "Momentum", "--lr", str(K.FT_LR),
             "--momentum", str(K.FT_MOMENTUM), "--out", out, "--snapshot-iters", "0"])
    recs = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    losses = [r["model_loss"] for r in recs]
    print(losses)
    assert len(recs) == K.FT_STEPS and all(np.isfinite(v) for v in losses) and all(r["grad_norm"] > 0 and r["reg_loss"] > 0 for r in recs)
    assert losses[-1] < losses[0], losses
    back, old = np.load(out + ".npy"), ctpn_amd.make_synthetic_arena(0)
    assert back.shape == old.shape and not np.array_equal(back, old)


def test_train_net_adam_from_the_reference_settings(page_dir, capsys, root):
    from ctpn_amd.ctpn import train_net as TN
    out = str(page_dir / "run")
    TN.main([str(page_dir / "images"), str(page_dir / "labels"), "--synthetic", "0", "--steps", "2", "--cfg",
             os.path.join(root, "tests", "golden", "train", "text_train.yml"), "--from", "conv5_1", "--out", out, "--snapshot-iters", "2"])
    recs = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(recs) == 2
    for k, r in enumerate(recs):
        assert set(ctpn_amd.train.RECORD_FIELDS) | {"page"} <= set(r) and r["step"] == k and r["lr"] == 1e-5
        assert all(np.isfinite(r[f]) for f in ctpn_amd.train.RECORD_FIELDS) and r["total_loss"] == r["model_loss"] + r["reg_loss"]
    with np.load(out + "_iter_2.npz") as z:
        assert str(z["solver"]) == "Adam" and float(z["weight_decay"]) == 0.0005 and int(z["iter"]) == 2 and float(z["hyper"][0]) == 1e-5
        assert z["arena"].shape == (ctpn_amd.WEIGHT_FLOATS,) and z["s1"].shape == z["s2"].shape == (ctpn_amd.WEIGHT_FLOATS - S.trained_offset("conv5_1"),)
        assert np.array_equal(z["arena"], np.load(out + ".npy")) and np.any(z["s2"] != 0)
