"""GPU: ctpn_tail_forward / ctpn_tail_backward (include/ctpn_hip.h, "the recurrent tail: forward with saved activations, backward") through the
C ABI, against tests/tail_grad_ref.py, which tests/test_tail_grad.py holds against oracle.network and central differences on the CPU.

Shapes: rows n hf in {1, 15, 16, 17, 33} -- either side of the 16 rows a workgroup of the forward and of the backward recurrence owns; T = wf in
{1, 2, 3, 20}; cell counts 1 .. 660 around the reductions' seams: no multiple of the 4 cells one MFMA consumes, one block of 256 exactly, one short
block, two and three blocks with a short last one.

  * exact data: small integers and dyadic gate values, so that every product and sum is exact in fp32 whatever the order (the test checks that
    condition on the float64 reference: sum |a b| below 2^24 units). The recurrence is neutralised through the saved block itself, which is an
    INPUT of the backward: Wh = 0, f = 0 (no cell-state carry), c = 0, i = j = o = 1/2, so d_pre = d_lstm_out x {1/16, 3/16, 0, 0}. The four weight
    products, the bias sums and the three data-gradient GEMMs then equal float64 bit for bit.
  * stage by stage on random data: the error of every tensor against float64 autograd, max |got - ref64| / max |ref64|, is allowed four times the
    error e32 of the restatement's own float32 autograd on the same case; where e32 is 0 the device is 0. Measured on an MI355X
    (profiles/tail_backward_accuracy.json; tools/tail_backward_throughput.py --accuracy writes it from these same cases): worst ratio over
    d_pre, d_x and the ten gradient tensors 3.85 (d_x at 33 rows x 1 step), worst weight tensor 3.74 (the fw bias at 16 x 3).
  * structure, forward identity with a CTPN_PREC_FP32 ctx, arguments, the fine-tune loop."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ctpn_amd
import tail_grad_cases as K
import tail_grad_ref as TR
from ctpn_amd import _binding as B
from ctpn_amd import tail_grad as TG

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 15, 2), (1, 16, 3), (1, 17, 20), (3, 11, 20), (1, 16, 16), (1, 33, 1)]      # (n, hf, wf)
KERNEL = "lstm_o/bidirectional_rnn/%s/lstm_cell/kernel"
BIAS = "lstm_o/bidirectional_rnn/%s/lstm_cell/bias"


def live():
    out = (C.c_longlong * 4)()
    B.load_library().ctpn_debug_live_resources(out)
    return list(out)


# ---- exact data
def exact_case(n, hf, wf, seed):
    """integer inputs and the float64 gradients they give; every sum's |terms| stay below 2^24 units of 1/16"""
    rng = np.random.default_rng([seed, n, hf, wf])
    M = n * hf * wf

    def sparse(shape, hi, density):
        return (rng.integers(-hi, hi + 1, shape) * (rng.random(shape) < density)).astype(np.float64)

    w = {}
    for d in ("fw", "bw"):
        k = np.zeros((640, 512))
        k[:512] = sparse((512, 512), 2, 0.2)      # Wh = kernel[512:] stays 0
        w[KERNEL % d], w[BIAS % d] = k, sparse((512,), 3, 1.0)
    w["lstm_o/weights"], w["lstm_o/biases"] = sparse((256, 512), 1, 0.1), sparse((512,), 3, 1.0)
    w["rpn_bbox_pred/weights"], w["rpn_bbox_pred/biases"] = sparse((512, 40), 2, 0.3), sparse((40,), 3, 1.0)
    w["rpn_cls_score/weights"], w["rpn_cls_score/biases"] = sparse((512, 20), 2, 0.3), sparse((20,), 3, 1.0)
    x = sparse((M, 512), 3, 0.5)
    lstm_out, lstm_o = sparse((M, 256), 3, 0.5), sparse((M, 512), 3, 0.5)
    gates = np.zeros((M, 2, 5, 128))
    gates[:, :, [0, 1, 3], :] = 0.5
    dh = np.zeros((M, 64))
    dh[:, :60] = sparse((M, 60), 2, 0.3)
    # float64
    wheads = np.concatenate([w["rpn_bbox_pred/weights"], w["rpn_cls_score/weights"]], axis=1)       # (512, 60)
    d_lstm_o = dh[:, :60] @ wheads.T
    d_lstm_out = d_lstm_o @ w["lstm_o/weights"].T
    d_pre = np.zeros((M, 1024))
    for d in range(2):
        dl = d_lstm_out[:, d * 128:(d + 1) * 128]
        d_pre[:, d * 512: d * 512 + 128] = dl / 16.0
        d_pre[:, d * 512 + 128: d * 512 + 256] = dl * 3.0 / 16.0
    wx = np.concatenate([w[KERNEL % "fw"][:512], w[KERNEL % "bw"][:512]], axis=1)                   # (512, 1024)
    want = {"d_x": d_pre @ wx.T}
    bound = [np.abs(d_pre) @ np.abs(wx.T), np.abs(dh[:, :60]) @ np.abs(wheads.T), np.abs(d_lstm_o) @ np.abs(w["lstm_o/weights"].T)]
    g = {}
    lo3 = lstm_out.reshape(n * hf, wf, 256)
    for d, name in enumerate(("fw", "bw")):
        dp = d_pre[:, d * 512:(d + 1) * 512]
        prev = np.zeros_like(lo3[:, :, :128])
        if d == 0:
            prev[:, 1:] = lo3[:, :-1, :128]
        else:
            prev[:, :-1] = lo3[:, 1:, 128:]
        prev = prev.reshape(M, 128)
        g[KERNEL % name] = np.concatenate([x.T @ dp, prev.T @ dp], axis=0)
        g[BIAS % name] = dp.sum(axis=0)
        bound += [np.abs(x.T) @ np.abs(dp), np.abs(prev.T) @ np.abs(dp), np.abs(dp).sum(axis=0)]
    g["lstm_o/weights"], g["lstm_o/biases"] = lstm_out.T @ d_lstm_o, d_lstm_o.sum(axis=0)
    g["rpn_bbox_pred/weights"], g["rpn_bbox_pred/biases"] = lstm_o.T @ dh[:, :40], dh[:, :40].sum(axis=0)
    g["rpn_cls_score/weights"], g["rpn_cls_score/biases"] = lstm_o.T @ dh[:, 40:60], dh[:, 40:60].sum(axis=0)
    bound += [np.abs(lstm_out.T) @ np.abs(d_lstm_o), np.abs(lstm_o.T) @ np.abs(dh[:, :60]), np.abs(d_lstm_o).sum(axis=0)]
    assert max(float(b.max()) for b in bound) * 16.0 < 2.0 ** 24, "the case is not exact in fp32"
    saved = np.concatenate([lstm_out.reshape(-1), lstm_o.reshape(-1), gates.reshape(-1)]).astype(np.float32)
    return (x.reshape(n, hf, wf, 512).astype(np.float32), TR.join_tail(w), saved, dh.reshape(n, hf, wf, 64).astype(np.float32), want, g)


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_data_equals_float64_bit_for_bit(shape):
    n, hf, wf = shape
    x, tail, saved, dh, want, g = exact_case(n, hf, wf, 1)
    r = ctpn_amd.tail_backward(x, tail, saved, dh, want_dx=True)
    assert np.array_equal(r.d_x.reshape(-1, 512), want["d_x"].astype(np.float32)) and np.array_equal(r.d_x.astype(np.float64).reshape(-1, 512), want["d_x"])
    v = ctpn_amd.tail_views(r.d_tail)
    for name in TR.TAIL_NAMES:
        assert np.array_equal(v[name].astype(np.float64), g[name]), (shape, name)
    if wf == 1:
        assert not v[KERNEL % "fw"][512:].any() and not v[KERNEL % "bw"][512:].any()
    else:
        assert v[KERNEL % "fw"][512:].any() and v[KERNEL % "bw"][512:].any()


# ---- stage by stage on random data
CASES = [("biased", (1, 1, 1)), ("biased", (1, 15, 2)), ("biased", (1, 16, 3)), ("biased", (1, 17, 20)), ("biased", (3, 11, 20)), ("biased", (1, 33, 1)),
         ("fullscale", (1, 17, 20))]


def device_stages(x, tail, g):
    """every stage the ABI hands out, as {name: array}"""
    n, hf, wf = x.shape[:3]
    f = ctpn_amd.tail_forward(x, tail)
    s = TG.saved_views(f.saved, n, hf, wf)
    b = ctpn_amd.tail_backward(x, tail, f.saved, g, want_dx=True)
    # d_lstm_out for the recurrence's own hook: the two data-gradient GEMMs in float64 from the same d_heads (exactly what feeds bptt up to fp32 rounding)
    w = TR.split_tail(tail)
    wheads = np.concatenate([w["rpn_bbox_pred/weights"], w["rpn_cls_score/weights"]], axis=1).astype(np.float64)
    d_lo = (g.reshape(-1, 64)[:, :60].astype(np.float64) @ wheads.T @ w["lstm_o/weights"].astype(np.float64).T).astype(np.float32)
    d_pre = TG.debug_tail_bptt(d_lo.reshape(n * hf, wf, 256), s["gates"].reshape(n * hf, wf, 2, 5, 128), tail)
    out = {"heads": f.heads[..., :60], "lstm_out": s["lstm_out"], "lstm_o": s["lstm_o"], "d_pre": d_pre.reshape(n, hf, wf, 1024), "d_x": b.d_x}
    for k, name in enumerate(("gate_i", "gate_j", "gate_f", "gate_o", "cell_c")):
        out[name] = s["gates"][..., k, :]
    out.update(ctpn_amd.tail_views(b.d_tail))
    return out, f, b


def ref_stages(r):
    out = {k: r[k] for k in ("heads", "lstm_out", "lstm_o", "d_pre", "d_x")}
    for k, name in enumerate(("gate_i", "gate_j", "gate_f", "gate_o", "cell_c")):
        out[name] = r["gates"][..., k, :]
    out.update(r["d_tail"])
    return out


def stage_errors(kind, shape):
    """{stage: (device error, e32)} of a case against float64 autograd"""
    n, hf, wf = shape
    x, tail, g, r64, r32 = K.reference(n, hf, wf, kind, 3)
    got, _, _ = device_stages(x, tail, g)
    a, b = ref_stages(r64), ref_stages(r32)
    return {k: (K.rel_error(got[k], a[k]), K.rel_error(b[k], a[k])) for k in a}, got


FORWARD_STAGES = ("heads", "lstm_out", "lstm_o", "gate_i", "gate_j", "gate_f", "gate_o", "cell_c")
GRADIENT_STAGES = ("d_pre", "d_x") + tuple(TR.TAIL_NAMES)
# The forward stages are the bytes of the fp32 ctx's forward (test_forward_is_the_fp32_ctx_tail_byte_for_byte), whose products are strictly
# K-ordered fma chains (K = 512 + 128 into a gate) where torch's float32 matmul sums in blocks: a saved gate may sit further from float64 than
# 4 e32 without anything being wrong. They are held to 4 e32 or to the bound the suite has always put on these tensors in the fp32 forward
# (tests/test_gpu_bias_and_saturation.py TOL["fp32"] = REC_TOL["exact"] = FC_TOL: 5e-6 of the tensor's maximum), whichever is larger; a
# swapped, mis-stored or wrongly activated gate is an error of the gate's own size. The gradient stages get the 4 e32 and nothing else.
FORWARD_TOL = 5e-6


@pytest.mark.parametrize("kind,shape", CASES)
def test_every_stage_against_float64_autograd(kind, shape):
    """Worst device / e32 ratio measured over these cases: see profiles/tail_backward_accuracy.json."""
    errs, got = stage_errors(kind, shape)
    assert set(errs) == set(FORWARD_STAGES) | set(GRADIENT_STAGES)
    for k, (e, e32) in errs.items():
        print("%-50s device %.3e  e32 %.3e" % (k, e, e32))
    if kind == "fullscale":      # the case does what it is for: gates at exactly 0 and 1
        assert (got["gate_i"] == 0).any() and (got["gate_i"] == 1).any() and (got["gate_o"] == 0).any()
    bad = {k: errs[k] for k in FORWARD_STAGES if not (errs[k][0] <= max(4.0 * errs[k][1], FORWARD_TOL))}
    bad.update({k: errs[k] for k in GRADIENT_STAGES if not (errs[k][0] <= 4.0 * errs[k][1])})
    assert not bad, bad


# ---- structure
def small_case(n=1, hf=17, wf=20):
    x, tail, g = K.features(n, hf, wf, "biased", 5), K.tail_weights("biased"), K.head_gradient(n, hf, wf, 5)
    return x, tail, g, ctpn_amd.tail_forward(x, tail)


def test_zero_head_gradient_gives_zero():
    x, tail, g, f = small_case()
    b = ctpn_amd.tail_backward(x, tail, f.saved, np.zeros_like(g), want_dx=True)
    assert not b.d_tail.any() and not b.d_x.any()


def test_one_cell_reaches_only_its_side_of_its_row():
    n, hf, wf = 1, 17, 20
    x, tail, _, f = small_case(n, hf, wf)
    row, t = 9, 7
    g = np.zeros((n, hf, wf, 64), np.float32)
    g[0, row, t, :60] = K.head_gradient(1, 1, 1, 6).reshape(-1)[:60]
    w = TR.split_tail(tail)
    wheads = np.concatenate([w["rpn_bbox_pred/weights"], w["rpn_cls_score/weights"]], axis=1)
    d_lo = (g.reshape(-1, 64)[:, :60] @ wheads.T @ w["lstm_o/weights"].T).astype(np.float32).reshape(hf, wf, 256)
    s = TG.saved_views(f.saved, n, hf, wf)
    d_pre = TG.debug_tail_bptt(d_lo, s["gates"].reshape(hf, wf, 2, 5, 128), tail)
    fw, bw = d_pre[..., :512], d_pre[..., 512:]
    assert fw[row, : t + 1].any() and bw[row, t:].any()
    assert not fw[row, t + 1:].any(), "fw runs left to right: nothing right of t depends on cell t"
    assert not bw[row, :t].any(), "bw runs right to left: nothing left of t depends on cell t"
    other = np.arange(hf) != row
    assert not d_pre[other].any()
    d_x = ctpn_amd.tail_backward(x, tail, f.saved, g, want_dx=True).d_x[0]
    assert d_x[row].any() and not d_x[other].any()


def test_batch_gradient_is_the_ordered_sum_of_its_blocks():
    """What the reduction order guarantees (ctpn_hip.h): 48 rows x 16 steps = 3 blocks of 256 cells that end at sequence ends; the batch's
    gradient is ((g_1 + g_2) + g_3) in float32 of the calls on each block's 16 rows alone, bit for bit."""
    n, hf, wf = 3, 16, 16
    x, tail, g, f = small_case(n, hf, wf)
    whole = ctpn_amd.tail_backward(x, tail, f.saved, g).d_tail
    s = TG.saved_views(f.saved, n, hf, wf)
    parts = []
    for i in range(n):
        saved_i = np.concatenate([s[k][i].reshape(-1) for k in ("lstm_out", "lstm_o", "gates")])
        parts.append(ctpn_amd.tail_backward(x[i:i + 1], tail, saved_i, g[i:i + 1]).d_tail)
    assert np.array_equal(whole, (parts[0] + parts[1]) + parts[2])
    assert not np.array_equal(whole, parts[0] + (parts[1] + parts[2])), "the case cannot tell the order"


def test_same_bytes_twice_and_from_device_pointers_and_with_nan_pads():
    x, tail, g, f = small_case(1, 17, 20)
    f2 = ctpn_amd.tail_forward(x, tail)
    assert f.heads.tobytes() == f2.heads.tobytes() and f.saved.tobytes() == f2.saved.tobytes()
    assert not f.heads[..., 60:].any()
    assert ctpn_amd.tail_forward(x, tail, want_saved=False).heads.tobytes() == f.heads.tobytes()
    b1 = ctpn_amd.tail_backward(x, tail, f.saved, g, want_dx=True)
    b2 = ctpn_amd.tail_backward(x, tail, f.saved, g, want_dx=True)
    assert b1.d_tail.tobytes() == b2.d_tail.tobytes() and b1.d_x.tobytes() == b2.d_x.tobytes()
    assert ctpn_amd.tail_backward(x, tail, f.saved, g).d_tail.tobytes() == b1.d_tail.tobytes()
    gn = g.copy()
    gn[..., 60:] = np.nan
    bn = ctpn_amd.tail_backward(x, tail, f.saved, gn, want_dx=True)
    assert bn.d_tail.tobytes() == b1.d_tail.tobytes() and bn.d_x.tobytes() == b1.d_x.tobytes()
    dev = torch.device("cuda", 0)
    before = live()
    xd, td, gd = torch.from_numpy(x).to(dev), torch.from_numpy(tail).to(dev), torch.from_numpy(gn).to(dev)
    fd = ctpn_amd.tail_forward(xd, td)
    assert fd.heads.is_cuda and fd.heads.cpu().numpy().tobytes() == f.heads.tobytes() and fd.saved.cpu().numpy().tobytes() == f.saved.tobytes()
    bd = ctpn_amd.tail_backward(xd, td, fd.saved, gd, want_dx=True)
    assert bd.d_tail.cpu().numpy().tobytes() == b1.d_tail.tobytes() and bd.d_x.cpu().numpy().tobytes() == b1.d_x.tobytes()
    assert live() == before


# ---- the forward is the ctx's own
@pytest.mark.parametrize("hw", [(64, 96), (48, 272)])
def test_forward_is_the_fp32_ctx_tail_byte_for_byte(arena, hw):
    h, w = hw
    imgs = ctpn_amd.weights.synthetic_images(2, h, w, 3)
    with ctpn_amd.Context(0, 2, h, w, "fp32") as ctx:
        ctx.load_weights(arena)
        ctx.forward(imgs)
        x, heads, lstm_out, lstm_o = (ctx.get_tensor(k) for k in ("rpn_conv/3x3", "heads", "lstm_out", "lstm_o"))
    f = ctpn_amd.tail_forward(x, arena[TG.TAIL_OFFSET:])
    s = TG.saved_views(f.saved, *x.shape[:3])
    assert f.heads[..., :60].tobytes() == heads.tobytes()
    assert s["lstm_out"].tobytes() == lstm_out.tobytes() and s["lstm_o"].tobytes() == lstm_o.tobytes()


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_tail_gradients_in_the_other_precisions(arena, prec):
    img, gts = K.finetune_page()
    with ctpn_amd.Context(0, 1, K.FT_H, K.FT_W, prec) as ctx:
        ctx.load_weights(arena)
        losses, grads = ctpn_amd.tail_gradients(ctx, img, gts, cfg=K.finetune_cfg())
        x = ctx.get_tensor("rpn_conv/3x3")
    assert np.isfinite(losses[0]["model_loss"]) and all(np.isfinite(v).all() for v in grads.values()) and list(grads) == TR.TAIL_NAMES
    heads = ctpn_amd.tail_forward(x, arena[TG.TAIL_OFFSET:], want_saved=False).heads
    hf, wf = x.shape[1:3]
    gt5 = np.concatenate([gts[0], np.ones((len(gts[0]), 1), np.float32)], axis=1)
    t = ctpn_amd.anchor_targets(hf, wf, np.array([[K.FT_H, K.FT_W, 1.0]], np.float32), [gt5], cfg=K.finetune_cfg())
    r = ctpn_amd.rpn_loss(heads, t.labels, t.bbox_targets, t.inside_weights, t.outside_weights)
    assert losses[0]["model_loss"] == float(r.losses[0, 2]) and losses[0]["fg"] == int(r.counts[0, 1]) > 0


# ---- arguments
def test_bad_arguments_leave_nothing_behind():
    lib = B.load_library()
    x, tail, g, f = small_case(1, 2, 3)
    before = live()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    heads, d_tail = np.full((6, 64), 7.0, np.float32), np.full(TG.TAIL_FLOATS, 7.0, np.float32)
    assert lib.ctpn_tail_forward(0, 0, 2, 3, vp(x), vp(tail), 0, vp(heads), None) == -1
    assert lib.ctpn_tail_forward(0, 1, 2, 3, None, vp(tail), 0, vp(heads), None) == -1
    assert lib.ctpn_tail_forward(0, 1, 2, 3, vp(x), vp(tail), 3, vp(heads), None) == -1
    assert lib.ctpn_tail_forward(99, 1, 2, 3, vp(x), vp(tail), 0, vp(heads), None) == -1
    assert lib.ctpn_tail_forward(0, 1 << 10, 1 << 10, 3, vp(x), vp(tail), 0, vp(heads), None) == -1
    assert lib.ctpn_tail_backward(0, 1, 2, 3, vp(x), vp(tail), None, vp(g), 0, vp(d_tail), None) == -1
    assert lib.ctpn_tail_backward(0, 1, 2, -3, vp(x), vp(tail), vp(f.saved), vp(g), 0, vp(d_tail), None) == -1
    xd = torch.zeros(6 * 512 + 4, dtype=torch.float32, device="cuda:0")
    assert lib.ctpn_tail_forward(0, 1, 2, 3, C.c_void_p(xd.data_ptr() + 4), C.c_void_p(xd.data_ptr()), 1, C.c_void_p(xd.data_ptr()), None) == -1
    assert (heads == 7.0).all() and (d_tail == 7.0).all() and live() == before
    cur = torch.cuda.current_device()
    assert lib.ctpn_tail_forward(0, 1, 2, 3, vp(x), vp(tail), 0, vp(heads), None) == 0
    assert heads.tobytes() == f.heads.tobytes() and live() == before and torch.cuda.current_device() == cur


# ---- the fine-tune loop
def test_finetune_steps_lower_the_loss_and_touch_the_tail_alone(arena, tmp_path):
    """tests/test_tail_grad.py sets the condition on the CPU (the float64 loss of these steps falls under half); here the device's model_loss
    after the steps is below the one before, and the written arena differs from the input in the tail slice alone."""
    from ctpn_amd.ctpn import finetune_tail as FT
    img, gts = K.finetune_page()
    with ctpn_amd.Context(0, 1, K.FT_H, K.FT_W, "fp32") as ctx:
        new, recs = FT.run_steps(lambda h, w: ctx, arena, [(img[0], gts[0])], K.FT_STEPS, K.FT_LR, K.FT_MOMENTUM, K.finetune_cfg())
        ctx.load_weights(new)
        after = ctpn_amd.score_pages(ctx, img, gts, cfg=K.finetune_cfg())[0]["model_loss"]
    assert len(recs) == K.FT_STEPS and all(np.isfinite(r["model_loss"]) and r["grad_norm"] > 0 for r in recs)
    print([r["model_loss"] for r in recs], after)
    assert after < recs[0]["model_loss"]
    out = str(tmp_path / "arena.npy")
    np.save(out, new)
    back = np.load(out)
    assert np.array_equal(back[: TG.TAIL_OFFSET], arena[: TG.TAIL_OFFSET]) and not np.array_equal(back[TG.TAIL_OFFSET:], arena[TG.TAIL_OFFSET:])
    assert os.path.getsize(out) > 4 * ctpn_amd.WEIGHT_FLOATS
