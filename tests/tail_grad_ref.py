"""Test infrastructure: a torch restatement of the recurrent tail -- rpn_conv/3x3's output to the heads -- with gradients enabled, op for op
oracle/network.py's lstm_pre / lstm_direction / dense (which switch gradients off globally and go through numpy, so they cannot be
differentiated). Gradients come from autograd, in float64 (the reference of every device check) and in float32 (the measure of what an fp32
chain loses: the device is allowed a multiple of ITS error, tests/test_gpu_tail_grad.py). tests/test_tail_grad.py holds this file against
oracle.network bit for bit and against central differences."""
import numpy as np
import torch

TAIL_NAMES = ["lstm_o/bidirectional_rnn/fw/lstm_cell/kernel", "lstm_o/bidirectional_rnn/fw/lstm_cell/bias",
              "lstm_o/bidirectional_rnn/bw/lstm_cell/kernel", "lstm_o/bidirectional_rnn/bw/lstm_cell/bias",
              "lstm_o/weights", "lstm_o/biases", "rpn_bbox_pred/weights", "rpn_bbox_pred/biases", "rpn_cls_score/weights", "rpn_cls_score/biases"]
TAIL_SHAPES = [(640, 512), (512,), (640, 512), (512,), (256, 512), (512,), (512, 40), (40,), (512, 20), (20,)]
TAIL_FLOATS = sum(int(np.prod(s)) for s in TAIL_SHAPES)


def split_tail(flat):
    """a TAIL_FLOATS vector -> {name: view}"""
    flat = np.asarray(flat).reshape(-1)
    assert flat.shape[0] == TAIL_FLOATS
    out, off = {}, 0
    for name, shape in zip(TAIL_NAMES, TAIL_SHAPES):
        k = int(np.prod(shape))
        out[name] = flat[off: off + k].reshape(shape)
        off += k
    return out


def join_tail(views, dtype=np.float32):
    return np.concatenate([np.asarray(views[name], dtype).reshape(-1) for name in TAIL_NAMES])


class _Sigmoid(torch.autograd.Function):
    """oracle.network's sigmoid, 1 / (1 + exp(-x)), with the derivative s (1 - s): autograd through the quotient itself multiplies exp(-x) = inf
    by 1 / inf^2 = 0 once a float32 gate saturates and hands back NaN, where the true slope is 0"""

    @staticmethod
    def forward(ctx, x):
        s = 1.0 / (1.0 + torch.exp(-x))
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        return g * (s * (1.0 - s))


def _sigmoid(x):
    return _Sigmoid.apply(x)


def forward(x, w, keep_z=False):
    """x: tensor (n, hf, wf, 512); w: {name: tensor}; all of one dtype. -> dict of tensors: heads (n, hf, wf, 60), lstm_out, lstm_o,
    gates (n, hf, wf, 2, 5, 128) = activated i, j, f, o and c; with keep_z also "z": the per-step pre-activation tensors z[d][t] (rows, 512)
    with retain_grad set, whose .grad after backward() is d_pre."""
    n, hf, wf, c = x.shape
    xr = x.reshape(n * hf, wf, c)
    R = n * hf
    outs, gates, zs = [], [], []
    for name, reverse in (("fw", False), ("bw", True)):
        k, b = w["lstm_o/bidirectional_rnn/%s/lstm_cell/kernel" % name], w["lstm_o/bidirectional_rnn/%s/lstm_cell/bias" % name]
        h = torch.zeros(R, 128, dtype=x.dtype, device=x.device)
        cs = torch.zeros(R, 128, dtype=x.dtype, device=x.device)
        hs, gs, zd = [None] * wf, [None] * wf, [None] * wf
        for t in (range(wf - 1, -1, -1) if reverse else range(wf)):
            z = torch.cat([xr[:, t, :], h], dim=1) @ k + b
            if keep_z:
                z.retain_grad()
                zd[t] = z
            i, j, f, o = torch.split(z, 128, dim=1)
            ig, jg, fg, og = _sigmoid(i), torch.tanh(j), _sigmoid(f + 1.0), _sigmoid(o)
            cs = fg * cs + ig * jg
            h = og * torch.tanh(cs)
            hs[t] = h
            gs[t] = torch.stack([ig, jg, fg, og, cs], dim=1)      # (R, 5, 128)
        outs.append(torch.stack(hs, dim=1))                       # (R, T, 128)
        gates.append(torch.stack(gs, dim=1))                      # (R, T, 5, 128)
        zs.append(zd)
    lstm_out = torch.cat(outs, dim=-1).reshape(n, hf, wf, 256)
    lstm_o = (lstm_out.reshape(-1, 256) @ w["lstm_o/weights"] + w["lstm_o/biases"]).reshape(n, hf, wf, 512)
    fc = lstm_o.reshape(-1, 512)
    bbox = fc @ w["rpn_bbox_pred/weights"] + w["rpn_bbox_pred/biases"]
    cls = fc @ w["rpn_cls_score/weights"] + w["rpn_cls_score/biases"]
    out = {"heads": torch.cat([bbox, cls], dim=1).reshape(n, hf, wf, 60), "lstm_out": lstm_out, "lstm_o": lstm_o,
           "gates": torch.stack(gates, dim=2).reshape(n, hf, wf, 2, 5, 128)}
    if keep_z:
        out["z"] = zs
    else:      # the hoisted input projection as oracle.network.lstm_pre states it (the device's first GEMM); not on the path to the heads here
        flat = x.reshape(-1, c)
        out["lstm_pre"] = torch.cat([flat @ w["lstm_o/bidirectional_rnn/%s/lstm_cell/kernel" % d][:512] + w["lstm_o/bidirectional_rnn/%s/lstm_cell/bias" % d]
                                     for d in ("fw", "bw")], dim=1).reshape(n, hf, wf, 1024)
    return out


def tensors(x, tail, dtype, grad=True):
    """numpy x and a TAIL_FLOATS vector -> (x tensor, {name: tensor}) of `dtype`, leaves that require gradients"""
    xt = torch.tensor(np.asarray(x, np.float32).astype(np.float64), dtype=dtype, requires_grad=grad)
    w = {k: torch.tensor(np.asarray(v, np.float32).astype(np.float64), dtype=dtype, requires_grad=grad) for k, v in split_tail(tail).items()}
    return xt, w


def gradients(x, tail, d_heads, dtype=torch.float64, d_lstm_out=None):
    """The tail's forward, then the backward of sum(heads * d_heads[..., :60]) by autograd in `dtype` (d_heads None: of sum(lstm_out *
    d_lstm_out), the recurrence alone).
    -> dict of numpy arrays (of that dtype): heads, lstm_out, lstm_o, gates, d_x, d_pre (n, hf, wf, 1024: fw gates | bw gates, TF order), and
    d_tail as {name: array}"""
    with torch.enable_grad():
        xt, w = tensors(x, tail, dtype)
        f = forward(xt, w, keep_z=True)
        if d_heads is not None:
            g = torch.tensor(np.asarray(d_heads, np.float32)[..., :60].astype(np.float64), dtype=dtype)
            (f["heads"] * g).sum().backward()
        else:
            g = torch.tensor(np.asarray(d_lstm_out, np.float32).astype(np.float64), dtype=dtype)
            (f["lstm_out"] * g.reshape(f["lstm_out"].shape)).sum().backward()
    n, hf, wf, _ = xt.shape
    d_pre = np.zeros((n * hf, wf, 1024), xt.grad.numpy().dtype)
    for d in range(2):
        for t in range(wf):
            zg = f["z"][d][t].grad
            d_pre[:, t, d * 512:(d + 1) * 512] = 0.0 if zg is None else zg.numpy()
    out = {k: f[k].detach().numpy() for k in ("heads", "lstm_out", "lstm_o", "gates")}
    out["d_x"] = xt.grad.numpy()
    out["d_pre"] = d_pre.reshape(n, hf, wf, 1024)
    out["d_tail"] = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), d_pre.dtype)) for k, v in w.items()}
    return out


def loss_and_grad64(x, tail, targets):
    """model_loss summed over the batch and its float64 gradient at the tail weights, through anchor_target_ref.rpn_loss_torch per image.
    targets: per image (labels, bbox_targets, inside_weights, outside_weights). -> (losses per image, d_tail flat float64)"""
    import anchor_target_ref as R
    with torch.enable_grad():
        xt, w = tensors(x, tail, torch.float64)
        heads = forward(xt, w)["heads"]
        n = heads.shape[0]
        losses, dh = [], np.zeros(tuple(heads.shape), np.float64)
        for i in range(n):
            loss, g = R.rpn_loss_torch(heads[i].detach().numpy().reshape(-1, 60), *targets[i])
            losses.append(loss)
            dh[i] = g.reshape(dh[i].shape)
        (heads * torch.tensor(dh)).sum().backward()
    return losses, np.concatenate([w[k].grad.numpy().reshape(-1) for k in TAIL_NAMES])
