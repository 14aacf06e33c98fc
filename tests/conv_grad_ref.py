"""Test infrastructure: a torch restatement of the conv stack -- conv + bias + ReLU, 2x2 max-pool -- with gradients enabled, op for op
oracle/network.py's conv3x3_relu / maxpool2x2 (which switch gradients off globally and go through numpy, so they cannot be differentiated).
Gradients come from autograd, in float64 (the reference of every device check) and in float32 (the measure of what an fp32 chain loses).
tests/test_conv_grad.py holds this file against oracle.network bit for bit, against central differences and on tied pool windows."""
import numpy as np
import torch
import torch.nn.functional as F

import tail_grad_ref as TR

CONVS = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2", "conv5_3",
         "rpn_conv/3x3"]
POOL_AFTER = {"conv1_2": "pool1", "conv2_2": "pool2", "conv3_3": "pool3", "conv4_3": "pool4"}
CHANNELS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512), (512, 512),
            (512, 512), (512, 512)]
LEVEL = [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4]      # how many pools lie in front of the conv


def layer_shapes(n, h, w):
    """(name, (n, h_l, w_l, ci, co)) of the 14 convs for an h x w input"""
    return [(name, (n, h >> lv, w >> lv, ci, co)) for name, (ci, co), lv in zip(CONVS, CHANNELS, LEVEL)]


def t(a, dtype, grad=False):
    """numpy (float32 values) -> a torch leaf of `dtype`"""
    return torch.tensor(np.asarray(a).astype(np.float64), dtype=dtype, requires_grad=grad)


def conv(x_nhwc, w_hwio, b=None):
    """oracle.network.conv3x3_relu's conv2d call on tensors: NHWC in, NHWC out (a permuted view, as there)"""
    y = F.conv2d(x_nhwc.permute(0, 3, 1, 2), w_hwio.permute(3, 2, 0, 1), b, stride=1, padding=1)
    return y.permute(0, 2, 3, 1)


def conv_relu(x_nhwc, w_hwio, b):
    return torch.relu(conv(x_nhwc, w_hwio, b))


def pool(x_nhwc):
    return F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), kernel_size=2, stride=2, padding=0).permute(0, 2, 3, 1)


def stack_forward(blob, w, first=0):
    """blob: the tensor fed to CONVS[first]; w: {name: tensor}. -> {name: tensor} of every conv and pool output from there on"""
    out = {}
    x = blob
    for name in CONVS[first:]:
        x = conv_relu(x, w[name + "/weights"], w[name + "/biases"])
        out[name] = x
        if name in POOL_AFTER:
            x = pool(x)
            out[POOL_AFTER[name]] = x
    return out


def conv_backward(x, w, y, d_y, dtype=torch.float64):
    """ONE layer's backward with the mask as an input: dZ = d_y where the given post-ReLU output y is positive, then autograd through the linear
    conv alone. -> (d_w (3, 3, ci, co), d_b (co,), d_x (n, h, w, ci)) numpy of `dtype`"""
    dz = t(np.where(np.asarray(y) > 0, np.asarray(d_y), 0.0), dtype)
    with torch.enable_grad():
        xt, wt = t(x, dtype, True), t(w, dtype, True)
        (conv(xt, wt) * dz).sum().backward()
    return wt.grad.numpy(), dz.sum(dim=(0, 1, 2)).numpy(), xt.grad.numpy()


def conv_backward_abs(x, w, y, d_y):
    """the sums of |a_i b_i| behind every element of conv_backward's three results, float64: what an a priori rounding bound multiplies"""
    dz = np.where(np.asarray(y) > 0, np.abs(np.asarray(d_y, np.float64)), 0.0)
    return conv_backward(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.ones_like(dz), dz, torch.float64)


def pool_backward(y_full, d_pool, dtype=torch.float64):
    """autograd through max_pool2d -> d_full numpy"""
    with torch.enable_grad():
        yt = t(y_full, dtype, True)
        if yt.shape[1] < 2 or yt.shape[2] < 2:      # an empty pooled map: nothing reaches y_full
            return np.zeros(tuple(yt.shape), yt.detach().numpy().dtype)
        (pool(yt) * t(d_pool, dtype)).sum().backward()
    return yt.grad.numpy()


def network_loss_gradients(images_blob, arena_views, targets, dtype=torch.float64, first=0):
    """The whole network from CONVS[first] on: conv stack, the tail (tail_grad_ref.forward), model_loss through anchor_target_ref.rpn_loss_torch
    per image (its gradient at the heads is taken in float64 from this dtype's heads, as the device takes it), backward by autograd in `dtype`.
    targets: per image (labels, bbox_targets, inside_weights, outside_weights). -> (losses per image, {name: gradient} for the convs from
    `first` on and the ten tail tensors, {name: activation})"""
    import anchor_target_ref as R
    names = [c + s for c in CONVS[first:] for s in ("/weights", "/biases")] + TR.TAIL_NAMES
    with torch.enable_grad():
        w = {k: t(arena_views[k], dtype, True) for k in names}
        acts = stack_forward(t(images_blob, dtype), w, first)
        heads = TR.forward(acts["rpn_conv/3x3"], w)["heads"]
        n = heads.shape[0]
        losses, dh = [], np.zeros(tuple(heads.shape), np.float64)
        for i in range(n):
            loss, g = R.rpn_loss_torch(heads[i].detach().numpy().astype(np.float64).reshape(-1, 60), *targets[i])
            losses.append(loss)
            dh[i] = np.asarray(g).reshape(dh[i].shape)
        (heads * torch.tensor(dh, dtype=dtype)).sum().backward()
    grads = {k: (w[k].grad.numpy() if w[k].grad is not None else np.zeros(tuple(w[k].shape))) for k in names}
    return losses, grads, {k: v.detach().numpy() for k, v in acts.items()}
