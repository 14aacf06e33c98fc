"""A training step that stays on the device: lib/fast_rcnn/train.py's loop body over the C ABI.

network_gradients_device is conv_grad.network_gradients on device tensors: the stored activations come through ctx.get_tensor_device (a
kernel, not a host loop), the conv1_1 blob is formed on the device, the weights are views of a device arena and every gradient is written
into one flat device vector in manifest order. It returns the bytes network_gradients returns.

Trainer owns the device arena, the gradient vector and the solver's two state vectors; step() is forward -> gradient -> solver_step ->
ctx.load_weights_device, and nothing larger than the image, its labels and a few scalars crosses PCIe. The three solvers of
cfg.TRAIN.SOLVER (Momentum, Adam, RMS), the weight decay of total_loss and tf.clip_by_global_norm are ctpn_amd.solver's step.

The learning-rate schedule is the reference's, oddity included: at `iter != 0 and iter % STEPSIZE == 0` the loop multiplies the `lr`
VARIABLE by GAMMA, but only MomentumOptimizer was built on that variable -- AdamOptimizer and RMSPropOptimizer were given the constant
cfg.TRAIN.LEARNING_RATE (lib/fast_rcnn/train.py:94-102), so their rate never changes. Trainer keeps that: `lr` in the record is the rate
the step used.

The data layers are ctpn_amd.data_layer: Trainer.step_record takes a DataLayer record -- the page, its blob and its boxes already on the
device -- and a Trainer steps on pages of different sizes in one run: the ctx's capacity is the largest, each forward takes its page's."""
import collections

import numpy as np

from . import _binding as B
from .conv_grad import CONVS, PIXEL_MEANS, POOL_BEFORE, conv_stack_backward
from .solver import decay_table, solver_code, solver_defaults, solver_step, trained_offset, SOLVERS
from .tail_grad import TAIL_OFFSET, tail_backward, tail_forward
from .targets import STAT_NAMES, anchor_targets, rpn_loss
from .weights import MANIFEST, WEIGHT_FLOATS


def _device_arena(arena, device_id):
    import torch
    dev = torch.device("cuda", int(device_id))
    if type(arena).__module__.split(".")[0] == "torch":
        if not arena.is_cuda or arena.device.index != int(device_id) or arena.dtype != torch.float32 or not arena.is_contiguous() or arena.numel() != WEIGHT_FLOATS:
            raise ValueError("the device arena is a contiguous float32 tensor of %d floats on cuda:%d" % (WEIGHT_FLOATS, device_id))
        return arena.reshape(-1)
    a = B._f32(arena).reshape(-1)
    if a.shape[0] != WEIGHT_FLOATS:
        raise ValueError("the arena holds %d floats" % WEIGHT_FLOATS)
    return torch.from_numpy(np.array(a, np.float32)).to(dev)


def _ragged_dev(rows, width, np_dtype, dev):
    """per-image arrays -> (device tensor (total, width) or (total,), offsets): anchor_targets' device form"""
    import torch
    parts = [np.asarray(r, dtype=np_dtype).reshape(-1, width) if width > 1 else np.asarray(r, dtype=np_dtype).reshape(-1) for r in rows]
    offs = np.zeros((len(parts) + 1,), np.int32)
    offs[1:] = np.cumsum([p.shape[0] for p in parts])
    flat = np.ascontiguousarray(np.concatenate(parts, axis=0))
    return torch.from_numpy(flat).to(dev), offs


def network_gradients_device(ctx, images, gt_boxes, gt_hard=None, dontcare=None, cfg=None, seed=0, arena_dev=None, from_layer="conv1_1", out=None, mark=None,
                             images_dev=None, blob_dev=None, gt_dev=None, gt_offsets=None):
    """conv_grad.network_gradients with everything tensor-sized on the device. arena_dev: the WEIGHT_FLOATS weights as a float32 tensor on
    cuda:ctx.device_id -- the weights the ctx has loaded (ctx.load_weights_device(arena_dev.data_ptr())). The ctx option keep_acts must be 1.
    out: a float32 device vector of WEIGHT_FLOATS - trained_offset(from_layer) floats to write into (default: a new one). mark(leg) is called
    when "forward", "fetch" and "backward" are complete on the device (tools/train_step_throughput.py times the legs with it).
    images_dev (a uint8 tensor (n, h, w, 3) on the ctx's device), blob_dev (its float32 blob, image - PIXEL_MEANS; None: formed here) and
    gt_dev (a float32 tensor (total, 5)) with gt_offsets (n + 1 ints) replace images and gt_boxes, which are then None: the forward runs
    from the device pointer and no image, blob or box array is built on the host (a DataLayer record's fields, see Trainer.step_record).
    -> (one dict per image as network_gradients returns, the gradient of the batch's summed model_loss at arena[trained_offset(from_layer):]
    as one flat device tensor in manifest order: the concatenation of network_gradients' arrays, bit for bit)."""
    import torch
    if from_layer not in CONVS:
        raise ValueError("from_layer is one of " + ", ".join(CONVS))
    if ctx.get_option("keep_acts") != 1:
        raise ValueError("network_gradients_device: the ctx option keep_acts is 0; set keep_acts = 1 so that the forward stores every activation")
    dev = torch.device("cuda", int(ctx.device_id))
    arena_dev = _device_arena(arena_dev, ctx.device_id)
    first_off = trained_offset(from_layer)
    if out is None:
        out = torch.empty((WEIGHT_FLOATS - first_off,), dtype=torch.float32, device=dev)
    elif out.dim() != 1 or out.numel() != WEIGHT_FLOATS - first_off:
        raise ValueError("network_gradients_device: out holds %d floats" % (WEIGHT_FLOATS - first_off))
    views = lambda flat, base: {name: flat[off - base: off - base + int(np.prod(shape))].view(shape) for name, shape, off in MANIFEST if off >= base}      # noqa: E731
    weights, g_views = views(arena_dev, 0), views(out, first_off)
    tail = arena_dev[TAIL_OFFSET:]
    if images_dev is not None:
        if images is not None or gt_boxes is not None or gt_dev is None or gt_offsets is None:
            raise ValueError("network_gradients_device: images_dev comes with gt_dev and gt_offsets, in place of images and gt_boxes")
        if not images_dev.is_cuda or images_dev.device != dev or images_dev.dtype != torch.uint8 or images_dev.dim() != 4 or images_dev.shape[3] != 3 or \
                not images_dev.is_contiguous():
            raise ValueError("network_gradients_device: images_dev is a contiguous uint8 tensor (n, h, w, 3) on cuda:%d" % ctx.device_id)
        n, h, w = int(images_dev.shape[0]), int(images_dev.shape[1]), int(images_dev.shape[2])
        if blob_dev is not None and (tuple(blob_dev.shape) != tuple(images_dev.shape) or blob_dev.dtype != torch.float32 or blob_dev.device != dev):
            raise ValueError("network_gradients_device: blob_dev is images_dev's float32 blob")
        torch.cuda.current_stream(dev).synchronize()      # the ctx runs on streams of its own: what torch queued for these tensors is done first
        ctx.forward(None, device_ptr=images_dev.data_ptr(), shape=(n, h, w))
    else:
        images = np.ascontiguousarray(images, dtype=np.uint8)
        n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
        ctx.forward(images)
    if mark:
        ctx.sync()
        mark("forward")
    fn, hf, wf = ctx.feat_shape()
    first = CONVS.index(from_layer)
    need = set(CONVS[max(first - 1, 0):])
    for conv, (pool, full) in POOL_BEFORE.items():
        if CONVS.index(conv) >= first:
            need.add(pool)
        if CONVS.index(conv) > first:
            need.add(full)
    acts = {name: ctx.get_tensor_device(name)[:n] for name in sorted(need)}
    if mark:
        mark("fetch")
    blob = None
    if first == 0:      # image - PIXEL_MEANS in float64, rounded once to float32: numpy's in-place subtraction in network_gradients
        if images_dev is not None and blob_dev is not None:
            blob = blob_dev.contiguous()
        else:
            means = torch.tensor(PIXEL_MEANS.reshape(-1), dtype=torch.float64, device=dev)
            blob = ((images_dev if images_dev is not None else torch.from_numpy(images).to(dev)).to(torch.float64) - means).to(torch.float32)
    x = acts["rpn_conv/3x3"]
    fwd = tail_forward(x, tail, True, ctx.device_id)
    info = np.array([[h, w, 1.0]] * n, np.float32)
    if images_dev is not None:
        gt_offs = np.ascontiguousarray(gt_offsets, dtype=np.int32).reshape(-1)
        gt_dev = gt_dev.reshape(-1, 5)
    else:
        gts = []
        for g in gt_boxes:
            g = np.asarray(g, np.float32).reshape(-1, np.asarray(g).shape[-1] if np.asarray(g).size else 5)
            if g.shape[1] == 4:
                g = np.concatenate([g, np.ones((g.shape[0], 1), np.float32)], axis=1)
            gts.append(g)
        gt_dev, gt_offs = _ragged_dev(gts, 5, np.float32, dev)
    hard_dev = None if gt_hard is None else _ragged_dev(gt_hard, 1, np.int32, dev)[0]
    dc_dev, dc_offs = (None, None) if dontcare is None else _ragged_dev(dontcare, 4, np.float32, dev)
    t = anchor_targets(hf, wf, info, gt_dev, hard_dev, dc_dev, cfg, seed, ctx.device_id, gt_offsets=gt_offs, dc_offsets=dc_offs)
    r = rpn_loss(fwd.heads, t.labels, t.bbox_targets, t.inside_weights, t.outside_weights, True, ctx.device_id)
    bwd = tail_backward(x, tail, fwd.saved, r.d_heads, True, ctx.device_id, out=out[TAIL_OFFSET - first_off:])
    conv_stack_backward(acts, blob, weights, bwd.d_x, from_layer, ctx.device_id, outs=g_views)
    if mark:
        mark("backward")
    losses = []
    for i in range(n):
        losses.append({"rpn_cross_entropy": float(r.losses[i, 0]), "rpn_loss_box": float(r.losses[i, 1]), "model_loss": float(r.losses[i, 2]),
                       "kept": int(r.counts[i, 0]), "fg": int(r.counts[i, 1]), "stats": {k: int(v) for k, v in zip(STAT_NAMES, t.stats[i])}})
    return losses, out


RECORD_FIELDS = ("step", "model_loss", "rpn_cross_entropy", "rpn_loss_box", "reg_loss", "total_loss", "sumsq", "grad_norm", "lr")


class Trainer(object):
    """The reference's training loop body on the device. ctx: a Context with keep_acts = 1 (the Trainer loads the arena into it and reloads it
    after every step); arena: the WEIGHT_FLOATS start weights (numpy, copied); solver: "Momentum" | "Adam" | "RMS"; hyper: the 8 values of
    solver_defaults(solver) (default: those); weight_decay: cfg.TRAIN.WEIGHT_DECAY, on the tensors decay_table names; from_layer: the first
    conv trained; stepsize, gamma: cfg.TRAIN.STEPSIZE, GAMMA -- the schedule of the module docstring (Momentum alone follows it); cfg: the 12
    anchor-target settings (default: the library's)."""

    def __init__(self, ctx, arena, solver="Momentum", hyper=None, weight_decay=0.0005, from_layer="conv1_1", stepsize=50000, gamma=0.1, cfg=None):
        import torch
        self.ctx = ctx
        self.solver = [k for k, v in SOLVERS.items() if v == solver_code(solver)][0]
        self.hyper = solver_defaults(self.solver) if hyper is None else np.array(hyper, np.float64).reshape(-1)
        if self.hyper.shape[0] != 8:
            raise ValueError("hyper is the 8 values of solver_defaults")
        self.weight_decay, self.from_layer, self.stepsize, self.gamma, self.cfg = float(weight_decay), from_layer, int(stepsize), float(gamma), cfg
        if self.stepsize < 1:
            raise ValueError("stepsize >= 1")
        self.first = trained_offset(from_layer)
        self.seg_end, self.seg_decay = decay_table(from_layer, weight_decay)
        dev = torch.device("cuda", int(ctx.device_id))
        self.arena_dev = _device_arena(arena, ctx.device_id).clone()
        count = WEIGHT_FLOATS - self.first
        self.grad = torch.zeros((count,), dtype=torch.float32, device=dev)
        self.s1 = torch.full((count,), float(self.hyper[5]), dtype=torch.float32, device=dev)
        self.s2 = torch.full((count,), float(self.hyper[6]), dtype=torch.float32, device=dev)
        self.iter = 0                                   # steps taken
        self.lr = float(np.float32(self.hyper[0]))      # the reference's float32 `lr` variable
        self._load()

    def _load(self):
        import torch
        torch.cuda.current_stream(self.arena_dev.device).synchronize()
        self.ctx.load_weights_device(self.arena_dev.data_ptr())

    def step_record(self, rec, seed=0, mark=None):
        """one iteration on a DataLayer record: step() with the page, its blob and its boxes taken from the device as they are. The pages of
        one run may differ in size, within the ctx's capacity."""
        g = int(rec.gt_dev.shape[0])
        return self.step(None, None, seed=seed, mark=mark, images_dev=rec.image_dev[None], blob_dev=None if rec.blob_dev is None else rec.blob_dev[None],
                         gt_dev=rec.gt_dev, gt_offsets=np.array([0, g], np.int32))

    def step(self, images, gt_boxes, seed=0, gt_hard=None, dontcare=None, mark=None, images_dev=None, blob_dev=None, gt_dev=None, gt_offsets=None):
        """one iteration on `images` ((n, h, w, 3) uint8 BGR) and their boxes -> the record: RECORD_FIELDS. The losses are the batch's sums
        BEFORE the update; reg_loss is the sum of weight_decay w^2 / 2 over the decayed tensors trained, total_loss = model_loss + reg_loss
        is what the clipped gradient belongs to; sumsq is its squared global norm. mark: network_gradients_device's hook, also called
        with "update" and "load". images_dev, blob_dev, gt_dev, gt_offsets: network_gradients_device's device form (images, gt_boxes None)."""
        if self.iter != 0 and self.iter % self.stepsize == 0:
            self.lr = float(np.float32(np.float64(np.float32(self.lr)) * self.gamma))
        losses, _ = network_gradients_device(self.ctx, images, gt_boxes, gt_hard, dontcare, self.cfg, seed, self.arena_dev, self.from_layer, out=self.grad, mark=mark,
                                             images_dev=images_dev, blob_dev=blob_dev, gt_dev=gt_dev, gt_offsets=gt_offsets)
        hyper = self.hyper.copy()
        if self.solver == "Momentum":
            hyper[0] = self.lr
        sumsq, reg = solver_step(self.solver, self.arena_dev[self.first:], self.grad, self.s1, None if self.solver == "Momentum" else self.s2, hyper,
                                 self.iter + 1, self.seg_end, self.seg_decay, self.ctx.device_id)
        if mark:
            mark("update")
        self._load()
        if mark:
            self.ctx.sync()
            mark("load")
        model = float(sum(d["model_loss"] for d in losses))
        rec = collections.OrderedDict([
            ("step", self.iter), ("model_loss", model), ("rpn_cross_entropy", float(sum(d["rpn_cross_entropy"] for d in losses))),
            ("rpn_loss_box", float(sum(d["rpn_loss_box"] for d in losses))), ("reg_loss", reg), ("total_loss", model + reg), ("sumsq", sumsq),
            ("grad_norm", float(np.sqrt(sumsq))), ("lr", float(hyper[0]))])
        self.iter += 1
        return rec

    def arena(self):
        """the weights now, as a host array"""
        return self.arena_dev.cpu().numpy()

    def snapshot(self, path):
        """an .npz of the arena, the two state vectors, the step count, the lr variable and the settings: what restore needs to go on as if
        the run had not stopped"""
        np.savez(path, arena=self.arena(), s1=self.s1.cpu().numpy(), s2=self.s2.cpu().numpy(), iter=np.int64(self.iter), lr=np.float64(self.lr),
                 solver=np.array(self.solver), hyper=self.hyper, weight_decay=np.float64(self.weight_decay), from_layer=np.array(self.from_layer),
                 stepsize=np.int64(self.stepsize), gamma=np.float64(self.gamma), cfg=np.zeros((0,)) if self.cfg is None else np.asarray(self.cfg, np.float64))

    @classmethod
    def restore(cls, ctx, path):
        """a Trainer on `ctx` from snapshot(path)'s file"""
        import torch
        with np.load(path) as z:
            cfg = None if z["cfg"].size == 0 else z["cfg"]
            tr = cls(ctx, z["arena"], str(z["solver"]), z["hyper"], float(z["weight_decay"]), str(z["from_layer"]), int(z["stepsize"]), float(z["gamma"]), cfg)
            dev = tr.s1.device
            tr.s1.copy_(torch.from_numpy(z["s1"]).to(dev))
            tr.s2.copy_(torch.from_numpy(z["s2"]).to(dev))
            tr.iter, tr.lr = int(z["iter"]), float(z["lr"])
        return tr
