"""The solver step over the C ABI (include/ctpn_hip.h, "the solver step"): one step of lib/fast_rcnn/train.py's optimiser -- the gradient of
total_loss formed from the gradient of model_loss and the weight decay, tf.clip_by_global_norm, then Momentum, Adam (ApplyAdam) or RMSProp
(ApplyRMSProp) -- on flat float32 vectors. solver_step takes numpy arrays, or torch tensors on the device, which go through on_device = 1
with no host copy; both are updated in place. decay_table is the reference's choice of what is decayed (lib/networks/network.py: every
`weights` made by make_var with a regulariser; no bias, neither LSTMCell kernel). ctpn_amd.train chains a ctx's forward, the gradient and
this step into a training step that stays on the device."""
import ctypes as C

import numpy as np

from . import _binding as B
from .targets import _dev_ptr, _is_torch
from .weights import MANIFEST, WEIGHT_FLOATS

SOLVERS = {"Momentum": 0, "Adam": 1, "RMS": 2}
HYPER_NAMES = ("lr", "a", "b", "epsilon", "clip_norm", "s1_init", "s2_init", "reserved")
MAX_SEGMENTS = 64


def solver_code(solver):
    """'Momentum' | 'Adam' | 'RMS' (cfg.TRAIN.SOLVER's values) or the ABI's 0 | 1 | 2 -> the ABI's code"""
    if isinstance(solver, str):
        if solver not in SOLVERS:
            raise ValueError("solver is one of " + ", ".join(SOLVERS))
        return SOLVERS[solver]
    if int(solver) not in SOLVERS.values():
        raise ValueError("solver is 0 (Momentum), 1 (Adam) or 2 (RMS)")
    return int(solver)


def solver_plan(count):
    """ctpn_solver_plan -> (block_floats, blocks): the fixed order of the two sums, a function of count alone. Needs no device."""
    bf, nb = C.c_longlong(0), C.c_int(0)
    B._check(B.load_library().ctpn_solver_plan(int(count), C.byref(bf), C.byref(nb)))
    return int(bf.value), int(nb.value)


def solver_defaults(solver):
    """ctpn_solver_defaults -> hyper8 (float64): lr, momentum | beta1 | decay, - | beta2 | RMS momentum, epsilon, clip norm, the values s1
    and s2 start at (RMS: ms = 1), zero. Needs no device."""
    h = np.zeros((8,), np.float64)
    B._check(B.load_library().ctpn_solver_defaults(solver_code(solver), B._ptr(h, C.c_double)))
    return h


def trained_offset(from_layer):
    """the arena offset of from_layer's weights: arena[offset:] is what a loop from that layer on trains"""
    for name, _, off in MANIFEST:
        if name == from_layer + "/weights":
            return off
    raise ValueError("from_layer names a conv of the manifest")


def decayed(name):
    """does the reference put an L2 term on this tensor: make_var's regulariser reaches the convs' `weights`, lstm_o/weights and the two
    heads' weights (lib/networks/network.py:91-93, 146, 166); biases are made without one and the LSTMCell makes its own variables"""
    return name.endswith("/weights")


def decay_table(from_layer="conv1_1", weight_decay=0.0005):
    """-> (seg_end int64, seg_decay float32) for arena[trained_offset(from_layer):]: one segment per run of tensors with the same decay"""
    first = trained_offset(from_layer)
    ends, decays = [], []
    for name, shape, off in MANIFEST:
        if off < first:
            continue
        d = float(weight_decay) if decayed(name) else 0.0
        end = off + int(np.prod(shape)) - first
        if decays and decays[-1] == d:
            ends[-1] = end
        else:
            ends.append(end)
            decays.append(d)
    assert ends[-1] == WEIGHT_FLOATS - first
    return np.array(ends, np.int64), np.array(decays, np.float32)


def _segments(count, seg_end, seg_decay):
    if seg_end is None:
        seg_end, seg_decay = [count], [0.0 if seg_decay is None else float(seg_decay)]
    e = np.ascontiguousarray(seg_end, dtype=np.int64).reshape(-1)
    d = np.ascontiguousarray(seg_decay, dtype=np.float32).reshape(-1)
    if e.shape[0] != d.shape[0] or not 1 <= e.shape[0] <= MAX_SEGMENTS:
        raise ValueError("solver_step: seg_end and seg_decay hold the same 1 .. %d entries" % MAX_SEGMENTS)
    return e, d


def solver_step(solver, w, g, s1, s2, hyper, t, seg_end=None, seg_decay=None, device_id=0):
    """ctpn_solver_step: w, s1, s2 updated IN PLACE -> (sumsq, reg_loss) = (sum of ge^2, sum of decay w^2 / 2) of the weights before the update.
    w, g, s1, s2: flat float32 vectors of one length, all numpy (C-contiguous, writable) or all torch tensors on cuda:device_id (any 4-byte
    alignment: views at an offset are fine); s2 may be None for Momentum. hyper: the 8 values of solver_defaults; t: the 1-based step;
    seg_end / seg_decay: decay_table's pair (default: one segment without decay). A gradient whose sum of squares is not finite raises
    CtpnError and leaves the vectors as they were."""
    lib = B.load_library()
    code = solver_code(solver)
    h = np.ascontiguousarray(hyper, dtype=np.float64).reshape(-1)
    if h.shape[0] != 8:
        raise ValueError("hyper is the 8 values of solver_defaults")
    vecs = [("w", w), ("g", g), ("s1", s1), ("s2", s2)]
    if s2 is None and code != 0:
        raise ValueError("solver_step: only Momentum runs without s2")
    count = int(w.numel()) if _is_torch(w) else int(np.asarray(w).size)
    e, d = _segments(count, seg_end, seg_decay)
    out2 = np.zeros((2,), np.float64)
    if _is_torch(w):
        import torch
        dev = torch.device("cuda", int(device_id))
        ptrs = []
        for name, v in vecs:
            if v is not None and (v.dim() != 1 or int(v.numel()) != count):
                raise ValueError("solver_step: %s is a flat vector of w's length" % name)
            ptrs.append(_dev_ptr(v, torch.float32, device_id, name))
        torch.cuda.current_stream(dev).synchronize()      # the call runs on a stream of its own: what torch queued for these tensors is done first
        on_dev = 1
    else:
        ptrs = []
        for name, v in vecs:
            if v is None:
                ptrs.append(None)
                continue
            if not isinstance(v, np.ndarray) or v.dtype != np.float32 or v.ndim != 1 or v.size != count or not v.flags.c_contiguous or \
                    (name != "g" and not v.flags.writeable):
                raise ValueError("solver_step: %s is a flat C-contiguous float32 array of w's length (it is updated in place)" % name)
            ptrs.append(v.ctypes.data_as(C.c_void_p))
        on_dev = 0
    B._check(lib.ctpn_solver_step(int(device_id), code, count, ptrs[0], ptrs[1], ptrs[2], ptrs[3], e.ctypes.data_as(C.POINTER(C.c_longlong)),
                                  B._ptr(d, C.c_float), int(e.shape[0]), B._ptr(h, C.c_double), int(t), on_dev, B._ptr(out2, C.c_double)))
    return float(out2[0]), float(out2[1])
