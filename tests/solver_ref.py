"""The solver step and ctpn_get_tensor's unpacking, restated in numpy: what tests/test_solver.py holds against a float64 evaluation and
against csrc/solver_dev.h / csrc/unpack_dev.h compiled for the host, and what tests/test_gpu_train.py holds the device against.

Every float32 operation below is one numpy operation on float32 arrays, so it is rounded once, as the kernels' are (-ffp-contract=off). The
two sums are taken in ctpn_solver_plan's order: lane l of a block adds its quads l, l + 256, ... element by element to one double, the 256
lanes are added pairwise (stride 128 .. 1), the blocks left to right."""
import numpy as np

MOMENTUM, ADAM, RMS = 0, 1, 2
F = np.float32
LANES, UNIT, MAX_BLOCKS = 256, 1024, 2048


def plan(count):
    b = -(-count // MAX_BLOCKS)
    b = max(-(-b // UNIT) * UNIT, UNIT)
    return b, -(-count // b)


def defaults(solver):
    h = np.zeros(8)
    h[0], h[4] = 0.001, 10.0
    if solver == MOMENTUM:
        h[1] = 0.9
    elif solver == ADAM:
        h[1], h[2], h[3] = 0.9, 0.999, 1e-8
    else:
        h[1], h[2], h[3], h[5] = 0.9, 0.0, 1e-10, 1.0
    return h


def decay_per_element(count, seg_end, seg_decay):
    e = np.asarray(seg_end, np.int64)
    assert e[-1] == count and (np.diff(np.concatenate([[0], e])) > 0).all()
    return np.repeat(np.asarray(seg_decay, F), np.diff(np.concatenate([[0], e])))


def grad_total(w, g, d):
    """ge = g + d w; d = 0: g itself"""
    with np.errstate(all="ignore"):
        return np.where(d == 0, g, g + d * w).astype(F)


def sums(w, g, d):
    """(sum ge^2, sum d w^2 / 2) in double, in the plan's order"""
    count = w.shape[0]
    b, nb = plan(count)
    with np.errstate(all="ignore"):
        ge = grad_total(w, g, d).astype(np.float64)
        w64, d64 = w.astype(np.float64), d.astype(np.float64)
        terms = [ge * ge, np.where(d != 0, 0.5 * (d64 * (w64 * w64)), 0.0)]
        out = []
        for t in terms:
            t = np.concatenate([t, np.zeros(nb * b - count)]).reshape(nb, b // UNIT, LANES, 4)
            lane = np.zeros((nb, LANES))
            for r in range(b // UNIT):
                for k in range(4):
                    lane = lane + t[:, r, :, k]
            s = LANES // 2
            while s >= 1:
                lane[:, :s] = lane[:, :s] + lane[:, s: 2 * s]
                s //= 2
            total = 0.0
            for v in lane[:, 0]:
                total = total + float(v)
            out.append(total)
    return out[0], out[1]


def params(solver, hyper, t, sumsq):
    """the float32 constants of the update, as sv_params forms them"""
    h = np.asarray(hyper, np.float64)
    norm = float(np.sqrt(np.float64(sumsq)))
    p = {"clip_on": norm > h[4], "scale": F(h[4] / norm) if norm > h[4] else F(1), "lr": F(h[0]), "eps": F(h[3])}
    if solver == MOMENTUM:
        p["a"] = F(h[1])
    elif solver == ADAM:
        p["one_m_a"], p["one_m_b"] = F(1) - F(h[1]), F(1) - F(h[2])
        p["lr_t"] = F(h[0] * np.sqrt(1.0 - float(h[2]) ** float(t)) / (1.0 - float(h[1]) ** float(t)))
    else:
        p["one_m_a"], p["a"] = F(1) - F(h[1]), F(h[2])
    return p


def update(solver, p, w, g, s1, s2, d, dtype=F):
    """the per-element update on arrays of `dtype`: float32 is the kernels' arithmetic; float64 with the same constants is the exact
    evaluation test_solver.py bounds it against -> (w, s1, s2)"""
    c = lambda v: dtype(v)      # noqa: E731
    w, g, s1, d = w.astype(dtype), g.astype(dtype), s1.astype(dtype), d.astype(dtype)
    s2 = None if s2 is None else s2.astype(dtype)
    with np.errstate(all="ignore"):
        ge = np.where(d == 0, g, g + d * w)
        gc = ge * c(p["scale"]) if p["clip_on"] else ge
        if solver == MOMENTUM:
            s1 = c(p["a"]) * s1 + gc
            w = w - c(p["lr"]) * s1
        elif solver == ADAM:
            s1 = s1 + (gc - s1) * c(p["one_m_a"])
            s2 = s2 + (gc * gc - s2) * c(p["one_m_b"])
            w = w - (s1 * c(p["lr_t"])) / (np.sqrt(s2) + c(p["eps"]))
        else:
            s1 = s1 + (gc * gc - s1) * c(p["one_m_a"])
            s2 = s2 * c(p["a"]) + (gc * c(p["lr"])) / np.sqrt(s1 + c(p["eps"]))
            w = w - s2
    return w, s1, s2


def step(solver, w, g, s1, s2, seg_end, seg_decay, hyper, t, sumsq=None):
    """ctpn_solver_step -> (w, s1, s2, (sumsq, reg)); sumsq: take the clip's norm from this sum instead of the restatement's own (the device's
    out2[0]: the order of a sum must not decide a comparison of the update)"""
    d = decay_per_element(w.shape[0], seg_end, seg_decay)
    sq, reg = sums(w, g, d)
    p = params(solver, hyper, t, sq if sumsq is None else sumsq)
    w2, a, b = update(solver, p, w, g, s1, s2, d)
    return w2, a, b, (sq, reg)


# ---- ctpn_get_tensor's host loop
F32, BF16, F16, SPLIT = 0, 1, 2, 3


def gate_col(c):
    g, u = c >> 7, c & 127
    return (u >> 4) * 64 + ((u >> 2) & 3) * 16 + g * 4 + (u & 3)


def widen(a16, kind):
    if kind == F16:      # a signalling NaN comes out quiet, as a hardware convert (and the library's host loop) leaves it; numpy keeps the bits
        out = a16.view(np.float16).astype(F)
        bits = out.view(np.uint32)
        return np.where(np.isnan(out), bits | np.uint32(0x400000), bits).astype(np.uint32).view(F)
    return (a16.astype(np.uint32) << 16).view(F)


def unpack(src, n, H, W, C, ld, border, kind, gates):
    """src: the stored block, a flat float32 (F32) or uint16 array of n (H + 2 border) (W + 2 border) ld values -> (n, H, W, C) float32"""
    Hs, Ws = H + 2 * border, W + 2 * border
    blk = src.reshape(n, Hs, Ws, ld)[:, border: border + H, border: border + W]
    if gates:
        cols = np.array([(ch & ~511) + gate_col(ch & 511) for ch in range(1024)])
        blk = blk[..., cols]
    if kind == F32:
        return np.ascontiguousarray(blk[..., :C], dtype=F)
    if kind == SPLIT:
        return widen(np.ascontiguousarray(blk[..., :C]), BF16) + widen(np.ascontiguousarray(blk[..., C: 2 * C]), BF16)
    return widen(np.ascontiguousarray(blk[..., :C]), kind)
