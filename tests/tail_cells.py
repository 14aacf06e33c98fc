"""The kernels behind the conv stack, one at a time: the cells of lstm_pre's launch shapes, the data recipes, the float64 references and the
numpy models (with one defect each) that tests/test_tail_cells.py (CPU) and tests/test_gpu_tail_kernels.py (device) share. No device needed.

A CELL of lstm_pre (16-bit modes, csrc/lstm_pre.hip) is everything that changes what a wave of the kernel does:
    precision / form (small | lds) / waves per workgroup W / tail class of the last 32-cell group / whole idle waves in the last workgroup
written as one string, e.g. "fp16/lds/w5/t17-31/idle1". W sets how the 32 DMA pieces of a weight tile are dealt over the waves and so the
argument of every counted wait that hands an LDS buffer of the ring to the next tile; the tail class says which of the two store halves of
the last wave are masked; an idle wave has clamped loads and masked stores but takes part in every barrier and DMA.

The plan comes from the library (ctpn_debug_lstm_pre_plan: the function launch_lstm_pre follows) with cu_count = 2: one group of 32 cells
takes the small form, G > 1 groups W = min(ceil(G / 2), 12), so 24 groups (768 cells) reach every W. census() returns {cell: smallest
(n, hf, wf)} over n 1..3, hf in {1, 2, 3, 5}, every wf up to 768 cells, preferring n > 1 and hf > 1 (the map's row and image strides then
matter); tail_cell_cases.CASES is the committed table (regenerate from the repository root: PYTHONPATH=. python tests/tail_cells.py >
tests/tail_cell_cases.py)."""
import functools

import numpy as np

from ctpn_amd import _binding as B
from oracle.rounding import bf16_round, fp16_round

CU = 2                                         # the CU count the table's launch shapes are planned for
PRECS16 = ("fp16", "bf16")
MAX_CELLS = 768
GRID_N = (1, 2, 3)
GRID_HF = (1, 2, 3, 5)
TAILS = ("t0", "t1-15", "t16", "t17-31")
# the project's per-mode bounds (tests/test_gpu_conv_forms.py::BOUND): max |diff| over the map's max |value|, no element beyond 4 x
BOUND = {"fp32": 5e-6, "split": 2e-5, "fp16": 1.5e-3, "bf16": 8e-3}
# the recurrence: max |diff| of outputs bounded by 1 (tests/test_gpu_bias_and_saturation.py::REC_TOL), by launch_bilstm's form
REC_TOL = {"exact": 5e-6, "exact_fast_gates": 2e-5, "split_16": 3e-5, "split_few": 3e-5}
# fp32 and split precision compute lstm_pre by the im2col GEMM: one form, no W; these M put a tail into its 128-row tile, (n, hf, wf)
IGEMM_PRE_SHAPES = ((1, 1, 1), (1, 1, 31), (1, 3, 11), (2, 8, 256), (1, 17, 241))


def tail_class(cells):
    r = cells % 32
    return "t0" if r == 0 else ("t16" if r == 16 else ("t1-15" if r < 16 else "t17-31"))


def cell_name(prec, plan, cells):
    return "%s/%s/w%d/%s/idle%d" % (prec, plan.form, plan.waves, tail_class(cells), 1 if plan.idle_waves > 0 else 0)


def case_cell(prec, case, cu=CU):
    n, hf, wf = case
    return cell_name(prec, B.lstm_pre_plan(n * hf * wf, cu), n * hf * wf)


def census(cu=CU):
    found = {}
    for n in GRID_N:
        for hf in GRID_HF:
            for wf in range(1, MAX_CELLS // (n * hf) + 1):
                cells = n * hf * wf
                key = cell_name("", B.lstm_pre_plan(cells, cu), cells)
                cand = (not (n > 1 and hf > 1), cells, n, hf, wf)
                if key not in found or cand < found[key]:
                    found[key] = cand
    return {prec + key: cand[2:] for key, cand in found.items() for prec in PRECS16}


# ---------------------------------------------------------------------------------------------------------------
# layouts restated: csrc/bilstm.hip lstm_gate_col, csrc/lstm_pre.hip's column tiles
# ---------------------------------------------------------------------------------------------------------------
def gate_col(c, swap_f_j=False):
    """TF gate column c = g * 128 + u of one direction -> column of the permuted lstm_pre layout"""
    g, u = c >> 7, c & 127
    if swap_f_j and g in (1, 2):
        g = 3 - g
    return (u >> 4) * 64 + ((u >> 2) & 3) * 16 + g * 4 + (u & 3)


def gate_perm(swap_f_j=False):
    """perm[c] = the device column of TF column c, both directions (1024)"""
    return np.array([(c & ~511) + gate_col(c & 511, swap_f_j) for c in range(1024)])


def operand(prec, a):
    """fp32 array -> the values the mode's kernels multiply"""
    a = np.asarray(a, np.float32)
    if prec == "bf16":
        return bf16_round(a)
    if prec == "fp16":
        return fp16_round(a)
    if prec == "split":
        hi = bf16_round(a)
        return hi + bf16_round(a - hi)
    return a


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------------------------------------------
# data recipes (seeded; nothing is read from outside the repository)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pre_problem(recipe, prec, cells):
    """(x [cells][512], wx [512][1024], bias [1024], float64 reference [cells][1024]); a case takes the first n * hf * wf cells.
    exact: integers, every product and partial sum exact in fp32 in any order -- the only rounding left is the output store.
    normal: ReLU'd normals x 3, He-scaled weights, a bias of size 0.1, rounded to the operand type first."""
    rng = np.random.default_rng({"exact": 11, "normal": 23}[recipe] * 1000 + cells)
    if recipe == "exact":
        x = rng.integers(-6, 7, (cells, 512)).astype(np.float32)
        wx = rng.integers(-6, 7, (512, 1024)).astype(np.float32)
        # the sums x @ wx have a standard deviation of ~320: a bias of +-(2100 .. 3000) puts an output between 2048 and 4096, where fp16 holds
        # even integers only and every odd one is an exact tie; the other half of the columns takes any integer up to +-3000
        big = rng.integers(2100, 3001, 1024) * rng.choice((-1, 1), 1024)
        bias = np.where(rng.random(1024) < 0.5, big, rng.integers(-3000, 3001, 1024)).astype(np.float32)
        assert (np.abs(x).astype(np.float64) @ np.abs(wx).astype(np.float64) + np.abs(bias)).max() < 2 ** 24
    else:
        x = operand(prec, np.maximum(rng.standard_normal((cells, 512)).astype(np.float32), 0) * 3.0)
        wx = operand(prec, (rng.standard_normal((512, 1024)) * np.sqrt(2.0 / 512)).astype(np.float32))
        bias = (rng.standard_normal(1024) * 0.1).astype(np.float32)
    ref = x.astype(np.float64) @ wx.astype(np.float64) + bias.astype(np.float64)
    return _frozen(x, wx, bias, ref)


@functools.lru_cache(maxsize=None)
def gemm_problem(recipe, M, K, Co):
    """(a [M][K], w [K][Co], bias [Co], float64 reference [M][Co]) for the fp32 GEMM"""
    rng = np.random.default_rng(({"exact": 5, "normal": 7}[recipe] * 8192 + K) * 8192 + Co)
    if recipe == "exact":
        a = rng.integers(-6, 7, (M, K)).astype(np.float32)
        w = rng.integers(-6, 7, (K, Co)).astype(np.float32)
        bias = rng.integers(-3000, 3001, Co).astype(np.float32)
        assert (np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64) + np.abs(bias)).max() < 2 ** 24
    else:
        a = (rng.standard_normal((M, K)) * 0.5).astype(np.float32)          # lstm_out-like: bounded by 1
        w = (rng.standard_normal((K, Co)) * np.sqrt(2.0 / K)).astype(np.float32)
        bias = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64) + bias.astype(np.float64)
    return _frozen(a, w, bias, ref)


REC_RECIPES = ("normal", "saturated", "growth", "growth_neg")


@functools.lru_cache(maxsize=None)
def rec_problem(recipe, rows, T, pre_f16):
    """(pre [rows][T][1024] in TF's order, wh [2][128][512]); pre is rounded to fp16 where the kernel reads fp16.
    normal: sigma 1.5. saturated: sigma 30 clipped to +-100 (the range of the fullscale arena). growth: i, j, f held at +30, so c_t = t;
    growth_neg: j at -30, c_t = -t."""
    rng = np.random.default_rng(((REC_RECIPES.index(recipe) * 1000 + rows) * 1000 + T) * 2 + int(pre_f16))
    wh = (rng.standard_normal((2, 128, 512)) / np.sqrt(128.0)).astype(np.float32)
    pre = (rng.standard_normal((rows, T, 1024)) * 1.5).astype(np.float32)
    if recipe == "saturated":
        pre = np.clip(rng.standard_normal((rows, T, 1024)) * 30.0, -100.0, 100.0).astype(np.float32)
    elif recipe in ("growth", "growth_neg"):
        p = pre.reshape(rows, T, 2, 4, 128)
        p[:, :, :, 0] = 30.0
        p[:, :, :, 1] = 30.0 if recipe == "growth" else -30.0
        p[:, :, :, 2] = 30.0
    if pre_f16:
        pre = fp16_round(pre)
    return _frozen(pre, wh)


# ---------------------------------------------------------------------------------------------------------------
# float64 references and models of the kernels; `defect` names ONE deliberate error (tests/test_tail_cells.py: the checks have teeth)
# ---------------------------------------------------------------------------------------------------------------
def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def bilstm_ref(pre, wh, defect=None):
    """The TF-1.3 LSTMCell recurrence of oracle/network.py::bilstm_from_pre in float64: pre [rows][T][1024] (fw gates | bw gates, i j f o),
    wh [2][128][512] -> [rows][T][256]"""
    pre = np.asarray(pre, np.float64)
    wh = np.asarray(wh, np.float64)
    rows, T, _ = pre.shape
    out = np.zeros((rows, T, 256))
    for d in range(2):
        reverse = d == 1 and defect != "bw_not_reversed"
        h, h_old, c = np.zeros((rows, 128)), np.zeros((rows, 128)), np.zeros((rows, 128))
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            z = pre[:, t, d * 512:(d + 1) * 512] + (h_old if defect == "h_two_back" else h) @ wh[d]
            i, j, f, o = z[:, :128], z[:, 128:256], z[:, 256:384], z[:, 384:]
            c = _sigmoid(f + (0.0 if defect == "no_forget_bias" else 1.0)) * c + _sigmoid(i) * np.tanh(j)
            h_old, h = h, _sigmoid(o) * np.tanh(c)
            out[:, t, d * 128:(d + 1) * 128] = h
    return out


def f16_store(v, mode="rne"):
    """float64 values -> the fp16 a store holds, as float64. rne: round to nearest, ties to even (v_cvt_pk_f16_f32); trunc: toward zero;
    away: to nearest, ties away from zero"""
    v = np.asarray(v, np.float64)
    r = v.astype(np.float16)
    if mode == "rne":
        return r.astype(np.float64)
    r64 = r.astype(np.float64)
    lo = np.where(np.abs(r64) > np.abs(v), np.nextafter(r, np.float16(0)), r).astype(np.float16)      # the neighbour toward zero
    if mode == "trunc":
        return lo.astype(np.float64)
    lo64 = lo.astype(np.float64)
    hi64 = np.nextafter(lo, np.where(v < 0, -np.inf, np.inf).astype(np.float16)).astype(np.float64)
    tie = (lo64 != v) & (np.abs(v - lo64) == np.abs(hi64 - v))
    return np.where(tie, hi64, r64)


def lstm_pre_model(x, wx, bias, defect=None):
    """lstm_pre of the 16-bit modes as the device computes it, in TF's column order: weights and bias permuted to the device's columns (rows
    of wt_x), fp32-class accumulation from the bias, an fp16 store, columns put back"""
    x, wx, bias = (np.asarray(a, np.float64) for a in (x, wx, bias))
    perm = gate_perm()
    pack = gate_perm(swap_f_j=True) if defect == "swap_f_j" else perm        # where the weight chain puts TF column c
    wp = np.zeros_like(wx)
    bp = np.zeros_like(bias)
    wp[:, pack] = wx
    bp[pack] = bias
    if defect == "bias_tf_order":
        bp = bias.copy()
    if defect == "stale_kslice":      # k-slice 9 of column tile 5 read from the LDS buffer's next occupant, tile 5 + 4
        wp[16 * 9:16 * 10, 32 * 5:32 * 6] = wp[16 * 9:16 * 10, 32 * 9:32 * 10]
    if defect == "bias_after_cvt":    # the sum stored as fp16 first, the bias added to that in fp16
        acc = f16_store(f16_store(x @ wp) + f16_store(bp))
    else:
        acc = f16_store(x @ wp + bp, {"f16_trunc": "trunc", "f16_ties_away": "away"}.get(defect, "rne"))
    return acc[:, perm]


def gemm_model(a, w, bias, defect=None):
    a, w, bias = (np.asarray(v, np.float64) for v in (a, w, bias))
    if defect == "drop_last_k":       # the last 128-byte K step (32 fp32) never multiplied
        return a[:, :-32] @ w[:-32] + bias
    return a @ w + bias


def rel_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-30))


if __name__ == "__main__":
    cells = census()
    print('"""Generated by `python tests/tail_cells.py`: cell -> (n, hf, wf), the smallest map of the census (tests/tail_cells.py) that reaches the\n'
          'cell when launch_lstm_pre plans for %d CUs. %d cells."""' % (CU, len(cells)))
    print("CASES = {")
    for cell in sorted(cells):
        print("    %r: %r," % (cell, tuple(int(v) for v in cells[cell])))
    print("}")
