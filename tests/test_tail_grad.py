"""CPU: the backward pass through the recurrent tail (include/ctpn_hip.h, "the recurrent tail: forward with saved activations, backward")
without a device.
  * tests/tail_grad_ref.py, the torch restatement with gradients, is held first: its float32 forward equals oracle.network's lstm_pre / bilstm /
    dense bit for bit, and its float64 autograd gradient agrees with central differences of the float64 loss along seeded random directions in
    weight space and in x (float64 on the CPU only; no finite differences are taken on the device);
  * csrc/tail_grad_dev.h, the kernels' per-thread text, compiled with g++ under ASan + UBSan as a stand-alone program
    (tests/tail_grad_host.cpp) and run as a subprocess over whole small problems from exact-size heap blocks, against the restatement; four
    mutants of the cell update each fail that comparison;
  * the fine-tune loop's condition: the steps ctpn/finetune_tail.py takes, run through the float64 restatement on oracle.network's features of
    the labelled page, bring the float64 loss under half (the GPU test then only asks for a smaller loss);
  * the three symbols in header, library and binding; bad arguments refused before any device work; no device: CTPN_ERR_NODEVICE."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import anchor_target_ref as R
import ctpn_amd
import tail_grad_cases as K
import tail_grad_ref as TR
from ctpn_amd import _binding as B
from ctpn_amd import tail_grad as TG
from oracle import network as N

GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all"]
NEW = ("ctpn_tail_saved_floats", "ctpn_tail_forward", "ctpn_tail_backward")


# ---- the restatement
def test_restatement_forward_equals_the_oracle_bit_for_bit():
    x, tail = K.features(2, 2, 5, "biased", 1), K.tail_weights("biased")
    w = TR.split_tail(tail)
    with torch.no_grad():
        xt, wt = TR.tensors(x, tail, torch.float32, grad=False)
        f = {k: v.numpy() for k, v in TR.forward(xt, wt).items()}
    assert np.array_equal(f["lstm_pre"], N.lstm_pre(x, w))
    lo = N.bilstm(x, w)
    assert np.array_equal(f["lstm_out"], lo)
    fc = N.dense(lo, w["lstm_o/weights"], w["lstm_o/biases"])
    assert np.array_equal(f["lstm_o"], fc)
    assert np.array_equal(f["heads"][..., :40], N.dense(fc, w["rpn_bbox_pred/weights"], w["rpn_bbox_pred/biases"]))
    assert np.array_equal(f["heads"][..., 40:], N.dense(fc, w["rpn_cls_score/weights"], w["rpn_cls_score/biases"]))
    # the saved gates are the recurrence's own: h = o tanh(c) reproduces lstm_out
    g = f["gates"]
    assert np.array_equal((torch.from_numpy(g[..., 3, :]) * torch.tanh(torch.from_numpy(g[..., 4, :]))).numpy().reshape(2, 2, 5, 256), lo)
    assert TR.TAIL_FLOATS == TG.TAIL_FLOATS == 818748 and [n for n, _, _ in TG.TAIL_MANIFEST] == TR.TAIL_NAMES


@pytest.mark.parametrize("kind", ["biased"])
def test_restatement_gradient_agrees_with_central_differences(kind):
    """Along a unit direction d, (L(p + e d) - L(p - e d)) / 2e with e = 1e-6 in float64: truncation ~ e^2 L''' and rounding ~ 2e-16 |L| / e, both
    far below 1e-5 of the slope; a wrong or missing term is an error of the slope's own size."""
    n, hf, wf = 1, 3, 4
    x, tail, g = K.features(n, hf, wf, kind, 2), K.tail_weights(kind), K.head_gradient(n, hf, wf, 2)
    ref = TR.gradients(x, tail, g, torch.float64)
    grad_tail = np.concatenate([ref["d_tail"][k].reshape(-1) for k in TR.TAIL_NAMES])
    g64 = torch.tensor(g[..., :60].astype(np.float64))

    def loss(xv, tv):
        with torch.no_grad():
            w = {k: torch.tensor(v) for k, v in TR.split_tail(tv).items()}
            return float((TR.forward(torch.tensor(xv), w)["heads"] * g64).sum())

    x64, t64 = x.astype(np.float64), tail.astype(np.float64)
    rng = np.random.default_rng(5)
    eps = 1e-6
    offs = np.cumsum([0] + [int(np.prod(s)) for s in TR.TAIL_SHAPES])
    for trial in range(14):
        d = np.zeros_like(t64)
        if trial < 10:      # one tensor at a time: a term missing from one tensor's gradient cannot hide behind the others
            d[offs[trial]: offs[trial + 1]] = rng.standard_normal(offs[trial + 1] - offs[trial])
        else:
            d = rng.standard_normal(t64.shape)
        d /= np.linalg.norm(d)
        slope = float(grad_tail @ d)
        fd = (loss(x64, t64 + eps * d) - loss(x64, t64 - eps * d)) / (2 * eps)
        assert abs(fd - slope) <= 1e-5 * max(abs(slope), 1e-3), (trial, fd, slope)
    for trial in range(3):
        d = rng.standard_normal(x64.shape)
        d /= np.linalg.norm(d)
        slope = float((ref["d_x"] * d).sum())
        fd = (loss(x64 + eps * d, t64) - loss(x64 - eps * d, t64)) / (2 * eps)
        assert abs(fd - slope) <= 1e-5 * max(abs(slope), 1e-3), (trial, fd, slope)


# ---- the per-thread text on the host
@pytest.fixture(scope="module")
def host_program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tail_grad_host") / "tail_grad_host")
    subprocess.run(GXX + ["-I", os.path.join(root, "text-detection-ctpn_amd", "csrc"), os.path.join(root, "tests", "tail_grad_host.cpp"), "-o", exe], check=True)
    return exe


def run_host(exe, tmp, rows, T, x, tail, d_lstm_out, mutant=0):
    w = TR.split_tail(tail)
    pre = N.lstm_pre(x.reshape(1, rows, T, 512), w).reshape(rows * T, 1024)
    wh = np.stack([w["lstm_o/bidirectional_rnn/%s/lstm_cell/kernel" % d][512:] for d in ("fw", "bw")])
    fin, fout = os.path.join(tmp, "in%d.bin" % mutant), os.path.join(tmp, "out%d.bin" % mutant)
    with open(fin, "wb") as f:
        f.write(struct.pack("ii", rows, T))
        for a in (x, pre, wh, d_lstm_out):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    p = subprocess.run([exe, fin, fout, str(mutant)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    raw = np.fromfile(fout, np.float32)
    M = rows * T
    sizes = [("gates", (M, 2, 5, 128)), ("lstm_out", (M, 256)), ("d_pre", (M, 1024)), ("d_wh", (2, 128, 512)), ("d_wx", (2, 512, 512)), ("d_b", (2, 512))]
    out, off = {}, 0
    for name, shape in sizes:
        k = int(np.prod(shape))
        out[name] = raw[off: off + k].reshape(shape)
        off += k
    assert off == raw.size
    return out


def host_errors(got, ref, rows, T):
    """{tensor: rel_error against the float64 autograd}"""
    e = {"gates": K.rel_error(got["gates"], ref["gates"].reshape(got["gates"].shape)), "lstm_out": K.rel_error(got["lstm_out"], ref["lstm_out"]),
         "d_pre": K.rel_error(got["d_pre"], ref["d_pre"])}
    for d, name in enumerate(("fw", "bw")):
        k = ref["d_tail"]["lstm_o/bidirectional_rnn/%s/lstm_cell/kernel" % name]
        e["d_wx_" + name] = K.rel_error(got["d_wx"][d], k[:512])
        e["d_wh_" + name] = K.rel_error(got["d_wh"][d], k[512:])
        e["d_b_" + name] = K.rel_error(got["d_b"][d], ref["d_tail"]["lstm_o/bidirectional_rnn/%s/lstm_cell/bias" % name])
    return e


def recurrence_case(rows, T, seed):
    x, tail = K.features(1, rows, T, "biased", seed), K.tail_weights("biased")
    d_lo = (np.random.default_rng([seed, 9]).standard_normal((rows * T, 256)) * 0.1).astype(np.float32)
    return x, tail, d_lo, TR.gradients(x, tail, None, torch.float64, d_lo), TR.gradients(x, tail, None, torch.float32, d_lo)


def test_host_program_equals_the_restatement(host_program, tmp_path):
    """17 rows x 20 steps = 340 cells: two partials in every reduction, the second one short. The program's fp32 chain against the float64
    autograd, allowed four times what the restatement's own float32 autograd loses on the same case (the rule of the device tests)."""
    rows, T = 17, 20
    x, tail, d_lo, ref64, ref32 = recurrence_case(rows, T, 3)
    got = run_host(host_program, str(tmp_path), rows, T, x, tail, d_lo)
    e = host_errors(got, ref64, rows, T)
    e32 = host_errors({"gates": ref32["gates"].reshape(rows * T, 2, 5, 128), "lstm_out": ref32["lstm_out"], "d_pre": ref32["d_pre"],
                       "d_wx": np.stack([ref32["d_tail"]["lstm_o/bidirectional_rnn/%s/lstm_cell/kernel" % n][:512] for n in ("fw", "bw")]),
                       "d_wh": np.stack([ref32["d_tail"]["lstm_o/bidirectional_rnn/%s/lstm_cell/kernel" % n][512:] for n in ("fw", "bw")]),
                       "d_b": np.stack([ref32["d_tail"]["lstm_o/bidirectional_rnn/%s/lstm_cell/bias" % n] for n in ("fw", "bw")])}, ref64, rows, T)
    print({k: (e[k], e32[k]) for k in e})
    for k in e:
        assert e[k] <= 4 * e32[k], (k, e[k], e32[k])


@pytest.mark.parametrize("mutant", [1, 2, 3, 4])
def test_mutants_of_the_cell_update_fail(host_program, tmp_path, mutant):
    """1 the f / o derivatives swapped, 2 the forget bias dropped, 3 c_t for c_{t-1}, 4 bw walked left to right: each is far outside the bound
    the unmutated program meets on the same small problem"""
    rows, T = 2, 3
    x, tail, d_lo, ref64, ref32 = recurrence_case(rows, T, 4)
    good = host_errors(run_host(host_program, str(tmp_path), rows, T, x, tail, d_lo), ref64, rows, T)
    bad = host_errors(run_host(host_program, str(tmp_path), rows, T, x, tail, d_lo, mutant), ref64, rows, T)
    assert max(good.values()) < 1e-5
    assert max(bad.values()) > 1e-2, bad


# ---- the fine-tune loop's condition, set on the CPU
def test_finetune_steps_halve_the_float64_loss(arena):
    img, gts = K.finetune_page()
    x = N.forward(img, ctpn_amd.arena_views(arena), keep={"rpn_conv/3x3"})["rpn_conv/3x3"]
    hf, wf = x.shape[1:3]
    gt5 = np.concatenate([gts[0], np.ones((len(gts[0]), 1), np.float32)], axis=1)
    t = R.anchor_targets(hf, wf, np.array([K.FT_H, K.FT_W, 1.0], np.float32), gt5, None, None, K.finetune_cfg(), 0)
    assert int((t["labels"] == 1).sum()) >= 4 and int((t["labels"] == 0).sum()) >= 4
    targets = [(t["labels"], t["bbox_targets"], t["inside_weights"], t["outside_weights"])]
    tail = arena[-TR.TAIL_FLOATS:].copy()
    vel = np.zeros_like(tail)
    losses = []
    for _ in range(K.FT_STEPS):
        ls, g = TR.loss_and_grad64(x, tail, targets)
        losses.append(ls[0])
        tail, vel, _ = TG.momentum_step(tail, vel, g.astype(np.float32), K.FT_LR, K.FT_MOMENTUM)
    losses.append(TR.loss_and_grad64(x, tail, targets)[0][0])
    assert losses[-1] < 0.5 * losses[0], losses


def test_momentum_step_is_the_reference_branch():
    """clip_by_global_norm(10.0), then accum = momentum accum + g, var -= lr accum"""
    g = np.array([30.0, -40.0], np.float32)                     # norm 50 -> scaled by 0.2
    w, v, norm = TG.momentum_step(np.array([1.0, 1.0], np.float32), np.array([1.0, 0.0], np.float32), g, 0.5, 0.9)
    assert norm == 50.0 and np.allclose(v, [0.9 + 6.0, -8.0]) and np.allclose(w, [1.0 - 0.5 * 6.9, 1.0 + 4.0])
    w, v, norm = TG.momentum_step(np.zeros(2, np.float32), np.zeros(2, np.float32), np.array([3.0, 4.0], np.float32), 1.0, 0.9)
    assert norm == 5.0 and np.array_equal(v, [3.0, 4.0]) and np.array_equal(w, [-3.0, -4.0])      # below the clip: untouched


# ---- the ABI without a device
def test_symbols_in_header_library_and_binding(root):
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    lib = B.load_library()
    declared = B._declare(C.CDLL(B.lib_path()))
    for name in NEW:
        assert name + "(" in hdr and hasattr(lib, name) and name in declared
    assert lib.ctpn_abi_version() == 10 and "#define CTPN_TAIL_FLOATS 818748" in hdr
    assert "ctpn_ctx" not in "".join(line for line in hdr.splitlines() if any(n + "(" in line for n in NEW))
    off = C.c_size_t()
    name = C.c_char_p()
    assert lib.ctpn_weight_manifest(lib.ctpn_weight_count() - 10, C.byref(name), None, None, C.byref(off)) == 0
    assert off.value == TG.TAIL_OFFSET == ctpn_amd.WEIGHT_FLOATS - 818748 and name.value.decode() == TR.TAIL_NAMES[0]


def test_tail_views_and_saved_layout():
    flat = np.arange(TG.TAIL_FLOATS, dtype=np.float32)
    v = TG.tail_views(flat)
    assert list(v) == TR.TAIL_NAMES and [v[k].shape for k in v] == TR.TAIL_SHAPES
    assert all(np.shares_memory(v[k], flat) for k in v) and v["rpn_cls_score/biases"][-1] == TG.TAIL_FLOATS - 1
    ref = TR.split_tail(flat)
    assert all(np.array_equal(v[k], ref[k]) for k in v)
    lib = B.load_library()
    assert lib.ctpn_tail_saved_floats(2, 3, 5) == 2 * 3 * 5 * 2048 and lib.ctpn_tail_saved_floats(0, 3, 5) == -1
    assert lib.ctpn_tail_saved_floats(1 << 10, 1 << 10, 3) == -1
    s = TG.saved_views(np.zeros(30 * 2048, np.float32), 2, 3, 5)
    assert s["lstm_out"].shape == (2, 3, 5, 256) and s["lstm_o"].shape == (2, 3, 5, 512) and s["gates"].shape == (2, 3, 5, 2, 5, 128)


def test_bad_arguments_and_no_device():
    lib = B.load_library()
    before = (C.c_longlong * 4)()
    lib.ctpn_debug_live_resources(before)
    M = 2 * 3
    x, tail, heads = np.zeros(M * 512, np.float32), np.zeros(TG.TAIL_FLOATS, np.float32), np.zeros(M * 64, np.float32)
    saved, d_tail = np.zeros(M * 2048, np.float32), np.zeros(TG.TAIL_FLOATS, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    fwd = lambda **k: lib.ctpn_tail_forward(k.get("dev", 0), k.get("n", 1), k.get("hf", 2), k.get("wf", 3), k.get("x", vp(x)), k.get("tail", vp(tail)),      # noqa: E731
                                            k.get("on", 0), k.get("heads", vp(heads)), k.get("saved", vp(saved)))
    bwd = lambda **k: lib.ctpn_tail_backward(k.get("dev", 0), k.get("n", 1), k.get("hf", 2), k.get("wf", 3), k.get("x", vp(x)), k.get("tail", vp(tail)),      # noqa: E731
                                             k.get("saved", vp(saved)), k.get("dh", vp(heads)), k.get("on", 0), k.get("d_tail", vp(d_tail)), k.get("d_x", None))
    for call in (fwd, bwd):
        assert call(n=0) == -1 and call(hf=0) == -1 and call(wf=-1) == -1
        assert call(n=1 << 10, hf=1 << 10, wf=3) == -1                     # beyond 2^21 cells
        assert call(x=None) == -1 and call(tail=None) == -1 and call(on=2) == -1
    assert fwd(heads=None) == -1
    assert bwd(saved=None) == -1 and bwd(dh=None) == -1 and bwd(d_tail=None) == -1
    # a device pointer off the 16-byte grid is refused before the device is looked for
    odd = C.c_void_p(x.ctypes.data + 4)
    assert fwd(on=1, x=odd) == -1 and b"16-byte" in lib.ctpn_last_error()
    assert bwd(on=1, dh=odd) == -1 and bwd(on=1, d_x=odd) == -1
    if lib.ctpn_device_count() <= 0:      # valid arguments reach the device check: an error, not a CPU fallback
        assert fwd() == -5 and bwd() == -5 and fwd(saved=None) == -5
        assert np.all(heads == 0) and np.all(d_tail == 0)
    after = (C.c_longlong * 4)()
    lib.ctpn_debug_live_resources(after)
    assert list(after) == list(before)
