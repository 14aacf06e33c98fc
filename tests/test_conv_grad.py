"""CPU: the backward pass through the conv stack (include/ctpn_hip.h, "the conv stack: backward") without a device.
  * tests/conv_grad_ref.py, the torch restatement with gradients, is held first: its float32 forward equals oracle.network's conv stack bit for
    bit, its float64 gradient agrees with central differences of the float64 loss along seeded random directions (float64 on the CPU only; no
    finite differences are taken on the device), and its pool gradient on tied integer data goes to the first maximum in scan order;
  * csrc/conv_grad_dev.h, the kernels' per-thread text, compiled with g++ under ASan + UBSan as a stand-alone program
    (tests/conv_grad_host.cpp) and run as a subprocess over whole small layers from exact-size heap blocks: on the exact cases of
    tests/conv_grad_cases.py its output equals the float64 restatement bit for bit; four mutants each fail that comparison;
  * the block plan for every layer of the network at 600 x 900 and 1280 x 1920, n in {1, 8, 32}, and for the small shapes;
  * the three symbols in header, library and binding; bad arguments refused before any device work; no device: CTPN_ERR_NODEVICE."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import conv_grad_cases as K
import conv_grad_ref as CR
import ctpn_amd
from ctpn_amd import _binding as B
from ctpn_amd import conv_grad as CG
from oracle import network as N
from util import stress_arena

GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all"]
NEW = ("ctpn_conv3x3_backward", "ctpn_maxpool2x2_backward", "ctpn_conv3x3_backward_plan")


# ---- the restatement
def test_restatement_forward_equals_the_oracle_bit_for_bit():
    arena = stress_arena("biased")
    views = ctpn_amd.arena_views(arena)
    img = ctpn_amd.weights.synthetic_images(2, 48, 80, 4)
    want = N.forward(img, views, keep=set(CR.CONVS) | set(CR.POOL_AFTER.values()))
    with torch.no_grad():
        w = {k: CR.t(v, torch.float32) for k, v in views.items() if k.startswith(("conv", "rpn_conv"))}
        got = CR.stack_forward(CR.t(N.image_blob(img), torch.float32), w)
    assert set(got) == set(CR.CONVS) | set(CR.POOL_AFTER.values())
    for name, v in got.items():
        assert np.array_equal(v.numpy(), want[name]), name
    assert CR.CONVS == N.CONVS == CG.CONVS and CR.POOL_AFTER == N.POOL_AFTER
    assert [tuple(views[c + "/weights"].shape[2:]) for c in CR.CONVS] == CR.CHANNELS
    # with gradients enabled the forward is the same bytes: what autograd differentiates is what the oracle computes
    with torch.enable_grad():
        wg = {k: CR.t(v, torch.float32, True) for k, v in views.items() if k.startswith(("conv", "rpn_conv"))}
        got_g = CR.stack_forward(CR.t(N.image_blob(img), torch.float32), wg)
    assert all(np.array_equal(v.detach().numpy(), want[k]) for k, v in got_g.items())


def test_restatement_gradient_agrees_with_central_differences():
    """Two layers with a pool between them, float64, small channel counts (the restatement has no shape limits). Along a unit direction d,
    (L(p + e d) - L(p - e d)) / 2e with e = 1e-6: truncation and rounding are far below 1e-5 of the slope unless a ReLU or a pool window
    changes its decision inside the step, which the test excludes (pre-activations and window gaps are checked to lie further than
    the step from a tie); a wrong or missing term is an error of the slope's own size."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 6, 5, 3))
    w1, b1 = rng.standard_normal((3, 3, 3, 4)) * 0.3, rng.standard_normal(4) * 0.1
    w2, b2 = rng.standard_normal((3, 3, 4, 5)) * 0.3, rng.standard_normal(5) * 0.1
    g = rng.standard_normal((2, 3, 2, 5))
    params = [x, w1, b1, w2, b2]

    def loss(ps, grad=False):
        ts = [torch.tensor(p, dtype=torch.float64, requires_grad=grad) for p in ps]
        z1 = CR.conv(ts[0], ts[1], ts[2])
        y1 = torch.relu(z1)
        z2 = CR.conv(CR.pool(y1), ts[3], ts[4])
        y2 = torch.relu(z2)
        return (y2 * torch.tensor(g)).sum(), ts, (y1, y2, z1, z2)

    with torch.enable_grad():
        L, ts, (y1, y2, z1, z2) = loss(params, True)
        L.backward()
    grads = [t.grad.numpy() for t in ts]
    # the layer-by-layer reference of the device tests gives the same gradients: mask as an input, pool by autograd
    d_w2, d_b2, d_p = CR.conv_backward(CR.pool(y1).detach().numpy(), w2, y2.detach().numpy(), g)
    d_y1 = CR.pool_backward(y1.detach().numpy(), d_p)
    d_w1, d_b1, d_x = CR.conv_backward(x, w1, y1.detach().numpy(), d_y1)
    for a, b in zip(grads, [d_x, d_w1, d_b1, d_w2, d_b2]):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-14)
    # no pre-activation within 1e-4 of its ReLU's corner, no window whose two largest values are positive and closer than that
    assert min(float(z.detach().abs().min()) for z in (z1, z2)) > 1e-4
    win = y1.detach().numpy()[:, :, :4].reshape(2, 3, 2, 2, 2, 4).transpose(0, 1, 3, 2, 4, 5).reshape(2, 3, 2, 4, 4)
    top = np.sort(win, axis=3)
    assert float((top[..., 3, :] - top[..., 2, :])[top[..., 2, :] > 0].min()) > 1e-4
    eps = 1e-6
    for trial in range(12):
        d = [np.zeros_like(p) for p in params]
        if trial < 5:
            d[trial] = rng.standard_normal(params[trial].shape)
        else:
            d = [rng.standard_normal(p.shape) for p in params]
        norm = np.sqrt(sum(float((v ** 2).sum()) for v in d))
        d = [v / norm for v in d]
        slope = sum(float((a * b).sum()) for a, b in zip(grads, d))
        with torch.no_grad():
            fd = (float(loss([p + eps * v for p, v in zip(params, d)])[0]) - float(loss([p - eps * v for p, v in zip(params, d)])[0])) / (2 * eps)
        assert abs(fd - slope) <= 1e-5 * max(abs(slope), 1e-3), (trial, fd, slope)


def test_restatement_pool_gradient_goes_to_the_first_maximum():
    """torch's rule on exact ties, which are real in ReLU data (a window of zeros): the gradient goes to the first maximum in (row, column) scan
    order, and nothing reaches the last row / column of an odd-sized map"""
    y = np.zeros((1, 5, 5, 2), np.float32)
    y[0, 0:2, 2:4, 0] = [[1, 3], [3, 3]]      # tie of three: (0, 3) comes first
    y[0, 2:4, 0:2, 1] = [[2, 0], [0, 2]]      # tie on the diagonal: (2, 0)
    d_pool = np.arange(1, 9, dtype=np.float32).reshape(1, 2, 2, 2)
    for dtype in (torch.float64, torch.float32):
        d = CR.pool_backward(y, d_pool, dtype)
        assert d[0, 0, 0, 0] == d_pool[0, 0, 0, 0] and d[0, 0, 0, 1] == d_pool[0, 0, 0, 1]      # all-zero windows: their first element
        assert d[0, 0, 3, 0] == d_pool[0, 0, 1, 0] and d[0, 1, 2, 0] == 0 and d[0, 1, 3, 0] == 0
        assert d[0, 2, 0, 1] == d_pool[0, 1, 0, 1] and d[0, 3, 1, 1] == 0
        assert not d[0, 4].any() and not d[0, :, 4].any() and float(d.sum()) == float(d_pool.sum())
    for shape in K.POOL_SHAPES:
        yy, dp, want = K.pool_exact_case(shape)
        n, h, w, c = shape
        mine = np.zeros((n, h, w, c))
        for i in range(h // 2):
            for j in range(w // 2):
                win = yy[:, 2 * i: 2 * i + 2, 2 * j: 2 * j + 2, :].reshape(n, 4, c)
                k = np.argmax(win, axis=1)      # numpy's argmax returns the first maximum
                for a in range(2):
                    for b in range(2):
                        mine[:, 2 * i + a, 2 * j + b, :] = np.where(k == 2 * a + b, dp[:, i, j, :], 0.0)
        assert np.array_equal(want, mine), shape


# ---- the per-thread text on the host
@pytest.fixture(scope="module")
def host_program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_grad_host") / "conv_grad_host")
    subprocess.run(GXX + ["-I", os.path.join(root, "text-detection-ctpn_amd", "csrc"), os.path.join(root, "tests", "conv_grad_host.cpp"), "-o", exe], check=True)
    return exe


def pool_input(shape):
    n, h, w, ci, co = shape
    return np.random.default_rng([5, n, h, w, co]).integers(1, 5, (n, h // 2, w // 2, co)).astype(np.float32)


def run_host(exe, tmp, shape, x, w, y, d_y, d_pool, mutant=0):
    n, h, wd, ci, co = shape
    fin, fout = os.path.join(tmp, "in%d.bin" % mutant), os.path.join(tmp, "out%d.bin" % mutant)
    with open(fin, "wb") as f:
        f.write(struct.pack("5i", *shape))
        for a in (x, w, y, d_y, d_pool):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    p = subprocess.run([exe, fin, fout, str(mutant)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert not p.stderr, p.stderr[-2000:]      # the sanitizers stay silent
    plan = np.fromfile(fout, np.int64, 2)
    raw = np.fromfile(fout, np.float32, offset=16)
    out, off = {"plan": (int(plan[0]), int(plan[1]))}, 0
    for name, shp in (("d_w", (3, 3, ci, co)), ("d_b", (co,)), ("d_x", (n, h, wd, ci)), ("d_full", (n, h, wd, co))):
        k = int(np.prod(shp))
        out[name] = raw[off: off + k].reshape(shp)
        off += k
    assert off == raw.size
    return out


def host_equals_reference(got, shape, x, w, y, d_y, d_pool, ref):
    """{tensor: equal to float64 bit for bit}"""
    return {"d_w": np.array_equal(got["d_w"].astype(np.float64), ref[0]), "d_b": np.array_equal(got["d_b"].astype(np.float64), ref[1]),
            "d_x": np.array_equal(got["d_x"].astype(np.float64), ref[2]),
            "d_full": np.array_equal(got["d_full"].astype(np.float64), CR.pool_backward(y, d_pool, torch.float64))}


@pytest.mark.parametrize("shape", K.ALL_SHAPES)
def test_host_program_equals_float64_on_the_exact_cases(host_program, tmp_path, shape):
    """y of the exact cases is small integers with many ties, so the pool backward over it meets the first-maximum rule on every window"""
    x, w, y, d_y, ref = K.exact_case(shape)
    d_pool = pool_input(shape)
    got = run_host(host_program, str(tmp_path), shape, x, w, y, d_y, d_pool)
    assert got["plan"] == ctpn_amd.conv_backward_plan(*shape)
    eq = host_equals_reference(got, shape, x, w, y, d_y, d_pool, ref)
    assert all(eq.values()), eq


@pytest.mark.parametrize("mutant,tensors", [(1, {"d_x"}), (2, {"d_x", "d_w"}), (3, {"d_x", "d_w", "d_b"}), (4, {"d_full"})])
def test_mutants_fail_the_comparison(host_program, tmp_path, mutant, tensors):
    """1 the data gradient's kernel not rotated, 2 taps crossing the image seam, 3 the mask y >= 0, 4 pool to the last maximum: each changes
    exactly the tensors it touches on the two-image case, which the unmutated program meets bit for bit"""
    shape = (2, 4, 6, 32, 128)
    x, w, y, d_y, ref = K.exact_case(shape)
    d_pool = pool_input(shape)
    good = host_equals_reference(run_host(host_program, str(tmp_path), shape, x, w, y, d_y, d_pool), shape, x, w, y, d_y, d_pool, ref)
    bad = host_equals_reference(run_host(host_program, str(tmp_path), shape, x, w, y, d_y, d_pool, mutant), shape, x, w, y, d_y, d_pool, ref)
    assert all(good.values()), good
    assert {k for k, v in bad.items() if not v} == tensors, bad


# ---- the plan
def plan_shapes():
    out = []
    for h, w in ((600, 900), (1280, 1920)):
        for n in (1, 8, 32):
            out += [s for _, s in CR.layer_shapes(n, h, w)]
    return out + K.ALL_SHAPES


def test_plan_covers_every_pixel_once_in_at_most_32_consecutive_blocks():
    lib = B.load_library()
    seen = set()
    for shape in plan_shapes():
        n, h, w, ci, co = shape
        block, blocks = ctpn_amd.conv_backward_plan(*shape)
        M = n * h * w
        assert 1 <= blocks <= 32 and block >= 1 and block % 64 == 0, shape
        # block p covers [p block, min((p + 1) block, M)): consecutive, every pixel once, no empty block
        assert (blocks - 1) * block < M <= blocks * block, shape
        assert ctpn_amd.conv_backward_plan(*shape) == (block, blocks)
        tiles = -(-ci // 16) * (co // 64)
        want = min(max(-(-1024 // tiles), 1), 32)      # the header's rule, restated
        assert block == -(-(-(-M // want)) // 64) * 64 and blocks == -(-M // block), shape
        seen.add(blocks)
    assert ctpn_amd.conv_backward_plan(1, 600, 900, 64, 64) == (16896, 32)          # conv1_2: 540 000 pixels, 36 864 outputs
    assert ctpn_amd.conv_backward_plan(1, 37, 56, 512, 512) == (576, 4)             # conv5_x: 2 072 pixels, 2 359 296 outputs
    assert {1, 2, 4, 32} <= seen
    for shape, (block, blocks, last) in K.PLAN_SHAPES.items():
        assert ctpn_amd.conv_backward_plan(*shape) == (block, blocks) and shape[0] * shape[1] * shape[2] - (blocks - 1) * block == last
    bp, nb = C.c_longlong(-7), C.c_int(-7)
    for bad in ((0, 2, 3, 32, 64), (1, 2, 3, 16, 64), (1, 2, 3, 32, 32), (1, 2, 3, 4096, 64), (1 << 10, 1 << 10, 1 << 10, 32, 64)):
        assert lib.ctpn_conv3x3_backward_plan(*bad, C.byref(bp), C.byref(nb)) == -1
    assert lib.ctpn_conv3x3_backward_plan(1, 2, 3, 32, 64, None, C.byref(nb)) == -1 and (bp.value, nb.value) == (-7, -7)
    if lib.ctpn_device_count() <= 0:      # reachable without a device
        assert ctpn_amd.conv_backward_plan(1, 2, 3, 32, 64) == (64, 1)


# ---- the ABI without a device
def test_symbols_in_header_library_and_binding(root):
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    lib = B.load_library()
    declared = B._declare(C.CDLL(B.lib_path()))
    for name in NEW:
        assert name + "(" in hdr and hasattr(lib, name) and name in declared
    assert lib.ctpn_abi_version() == 10
    assert "ctpn_ctx" not in "".join(line for line in hdr.splitlines() if any(n + "(" in line for n in NEW))
    for name in ("conv_backward", "pool_backward", "conv_backward_plan", "network_gradients"):
        assert name in ctpn_amd.__all__ and getattr(ctpn_amd, name) is getattr(CG, name)


def test_bad_arguments_and_no_device():
    lib = B.load_library()
    before = (C.c_longlong * 4)()
    lib.ctpn_debug_live_resources(before)
    M = 2 * 3
    x, w, y, g = np.zeros(M * 32, np.float32), np.zeros(9 * 32 * 64, np.float32), np.zeros(M * 64, np.float32), np.zeros(M * 64, np.float32)
    d_w, d_b, d_x = np.zeros(9 * 32 * 64, np.float32), np.zeros(64, np.float32), np.zeros(M * 32, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    conv = lambda **k: lib.ctpn_conv3x3_backward(k.get("dev", 0), k.get("n", 1), k.get("h", 2), k.get("w", 3), k.get("ci", 32), k.get("co", 64),      # noqa: E731
                                                 k.get("x", vp(x)), k.get("wt", vp(w)), k.get("y", vp(y)), k.get("g", vp(g)), k.get("on", 0),
                                                 k.get("d_w", vp(d_w)), k.get("d_b", vp(d_b)), k.get("d_x", vp(d_x)))
    pool = lambda **k: lib.ctpn_maxpool2x2_backward(k.get("dev", 0), k.get("n", 1), k.get("h", 2), k.get("w", 3), k.get("c", 64), k.get("y", vp(y)),      # noqa: E731
                                                    k.get("dp", vp(g)), k.get("on", 0), k.get("df", vp(y)))
    for call in (conv, pool):
        assert call(n=0) == -1 and call(h=0) == -1 and call(w=-1) == -1 and call(on=2) == -1 and call(on=-1) == -1
        assert call(n=1 << 10, h=1 << 10, w=1 << 10) == -1 and call(n=1 << 30, h=1 << 30, w=1 << 30) == -1      # a size overflow
        assert call(y=None) == -1
    for bad in (dict(ci=0), dict(ci=16), dict(ci=48), dict(ci=4), dict(co=0), dict(co=32), dict(co=96), dict(ci=4096), dict(ci=3)):
        assert conv(**bad) == -1, bad      # ci = 3 with a d_x: conv1_1's input has no gradient
    assert b"d_x is NULL" in lib.ctpn_last_error()
    for name in ("x", "wt", "g", "d_w", "d_b"):
        assert conv(**{name: None}) == -1, name
    assert pool(c=6) == -1 and pool(c=0) == -1 and pool(dp=None) == -1 and pool(df=None) == -1
    # a device pointer off the 16-byte grid is refused before the device is looked for
    odd = C.c_void_p(x.ctypes.data + 4)
    assert conv(on=1, x=odd) == -1 and b"16-byte" in lib.ctpn_last_error()
    assert conv(on=1, d_x=odd) == -1 and conv(on=1, d_b=odd) == -1 and pool(on=1, dp=odd) == -1 and pool(on=1, df=odd) == -1
    if lib.ctpn_device_count() <= 0:      # valid arguments reach the device check: an error, not a CPU fallback
        assert conv() == -5 and conv(d_x=None) == -5 and conv(ci=3, d_x=None) == -5 and pool() == -5
        assert pool(h=1, dp=None) == -5      # an empty pooled map is a valid call: d_pool may be NULL
        assert b"no CPU fallback" in lib.ctpn_last_error()
        assert not d_w.any() and not d_b.any() and not d_x.any()
        with pytest.raises(ctpn_amd.CtpnError) as e:
            ctpn_amd.conv_backward(x.reshape(1, 2, 3, 32), w.reshape(3, 3, 32, 64), y.reshape(1, 2, 3, 64), g.reshape(1, 2, 3, 64))
        assert e.value.code == -5
    with pytest.raises(ValueError):
        ctpn_amd.conv_backward(x.reshape(1, 2, 3, 32), w.reshape(3, 3, 32, 64), y.reshape(1, 3, 2, 64), g.reshape(1, 2, 3, 64))
    with pytest.raises(ValueError):
        ctpn_amd.pool_backward(y.reshape(1, 2, 3, 64), g.reshape(1, 2, 3, 64))
    after = (C.c_longlong * 4)()
    lib.ctpn_debug_live_resources(after)
    assert list(after) == list(before)
