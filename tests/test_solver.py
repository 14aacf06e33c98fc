"""CPU: the solver step (include/ctpn_hip.h) and ctpn_get_tensor_device's unpacking (include/ctpn_hip_train.h) without a device.
  * tests/solver_ref.py, the numpy restatement, is held first: against a float64 evaluation of the three formulas (same float32 constants,
    every operation exact to double) within a running first-order error bound built from the operations themselves, and against
    tail_grad.momentum_step bit for bit with decay 0;
  * csrc/solver_dev.h and csrc/unpack_dev.h, the kernels' per-element text, compiled with g++ -ffp-contract=off under ASan + UBSan as
    stand-alone programs (tests/solver_host.cpp, tests/unpack_host.cpp) and run over exact-size heap blocks: their output equals the
    restatements bit for bit, the sums included (the restatement adds in the plan's order); five mutants each fail that comparison;
  * the plan at its seams; the symbols in header, library and binding with the ABI still 10; the defaults; the decay table; bad arguments
    refused before any device work; the reference's TRAIN settings select Adam / 1e-5 / 5e-4."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ctpn_amd
import solver_ref as R
from ctpn_amd import _binding as B
from ctpn_amd import solver as S

GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all"]
NEW = ("ctpn_get_tensor_device", "ctpn_solver_plan", "ctpn_solver_defaults", "ctpn_solver_step")
U = 2.0 ** -24
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "text-detection-ctpn_amd", "csrc")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("solver_host")
    out = {}
    for name in ("solver_host", "unpack_host"):
        exe = str(d / name)
        subprocess.run(GXX + ["-I", CSRC, os.path.join(HERE, name + ".cpp"), "-o", exe], check=True)
        out[name] = exe
    return out


def case(count, seed, scale_g=1.0):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(count) * 0.05).astype(np.float32)
    g = (rng.standard_normal(count) * scale_g).astype(np.float32)
    s1 = np.abs(rng.standard_normal(count) * 0.1).astype(np.float32)
    s2 = np.abs(rng.standard_normal(count) * 0.1).astype(np.float32)
    return w, g, s1, s2


def segments(count, decay=0.0005):
    if count < 3:
        return np.array([count], np.int64), np.array([decay], np.float32)
    cuts = sorted(set([count // 3, count // 3 + 1, (2 * count) // 3, count]))
    return np.array(cuts, np.int64), np.array([decay if i % 2 == 0 else 0.0 for i in range(len(cuts))], np.float32)


# ---- the restatement
def running_bound(solver, p, w, g, s1, s2, d):
    """The float64 evaluation next to a first-order bound on what float32 adds, carried operation by operation: a result r computed from
    operands with absolute errors E has the propagated error of its formula plus U |r| for its own rounding (U = 2^-24; sqrt and / are
    correctly rounded; d(sqrt x) = dx / (2 sqrt x), d(a / b) = da / b + |a / b| db / b). -> (values, bounds) for w, s1, s2"""
    f = lambda v: np.asarray(v, np.float64)      # noqa: E731
    w, g, s1, d = f(w), f(g), f(s1), f(d)
    s2 = None if s2 is None else f(s2)
    c = {k: float(v) for k, v in p.items()}
    prod = d * w
    ge = g + prod
    e_ge = np.where(d == 0, 0.0, U * (np.abs(prod) + np.abs(ge)))
    if p["clip_on"]:
        gc = ge * c["scale"]
        e_gc = e_ge * c["scale"] + U * np.abs(gc)
    else:
        gc, e_gc = ge, e_ge
    if solver == R.MOMENTUM:
        m = c["a"] * s1
        n1 = m + gc
        e1 = U * np.abs(m) + e_gc + U * np.abs(n1)
        q = c["lr"] * n1
        nw = w - q
        return (nw, n1, None), (c["lr"] * e1 + U * np.abs(q) + U * np.abs(nw), e1, None)
    sq = gc * gc
    e_sq = 2 * np.abs(gc) * e_gc + U * sq
    if solver == R.ADAM:
        dl = gc - s1
        pr = dl * c["one_m_a"]
        n1 = s1 + pr
        e1 = c["one_m_a"] * (e_gc + U * np.abs(dl)) + U * np.abs(pr) + U * np.abs(n1)
        dl2 = sq - s2
        pr2 = dl2 * c["one_m_b"]
        n2 = s2 + pr2
        e2 = c["one_m_b"] * (e_sq + U * np.abs(dl2)) + U * np.abs(pr2) + U * np.abs(n2)
        num = n1 * c["lr_t"]
        e_num = c["lr_t"] * e1 + U * np.abs(num)
        r = np.sqrt(n2)
        e_r = e2 / (2 * r) + U * r
        den = r + c["eps"]
        e_den = e_r + U * den
        q = num / den
        e_q = e_num / den + np.abs(q) * e_den / den + U * np.abs(q)
        nw = w - q
        return (nw, n1, n2), (e_q + U * np.abs(nw), e1, e2)
    dl = sq - s1
    pr = dl * c["one_m_a"]
    n1 = s1 + pr
    e1 = c["one_m_a"] * (e_sq + U * np.abs(dl)) + U * np.abs(pr) + U * np.abs(n1)
    rad = n1 + c["eps"]
    e_rad = e1 + U * rad
    r = np.sqrt(rad)
    e_r = e_rad / (2 * r) + U * r
    num = gc * c["lr"]
    e_num = c["lr"] * e_gc + U * np.abs(num)
    q = num / r
    e_q = e_num / r + np.abs(q) * e_r / r + U * np.abs(q)
    m = s2 * c["a"]
    n2 = m + q
    e2 = U * np.abs(m) + e_q + U * np.abs(n2)
    nw = w - n2
    return (nw, n1, n2), (e2 + U * np.abs(nw), e1, e2)


@pytest.mark.parametrize("solver", [R.MOMENTUM, R.ADAM, R.RMS])
@pytest.mark.parametrize("clip", [10.0, 1e30])
def test_restatement_against_a_float64_evaluation(solver, clip):
    """|float32 - float64| <= 2 x the first-order running bound, elementwise. The factor 2 stands for the terms of second order the bound
    leaves out: each is a product of two relative errors of at most a few U, so together far below the first-order bound itself. The
    float64 evaluation is also held against the formulas written out directly, so that the bound's bookkeeping cannot hide a wrong formula."""
    count = 5000
    w, g, s1, s2 = case(count, 7 + solver)
    seg_end, seg_decay = segments(count)
    d = R.decay_per_element(count, seg_end, seg_decay)
    hyper = R.defaults(solver)
    hyper[4] = clip
    for t in (1, 4):
        sq, reg = R.sums(w, g, d)
        p = R.params(solver, hyper, t, sq)
        assert bool(p["clip_on"]) == (clip == 10.0)
        got = R.update(solver, p, w, g, s1, None if solver == R.MOMENTUM else s2, d)
        want, bound = running_bound(solver, p, w, g, s1, None if solver == R.MOMENTUM else s2, d)
        direct = R.update(solver, p, w, g, s1, None if solver == R.MOMENTUM else s2, d, dtype=np.float64)
        for k in range(3):
            if want[k] is None:
                assert got[k] is None
                continue
            assert got[k].dtype == np.float32 and np.array_equal(direct[k], want[k])
            err = np.abs(got[k].astype(np.float64) - want[k])
            assert (err <= 2 * bound[k]).all(), (solver, t, k, float((err / bound[k]).max()))
            assert err.max() > 0      # the float32 evaluation does round: the bound is not met by an accident of exact data
        # the sums against plain float64 sums: count 2^-53 relative, any order
        ge = R.grad_total(w, g, d).astype(np.float64)
        assert abs(sq - float(np.sum(ge * ge))) <= count * 2.0 ** -53 * sq
        assert abs(reg - float(np.sum(0.5 * d.astype(np.float64) * w.astype(np.float64) ** 2))) <= count * 2.0 ** -52 * reg
        # Adam's step size written out: lr sqrt(1 - b2^t) / (1 - b1^t)
        if solver == R.ADAM:
            assert p["lr_t"] == np.float32(1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))
            assert p["one_m_a"] == np.float32(1) - np.float32(0.9) and p["one_m_b"] == np.float32(1) - np.float32(0.999)


def test_restatement_equals_momentum_step_bit_for_bit():
    """decay 0. With the clip active the data are dyadic, so the norm is exact whichever way its sum is taken (numpy's pairwise sum there,
    the plan's order here); with random data the clip is out of reach and the norm does not enter"""
    count = 3000
    rng = np.random.default_rng(5)
    for clip, data in ((10.0, "dyadic"), (1e30, "random")):
        if data == "dyadic":
            w, g, v = [(rng.integers(-64, 65, count) / 64.0).astype(np.float32) for _ in range(3)]
        else:
            w, g, v = [rng.standard_normal(count).astype(np.float32) for _ in range(3)]
        hyper = R.defaults(R.MOMENTUM)
        hyper[0], hyper[1], hyper[4] = 0.01, 0.7, clip
        for t in (1, 2):
            nw, nv, _, (sq, reg) = R.step(R.MOMENTUM, w, g, v, None, [count], [0.0], hyper, t)
            mw, mv, norm = ctpn_amd.momentum_step(w, v, g, 0.01, 0.7, clip)
            assert nw.tobytes() == mw.tobytes() and nv.tobytes() == mv.tobytes() and reg == 0
            assert (norm > clip) == (clip == 10.0)
            if data == "dyadic" and t == 1:
                assert np.sqrt(sq) == norm
            w, v = nw, nv


# ---- the kernels' text on the host
def run_host(exe, solver, w, g, s1, s2, seg_end, seg_decay, hyper, t, tmp, mutant=0):
    count = w.shape[0]
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([solver, count, len(seg_end), t], np.int64).tobytes())
        f.write(np.asarray(hyper, np.float64).tobytes())
        f.write(np.asarray(seg_end, np.int64).tobytes())
        f.write(np.asarray(seg_decay, np.float32).tobytes())
        for a in (w, g, s1, s2):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, src, dst] + ([str(mutant)] if mutant else []), stderr=subprocess.PIPE)
    raw = open(dst, "rb").read()
    out2 = np.frombuffer(raw[:16], np.float64)
    if r.returncode == 3:
        return None, out2
    assert r.returncode == 0, r.stderr.decode()
    v = np.frombuffer(raw[16:], np.float32).reshape(3, count)
    return v, out2


HOST_COUNTS = [1, 3, 1023, 1024, 1025, 2 * 1024 + 5, 2048 * 1024 + 1029]


@pytest.mark.parametrize("solver", [R.MOMENTUM, R.ADAM, R.RMS])
def test_host_program_equals_the_restatement_bit_for_bit(programs, solver, tmp_path):
    hyper = R.defaults(solver)
    for count in HOST_COUNTS:
        w, g, s1, s2 = case(count, count, 1.0 if count < 100000 else 0.02)
        seg_end, seg_decay = segments(count)
        for t in ((1, 3) if count < 100000 else (2,)):
            got, out2 = run_host(programs["solver_host"], solver, w, g, s1, s2, seg_end, seg_decay, hyper, t, str(tmp_path))
            nw, n1, n2, ref2 = R.step(solver, w, g, s1, None if solver == R.MOMENTUM else s2, seg_end, seg_decay, hyper, t)
            assert (out2[0], out2[1]) == ref2, (count, t)
            assert got[0].tobytes() == nw.tobytes() and got[1].tobytes() == n1.tobytes(), (count, t)
            assert got[2].tobytes() == (s2 if n2 is None else n2).tobytes(), (count, t)
    # a NaN in the gradient: out2 says so and nothing else is written
    g = g.copy()
    g[-1] = np.nan
    got, out2 = run_host(programs["solver_host"], solver, w, g, s1, s2, seg_end, seg_decay, hyper, 1, str(tmp_path))
    assert got is None and not np.isfinite(out2[0])


@pytest.mark.parametrize("mutant,solver", [(1, R.MOMENTUM), (1, R.ADAM), (1, R.RMS), (2, R.ADAM), (3, R.RMS), (4, R.ADAM), (5, R.MOMENTUM), (5, R.ADAM)])
def test_mutants_fail_the_comparison(programs, mutant, solver, tmp_path):
    """1 decay added after the clip, 2 epsilon inside Adam's root, 3 ms started at zero, 4 bias correction dropped, 5 a segment boundary off
    by one: each changes the bytes the unmutated program shares with the restatement (the clip is active: |g| ~ 1 over 2053 elements)"""
    count = 2 * 1024 + 5
    hyper = R.defaults(solver)
    w, g, s1, s2 = case(count, 11)
    if mutant == 3:
        s1 = np.full(count, hyper[5], np.float32)      # the first step of a run: ms = 1
    seg_end, seg_decay = segments(count, 0.25)      # a decay large enough that an element given the wrong one moves by far more than rounding
    nw, n1, n2, ref2 = R.step(solver, w, g, s1, None if solver == R.MOMENTUM else s2, seg_end, seg_decay, hyper, 1)
    assert np.sqrt(ref2[0]) > hyper[4]
    good, _ = run_host(programs["solver_host"], solver, w, g, s1, s2, seg_end, seg_decay, hyper, 1, str(tmp_path))
    bad, _ = run_host(programs["solver_host"], solver, w, g, s1, s2, seg_end, seg_decay, hyper, 1, str(tmp_path), mutant)
    assert good[0].tobytes() == nw.tobytes() and bad[0].tobytes() != nw.tobytes()
    # ... and by more than rounding: beyond twice the running bound somewhere
    d = R.decay_per_element(count, seg_end, seg_decay)
    want, bound = running_bound(solver, R.params(solver, hyper, 1, ref2[0]), w, g, s1, None if solver == R.MOMENTUM else s2, d)
    assert any((np.abs(bad[k].astype(np.float64) - want[k]) > 2 * bound[k]).any() for k in range(3) if want[k] is not None)
    assert all((np.abs(good[k].astype(np.float64) - want[k]) <= 2 * bound[k]).all() for k in range(3) if want[k] is not None)


UNPACK_CASES = [      # n, H, W, C, ld, border, kind, gates
    (2, 3, 5, 64, 64, 1, R.F32, 0), (1, 4, 3, 128, 128, 1, R.BF16, 0), (2, 3, 2, 64, 64, 1, R.F16, 0), (1, 3, 4, 64, 128, 1, R.SPLIT, 0),
    (2, 2, 3, 512, 1536, 1, R.SPLIT, 0), (1, 2, 3, 1024, 1024, 0, R.F32, 1), (2, 1, 2, 1024, 1024, 0, R.F16, 1), (1, 3, 5, 60, 64, 0, R.F32, 0),
    (1, 1, 1, 20, 20, 0, R.F32, 0)]


@pytest.mark.parametrize("c", UNPACK_CASES)
def test_unpack_program_equals_get_tensors_host_loop(programs, c, tmp_path):
    n, H, W, C_, ld, border, kind, gates = c
    rng = np.random.default_rng(sum(c))
    stored = n * (H + 2 * border) * (W + 2 * border) * ld
    if kind == R.F32:
        src = rng.standard_normal(stored).astype(np.float32)
    else:
        src = rng.integers(0, 1 << 16, stored).astype(np.uint16)
        if kind == R.F16:
            src[:8] = [0x0001, 0x83ff, 0x0400, 0x7c00, 0xfc00, 0x7e00, 0x0000, 0x8000]      # subnormals, the smallest normal, infinities, a NaN, zeros
        else:
            src[(src & 0x7f80) == 0x7f80] = 0x3f80      # bf16 and the split pairs: finite, so that hi + lo has no NaN payload to agree on
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(a, "wb") as f:
        f.write(np.array(c, np.int32).tobytes())
        f.write(src.tobytes())
    r = subprocess.run([programs["unpack_host"], a, b], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    got = np.fromfile(b, np.float32).reshape(n, H, W, C_)
    want = R.unpack(src, n, H, W, C_, ld, border, kind, gates)
    assert want.shape == got.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert sorted(R.gate_col(ch) for ch in range(512)) == list(range(512))


# ---- the plan, the symbols, the settings
def test_the_plan_at_its_seams():
    seams = {1: (1024, 1), 1023: (1024, 1), 1024: (1024, 1), 1025: (1024, 2), 2048 * 1024: (1024, 2048), 2048 * 1024 + 1: (2048, 1025),
             2048 * 2048: (2048, 2048), 2048 * 2048 + 1: (3072, 1366), ctpn_amd.WEIGHT_FLOATS: (9216, 1942), ctpn_amd.TAIL_FLOATS: (1024, 800)}
    for count, want in seams.items():
        assert S.solver_plan(count) == want == R.plan(count), count
    rng = np.random.default_rng(0)
    for count in [int(v) for v in rng.integers(1, 1 << 34, 200)] + [1 << 40]:
        b, nb = S.solver_plan(count)
        assert (b, nb) == R.plan(count) and b % 1024 == 0 and 1 <= nb <= 2048 and (nb - 1) * b < count <= nb * b
    for bad in (0, -1, (1 << 40) + 1):
        with pytest.raises(ctpn_amd.CtpnError):
            S.solver_plan(bad)


def header_functions(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ctpn_[a-z_0-9]+)\s*\(", txt)))


def test_symbols_in_header_library_and_binding_and_the_abi_is_still_10(root):
    """the three solver calls are stateless and live in ctpn_hip.h; ctpn_get_tensor_device takes a ctx and lives in the training-side
    companion header, whose functions the binding declares in a table of their own: all of them, and nothing else"""
    lib = B.load_library()
    header = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    assert lib.ctpn_abi_version() == 10 and "#define CTPN_ABI_VERSION 10" in header
    main, train = header_functions(os.path.join(root, "include", "ctpn_hip.h")), header_functions(os.path.join(root, "include", "ctpn_hip_train.h"))
    assert train == ["ctpn_get_tensor_device"] and not set(train) & set(main) and set(NEW[1:]) <= set(main)
    raw = C.CDLL(B.lib_path())
    assert sorted(B._declare_train(raw)) == train and not set(train) & set(B._declare(raw))
    for name in NEW:
        assert hasattr(raw, name) and getattr(lib, name).argtypes is not None, name
    for k, v in (("MOMENTUM", 0), ("ADAM", 1), ("RMS", 2)):
        assert "#define CTPN_SOLVER_%s" % k in header and S.SOLVERS[{"MOMENTUM": "Momentum", "ADAM": "Adam", "RMS": "RMS"}[k]] == v
    assert all(hasattr(ctpn_amd, n) for n in ("solver_plan", "solver_defaults", "solver_step", "decay_table", "network_gradients_device", "Trainer"))
    assert hasattr(ctpn_amd.Context, "get_tensor_device")


def test_defaults_and_the_decay_table():
    for name, code in S.SOLVERS.items():
        assert np.array_equal(S.solver_defaults(name), R.defaults(code)) and np.array_equal(S.solver_defaults(code), R.defaults(code))
    assert S.solver_defaults("RMS")[5] == 1.0 and S.solver_defaults("Adam")[1:4].tolist() == [0.9, 0.999, 1e-8] and S.solver_defaults("Momentum")[4] == 10.0
    with pytest.raises(ValueError):
        S.solver_defaults("SGD")
    decayed = [n for n, _, _ in ctpn_amd.MANIFEST if S.decayed(n)]
    assert len(decayed) == 17 and decayed[-3:] == ["lstm_o/weights", "rpn_bbox_pred/weights", "rpn_cls_score/weights"]
    assert not any("lstm_cell" in n or n.endswith("biases") for n in decayed)
    for from_layer in ("conv1_1", "conv3_2", "rpn_conv/3x3"):
        first = S.trained_offset(from_layer)
        seg_end, seg_decay = S.decay_table(from_layer, 0.0005)
        d = R.decay_per_element(ctpn_amd.WEIGHT_FLOATS - first, seg_end, seg_decay)
        for name, shape, off in ctpn_amd.MANIFEST:
            if off >= first:
                want = np.float32(0.0005) if S.decayed(name) else 0
                assert d[off - first] == want and d[off - first + int(np.prod(shape)) - 1] == want, name
        assert len(seg_end) <= S.MAX_SEGMENTS and (np.diff(seg_decay) != 0).all()
    with pytest.raises(ValueError):
        S.trained_offset("conv9_9")


def test_bad_arguments_are_refused_before_any_device_work():
    lib = B.load_library()
    n = 8
    w, g, s1, s2 = (np.ones(n, np.float32) for _ in range(4))
    hyper = R.defaults(R.ADAM)
    end, dec, out2 = np.array([n], np.int64), np.zeros(1, np.float32), np.zeros(2)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def call(**k):
        h = k.get("hyper", hyper)
        e = k.get("end", end)
        return lib.ctpn_solver_step(k.get("dev", 0), k.get("solver", 1), k.get("count", n), k.get("w", vp(w)), vp(g), vp(s1), k.get("s2", vp(s2)),
                                    e.ctypes.data_as(C.POINTER(C.c_longlong)), dec.ctypes.data_as(C.POINTER(C.c_float)), k.get("n_seg", 1),
                                    h.ctypes.data_as(C.POINTER(C.c_double)), k.get("t", 1), k.get("on", 0), out2.ctypes.data_as(C.POINTER(C.c_double)))
    nan_h, zero_clip = hyper.copy(), hyper.copy()
    nan_h[0], zero_clip[4] = np.nan, 0.0
    for bad in (dict(solver=3), dict(count=0), dict(w=None), dict(s2=None), dict(n_seg=0), dict(n_seg=65), dict(t=0), dict(on=2), dict(hyper=nan_h),
                dict(hyper=zero_clip), dict(end=np.array([n - 1], np.int64)), dict(w=C.c_void_p(w.ctypes.data + 2))):
        assert call(**bad) == -1, bad
    assert (w == 1).all() and (s1 == 1).all() and (s2 == 1).all()
    if lib.ctpn_device_count() <= 0:
        assert call() == -5 and call(solver=0, s2=None) == -5 and (w == 1).all()
    with pytest.raises(ValueError):
        ctpn_amd.solver_step("Adam", w, g, s1, None, hyper, 1)
    with pytest.raises(ValueError):
        ctpn_amd.solver_step("Adam", w, g[:4], s1, s2, hyper, 1)
    with pytest.raises(ValueError):
        ctpn_amd.solver_step("Adam", w.astype(np.float64), g, s1, s2, hyper, 1)


def test_the_references_train_settings_select_adam(root):
    from ctpn_amd.ctpn import train_net as TN
    from ctpn_amd.lib.fast_rcnn.config import cfg, cfg_from_file
    saved = dict(cfg.TRAIN)
    try:
        cfg.TRAIN.update(dict(SOLVER="Momentum", LEARNING_RATE=0.001, WEIGHT_DECAY=0.0, STEPSIZE=50000, SNAPSHOT_ITERS=5000))      # whatever an earlier test left
        assert TN.solver_settings(cfg.TRAIN)[:3:2] == ("Momentum", 0.0)
        cfg_from_file(os.path.join(root, "tests", "golden", "train", "text_train.yml"))
        name, hyper, wd, stepsize, gamma, snap = TN.solver_settings(cfg.TRAIN)
        assert (name, hyper[0], wd, stepsize, gamma, snap) == ("Adam", 1e-5, 0.0005, 30000, 0.1, 1000)
        assert hyper[1:5].tolist() == [0.9, 0.999, 1e-8, 10.0]
        name, hyper, wd = TN.solver_settings(cfg.TRAIN, "RMS", 0.01, 0.0)[:3]
        assert (name, hyper[0], hyper[5], wd) == ("RMS", 0.01, 1.0, 0.0)
    finally:
        cfg.TRAIN.update(saved)
