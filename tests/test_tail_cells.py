"""CPU: the cells of lstm_pre's launch shapes (tests/tail_cells.py) through the library's plan function, against the committed table
(tests/tail_cell_cases.py) that tests/test_gpu_tail_kernels.py runs on the device; the plan against the launcher's formula as it stood before
the plan became a function; and MUTANTS: numpy models of the kernels with one defect each, which the device tests' checks must catch.

What a mutant has to do is fixed by what the defect is:
  * a wrong ROUNDING of the fp16 store moves an output by one fp16 step at most, which no tolerance sees: it must break bit-equality with
    np.float16(float64 result) on at least 1 % of the outputs of the exact recipe. The bias added AFTER the conversion is of this kind (the
    sum and the bias each rounded to fp16, then added in fp16): on the normal recipe it stays at 0.35 x the fp16 bound, on the exact recipe
    19 % of the outputs differ;
  * every other defect must exceed the project's bound on the normal recipe by at least 10 x (lstm_pre: the fp16 mode's bound, the tighter of
    the two 16-bit ones -- a mis-ordered bias of size 0.1 is 0.03 of the map's maximum, below 10 x the bf16 bound of 8e-3 and 21 x the fp16 one)."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import tail_cells as C
from tail_cell_cases import CASES


@pytest.fixture(scope="module")
def reachable():
    return C.census()


def test_plan_entry_point_and_argument_errors():
    assert B.lstm_pre_plan(32, 2) == ("small", 1, 8, 0)
    assert B.lstm_pre_plan(33, 2) == ("lds", 1, 2, 0)
    assert B.lstm_pre_plan(65, 2) == ("lds", 2, 2, 1)
    assert B.lstm_pre_plan(25 * 32, 2) == ("lds", 12, 3, 11)
    # the benchmark's batch on 256 CUs: 2072 wave-groups are 231 workgroups of 9 waves (csrc/lstm_pre.hip); one image: 65 groups x 8 one-wave workgroups
    assert B.lstm_pre_plan(32 * 37 * 56, 256) == ("lds", 9, 231, 7)
    assert B.lstm_pre_plan(37 * 56, 256) == ("small", 1, 520, 0)
    for cells, cu in ((0, 2), (-5, 2), (1 << 31, 2), (100, -1)):
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.lstm_pre_plan(cells, cu)
        assert e.value.code == -1, (cells, cu)
    if B.device_count() == 0:       # cu_count 0 asks a device
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.lstm_pre_plan(100)
        assert e.value.code == -5


def test_every_cell_has_a_case_and_every_case_is_its_cell(reachable):
    assert reachable == CASES
    assert len(CASES) == 192                  # 2 precisions x (small: 4 tails; W = 1: 4 tails; W = 2 .. 12: 4 tails x idle 0 / 1)
    for cell, case in CASES.items():
        assert C.case_cell(cell.split("/")[0], case) == cell, (cell, case)
        n, hf, wf = case
        assert n * hf * wf <= C.MAX_CELLS and n > 1 and hf > 1, (cell, case)      # every cell is reached by a map whose strides matter
    for prec in C.PRECS16:
        mine = [c.split("/")[1:] for c in CASES if c.startswith(prec + "/")]
        assert {(f, w) for f, w, _t, _i in mine} == {("small", "w1")} | {("lds", "w%d" % w) for w in range(1, 13)}
        for w in range(2, 13):
            assert {(t, i) for f, ww, t, i in mine if ww == "w%d" % w} == {(t, i) for t in C.TAILS for i in ("idle0", "idle1")}, w
        assert {(t, i) for f, ww, t, i in mine if f == "small"} == {(t, "idle0") for t in C.TAILS}


def _formula(cells, ncu):
    """launch_lstm_pre's arithmetic as it stood before lstm_pre_plan: (small, waves, workgroups, idle waves), vectorised over cells"""
    groups = (cells + 31) // 32
    W = np.clip((groups + ncu - 1) // ncu, 1, 12)
    cellblks = (groups + W - 1) // W
    small = cellblks * 2 <= ncu
    return np.where(small, 0, 1), np.where(small, 1, W), np.where(small, groups * 8, cellblks), np.where(small, 0, cellblks * W - groups)


@pytest.mark.parametrize("ncu", [2, 64, 104, 228, 256, 304])
def test_plan_is_the_launchers_formula(ncu):
    import ctypes
    lib = B.load_library()
    cells = np.arange(1, 100001)
    want = np.stack(_formula(cells, ncu), axis=1)
    got = np.zeros((len(cells), 4), np.int32)
    p = got.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    for i, m in enumerate(cells):
        assert lib.ctpn_debug_lstm_pre_plan(int(m), ncu, ctypes.cast(ctypes.addressof(p.contents) + 16 * i, ctypes.POINTER(ctypes.c_int))) == 0
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, (ncu, cells[bad[:4, 0]].tolist(), got[bad[0, 0]].tolist(), want[bad[0, 0]].tolist())
    assert set(np.unique(got[:, 1])) <= set(range(1, 13))


def test_bilstm_hook_reports_the_form_and_refuses_the_pairs_the_forward_never_launches():
    pre, wh = C.rec_problem("normal", 1, 1, False)
    for kw in (dict(fast_gates=False, pre_f16=True), dict(fast_gates=True, pre_f16=False)):
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.debug_bilstm(pre, wh, split=False, **kw)
        assert e.value.code == -1, kw
    if B.device_count() == 0:       # the launch itself needs a device
        for fn in (lambda: B.debug_bilstm(pre, wh), lambda: B.debug_gemm(np.zeros((1, 32)), np.zeros((32, 4)), np.zeros(4)),
                   lambda: B.debug_lstm_pre(np.zeros((1, 1, 1, 512)), np.zeros((512, 1024)), np.zeros(1024), cu_count=2)):
            with pytest.raises(ctpn_amd.CtpnError) as e:
                fn()
            assert e.value.code == -5
    for kw in (dict(a=np.zeros((1, 48)), w=np.zeros((48, 4)), bias=np.zeros(4)), dict(a=np.zeros((1, 32)), w=np.zeros((32, 6)), bias=np.zeros(6)),
               dict(a=np.zeros((1, 32)), w=np.zeros((32, 8)), bias=np.zeros(8), ldc=4), dict(a=np.zeros((1, 32)), w=np.zeros((32, 8)), bias=np.zeros(8), precision="split")):
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.debug_gemm(**kw)
        assert e.value.code == -1, kw


def test_gate_permutation_is_a_permutation_of_64_byte_runs():
    perm = C.gate_perm()
    assert sorted(perm.tolist()) == list(range(1024))
    for d in (0, 512):              # a lane's 4 gates x 4 units are 16 consecutive device columns: units 4 k .. 4 k + 3 of i, j, f, o
        for k in range(32):
            cols = [perm[d + g * 128 + 4 * k + e] for g in range(4) for e in range(4)]
            assert cols == list(range(d + 16 * k, d + 16 * k + 16)), (d, k)
    assert not np.array_equal(C.gate_perm(swap_f_j=True), perm)


# ---------------------------------------------------------------------------------------------------------------
# the recipes do what they are for
# ---------------------------------------------------------------------------------------------------------------
def test_exact_recipe_is_exact_in_any_order_and_full_of_ties():
    x, wx, bias, ref = C.pre_problem("exact", "fp16", 800)
    assert (np.abs(x).astype(np.float64) @ np.abs(wx).astype(np.float64) + np.abs(bias)).max() < 2 ** 24
    assert np.array_equal(ref, np.rint(ref)) and np.abs(x).max() <= 6 and np.abs(wx).max() <= 6 and np.abs(bias).max() <= 3000
    for prec in ("bf16", "fp16", "split"):
        assert np.array_equal(C.operand(prec, x), x) and np.array_equal(C.operand(prec, wx), wx)      # no operand rounding; split: lo = 0
    a = np.abs(ref)
    ties = (a > 2048) & (a < 4096) & (a % 2 == 1)
    assert ties.mean() >= 0.01 and (a > 2048).mean() >= 0.20, (ties.mean(), (a > 2048).mean())
    # an fp32 accumulation in another order gives the same bits
    shuffled = np.random.default_rng(0).permutation(512)
    acc = np.tile(bias, (16, 1))
    for k in shuffled:
        acc = (acc + x[:16, k:k + 1] * wx[k:k + 1, :]).astype(np.float32)
    assert np.array_equal(acc.astype(np.float64), ref[:16])
    # the model of the correct kernel IS the expectation, bit for bit
    assert np.array_equal(C.lstm_pre_model(x, wx, bias), ref.astype(np.float16).astype(np.float64))


def test_recurrence_recipes():
    pre, wh = C.rec_problem("growth", 3, 57, False)
    out = C.bilstm_ref(pre, wh)
    neg = C.bilstm_ref(*C.rec_problem("growth_neg", 3, 57, False))
    assert np.abs(out).max() <= 1 and np.abs(neg).max() <= 1
    assert (np.sign(out[:, 5:, :128]) == 1).all() and (np.sign(neg[:, 5:, :128]) == -1).all()      # c_t = +-t, so h = +-sigmoid(o)
    sat = C.rec_problem("saturated", 3, 5, True)[0]
    assert np.abs(sat).max() == 100.0 and np.array_equal(sat, sat.astype(np.float16).astype(np.float32))
    # the float64 cell restates oracle/network.py::bilstm_from_pre (fp32 torch)
    from oracle import network as N
    pre, wh = C.rec_problem("normal", 5, 7, False)
    w = {"lstm_o/bidirectional_rnn/%s/lstm_cell/kernel" % nm: np.concatenate([np.zeros((512, 512), np.float32), wh[d]]) for d, nm in enumerate(("fw", "bw"))}
    want = N.bilstm_from_pre(pre.reshape(1, 5, 7, 1024).copy(), w).reshape(5, 7, 256)
    assert np.abs(C.bilstm_ref(pre, wh) - want).max() < 2e-6


# ---------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["f16_trunc", "f16_ties_away", "bias_after_cvt"])
def test_rounding_mutants_break_bit_equality_on_the_exact_recipe(defect):
    x, wx, bias, ref = C.pre_problem("exact", "fp16", 800)
    want = ref.astype(np.float16)
    got = C.lstm_pre_model(x, wx, bias, defect).astype(np.float16)
    differ = float((got.view(np.uint16) != want.view(np.uint16)).mean())
    print("%s: %.1f %% of the exact outputs differ" % (defect, 100 * differ))
    assert differ >= 0.01
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 4.0      # ... by one fp16 step (2 below 4096, 4 above): what no tolerance sees
    xn, wn, bn, rn = C.pre_problem("normal", "fp16", 800)
    assert C.rel_err(C.lstm_pre_model(xn, wn, bn, defect), rn) < C.BOUND["fp16"]      # and the normal recipe's bound does not


@pytest.mark.parametrize("defect", ["bias_tf_order", "swap_f_j", "stale_kslice"])
def test_lstm_pre_mutants_exceed_the_normal_bound_tenfold(defect):
    x, wx, bias, ref = C.pre_problem("normal", "fp16", 800)
    assert C.rel_err(C.lstm_pre_model(x, wx, bias), ref) < C.BOUND["fp16"]
    e = C.rel_err(C.lstm_pre_model(x, wx, bias, defect), ref)
    print("%s: %.2e = %.0f x the fp16 bound" % (defect, e, e / C.BOUND["fp16"]))
    assert e >= 10 * C.BOUND["fp16"]


@pytest.mark.parametrize("defect", ["no_forget_bias", "bw_not_reversed", "h_two_back"])
def test_recurrence_mutants_exceed_the_bound_tenfold(defect):
    pre, wh = C.rec_problem("normal", 5, 5, False)
    e = float(np.abs(C.bilstm_ref(pre, wh, defect) - C.bilstm_ref(pre, wh)).max())
    print("%s: %.2e = %.0f x the loosest recurrence bound" % (defect, e, e / max(C.REC_TOL.values())))
    assert e >= 10 * max(C.REC_TOL.values())


def test_gemm_mutant_exceeds_the_bound_tenfold():
    for K, Co in ((256, 60), (256, 512), (512, 60)):
        a, w, bias, ref = C.gemm_problem("normal", 65, K, Co)
        assert C.rel_err(C.gemm_model(a, w, bias), ref) == 0
        e = C.rel_err(C.gemm_model(a, w, bias, "drop_last_k"), ref)
        assert e >= 10 * C.BOUND["fp32"], (K, Co, e)
