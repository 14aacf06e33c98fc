"""GPU (-m gpu): the kernels behind the conv stack, each alone on caller data through its test hook -- lstm_pre_kernel / lstm_pre_small_kernel
(ctpn_debug_lstm_pre), the four BiLSTM kernels (ctpn_debug_bilstm), igemm_kernel as the plain GEMM of lstm_o, the heads and the fp32 / split
lstm_pre (ctpn_debug_gemm, ctpn_debug_lstm_pre). tests/tail_cells.py holds the cells, the recipes and the float64 references;
tests/test_tail_cells.py (CPU) keeps the table true and shows that a defective kernel would not pass what is asserted here.

lstm_pre, 16-bit modes: every cell of tests/tail_cell_cases.py (precision x form x waves per workgroup 1 .. 12 x tail class x idle waves), the
launch planned for 2 CUs, on the EXACT recipe -- integer operands, every sum exact in fp32 in any order, so the fp16 result must be
np.float16(float64 result) bit for bit, with a third of the outputs exact ties -- and on the NORMAL recipe within the project's per-mode bound
of the map's maximum. fp32 and split precision (the im2col GEMM) at M = 1, 31, 33, 4096, 4097. One problem under every launch shape, and an
image alone against its rows in the batch, compare bytes. The recurrence: the four reachable kernels x rows {1 .. 131} x T {1, 2, 5, 57} x
four recipes against the float64 cell; the 16-row and the 4-row split forms at the 128 / 129-row switch and row 0 alone compare bytes.
The GEMM: both tiles of Co <= 64 and the 128 x 128 tile, exact recipe bit for bit, pad columns and guard rows untouched (the hooks
themselves fail with CTPN_ERR_STATE when a guard row or pad column changes).

Every test prints one line per cell: TAIL <kernel> <cell> <shape> <measured> <bound>. Measured on an MI355X: profiles/tail_kernel_cells.txt
(830 lines). On the exact recipe no output of any lstm_pre cell or GEMM case differs by a bit. Worst on the other recipes, against the bound:
    lstm_pre fp16 3.20e-4 of 1.5e-3 and bf16 3.20e-4 of 8e-3 (both fp16 stores: one output rounding, 2^-12 of a value near the map's maximum);
    lstm_pre fp32 7.7e-7 of 5e-6, split 3.3e-6 of 2e-5 (the im2col GEMM);
    recurrence: exact 1.3e-6 of 5e-6, fast gates 1.0e-6 of 2e-5, split 16-row 7.3e-6 and 4-row 6.7e-6 of 3e-5 -- all on the saturated recipe at T = 57;
    GEMM fp32 1.1e-6 of 5e-6 (512 -> 60, M = 4096).
No bound needed the oracle-error allowance, and the new tests exposed no kernel defect."""
import functools

import numpy as np
import pytest

from ctpn_amd import _binding as B
import tail_cells as C
from tail_cell_cases import CASES

pytestmark = pytest.mark.gpu

PRE_CELLS = 800           # one problem per recipe and precision; a case takes its first n * hf * wf cells


def _bits16(a):
    """fp32 values that came out of an fp16 store -> their fp16 bits"""
    h = np.asarray(a, np.float32).astype(np.float16)
    assert np.array_equal(h.astype(np.float32), a)
    return h.view(np.uint16)


def _same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _judge(what, got, ref, tol):
    """whole map within tol of the map's max |value|, no element beyond 4 x tol"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    e = C.rel_err(got, ref)
    assert e < tol, (what, e, tol)
    assert not (np.abs(got - ref) > 4 * tol * float(np.abs(ref).max())).any(), what
    return e


def _run_pre(recipe, prec, case, cu, cells_total=PRE_CELLS):
    n, hf, wf = case
    m = n * hf * wf
    x, wx, bias, ref = C.pre_problem(recipe, prec, cells_total)
    got = B.debug_lstm_pre(x[:m].reshape(n, hf, wf, 512), wx, bias, prec, cu_count=cu).reshape(m, 1024)
    return got, ref[:m]


# ---------------------------------------------------------------------------------------------------------------
# lstm_pre
# ---------------------------------------------------------------------------------------------------------------
ALL_CELLS = sorted(CASES.items(), key=lambda kv: (kv[0].split("/")[0], kv[1][0] * kv[1][1] * kv[1][2], kv[0]))


@pytest.mark.parametrize("cell,case", ALL_CELLS, ids=[c.replace("/", ".") for c, _ in ALL_CELLS])
def test_lstm_pre_cell_is_exact_and_within_the_bound(cell, case):
    prec = cell.split("/")[0]
    m = case[0] * case[1] * case[2]
    assert C.cell_name(prec, B.lstm_pre_plan(m, C.CU), m) == cell          # the plan the launch below follows
    got, ref = _run_pre("exact", prec, case, C.CU)
    want = ref.astype(np.float16)
    wrong = _bits16(got) != want.view(np.uint16)
    a = np.abs(ref)
    ties = float(((a > 2048) & (a < 4096) & (a % 2 == 1)).mean())
    assert not wrong.any(), (cell, int(wrong.sum()), np.argwhere(wrong)[:4].tolist(), got[wrong][:4], ref[wrong][:4])
    again, _ = _run_pre("exact", prec, case, C.CU)
    assert _same_bytes(got, again), cell
    normal, nref = _run_pre("normal", prec, case, C.CU)
    e = _judge(cell, normal, nref, C.BOUND[prec])
    print("TAIL lstm_pre %-28s %-10s exact: 0 of %d differ (%.0f %% ties)  normal: %.3e of %.1e" % (cell, "x".join(map(str, case)), got.size, 100 * ties, e, C.BOUND[prec]))


@pytest.mark.parametrize("prec", ["fp32", "split"])
@pytest.mark.parametrize("case", C.IGEMM_PRE_SHAPES, ids=["M%d" % (n * h * w) for n, h, w in C.IGEMM_PRE_SHAPES])
def test_lstm_pre_of_fp32_and_split_precision(prec, case):
    got, ref = _run_pre("exact", prec, case, 0, 4097)
    wrong = got.astype(np.float64) != ref                                  # integers below 2^24: the float64 result itself; split: lo = 0
    assert not wrong.any(), (prec, case, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    normal, nref = _run_pre("normal", prec, case, 0, 4097)
    e = _judge((prec, case), normal, nref, C.BOUND[prec])
    again, _ = _run_pre("normal", prec, case, 0, 4097)
    assert _same_bytes(normal, again)
    print("TAIL lstm_pre %-28s %-10s exact: 0 of %d differ  normal: %.3e of %.1e" % (prec + "/igemm", "x".join(map(str, case)), got.size, e, C.BOUND[prec]))


# 23 groups with 17 cells in the last: cu_count -> W = 12, 8, 6, 5, 4, 3, 2, 1 and, from 46 CUs, the small form; ceil(23 / cu) is never 7, 9,
# 10 or 11, so four more problems (21, 27, 20, 22 groups, the same tail) reach those W, each against its own W = 1 and small-form results
INVARIANCE = (((1, 7, 103), (2, 3, 4, 5, 6, 8, 12, 16, 24, 46, 1000)), ((1, 9, 73), (3, 21, 1000)), ((3, 1, 283), (3, 27, 1000)),
              ((5, 5, 25), (2, 20, 1000)), ((1, 13, 53), (2, 22, 1000)))


@pytest.mark.parametrize("prec", C.PRECS16)
def test_lstm_pre_is_the_same_bytes_under_every_launch_shape(prec):
    shapes = set()
    for case, cus in INVARIANCE:
        m = case[0] * case[1] * case[2]
        assert m % 32 == 17
        first = None
        for cu in cus:
            plan = B.lstm_pre_plan(m, cu)
            shapes.add((plan.form, plan.waves))
            got, ref = _run_pre("normal", prec, case, cu, 849)
            if first is None:
                first = got
                e = _judge((prec, case), got, ref, C.BOUND[prec])
            assert _same_bytes(got, first), (prec, case, cu, plan, int((got != first).sum()))
        print("TAIL lstm_pre %-28s %-10s cu_count %s: one result, %.3e of %.1e" % (prec + "/launch shapes", "x".join(map(str, case)), list(cus), e, C.BOUND[prec]))
    assert shapes == {("small", 1)} | {("lds", w) for w in range(1, 13)}, sorted(shapes)


@pytest.mark.parametrize("prec", C.PRECS16)
@pytest.mark.parametrize("cu", [2, 0], ids=["cu2", "device"])
def test_lstm_pre_image_alone_equals_its_rows_in_the_batch(prec, cu):
    x, wx, bias, ref = C.pre_problem("normal", prec, PRE_CELLS)
    n, hf, wf = 3, 5, 37
    per = hf * wf
    batch = B.debug_lstm_pre(x[:n * per].reshape(n, hf, wf, 512), wx, bias, prec, cu_count=cu)
    alone = B.debug_lstm_pre(x[per:2 * per].reshape(1, hf, wf, 512), wx, bias, prec, cu_count=cu)
    assert B.lstm_pre_plan(n * per, cu) != B.lstm_pre_plan(per, cu) or cu == 0
    _judge((prec, "batch"), batch.reshape(-1, 1024), ref[:n * per], C.BOUND[prec])
    assert _same_bytes(batch[1:2], alone), (prec, cu)
    print("TAIL lstm_pre %-28s 3x5x37     image 1 alone %s == in the batch %s" % (prec + "/batch", B.lstm_pre_plan(per, cu)[:2], B.lstm_pre_plan(n * per, cu)[:2]))


# ---------------------------------------------------------------------------------------------------------------
# the recurrence
# ---------------------------------------------------------------------------------------------------------------
# the template pairs the forward launches: name -> (split, fast_gates, pre_f16)
REC_KERNELS = {"exact.f32": (False, False, False), "fast.f16": (False, True, True), "split.f32": (True, False, False), "split.f16": (True, True, True)}
REC_ROWS = (1, 3, 4, 5, 16, 17, 128, 129, 131)
REC_T = (1, 2, 5, 57)


def _form(kern, rows):
    split, fast, _ = REC_KERNELS[kern]
    return ("split_few" if rows <= 128 else "split_16") if split else ("exact_fast_gates" if fast else "exact")


def _run_rec(kern, recipe, rows, T):
    split, fast, f16 = REC_KERNELS[kern]
    pre, wh = C.rec_problem(recipe, rows, T, f16)
    out, form = B.debug_bilstm(pre, wh, split=split, fast_gates=fast, pre_f16=f16)
    return out, form, pre, wh


def test_recurrence_cases_reach_every_form():
    assert {_form(k, r) for k in REC_KERNELS for r in REC_ROWS} == set(B.BILSTM_FORMS)


@pytest.mark.parametrize("T", REC_T)
@pytest.mark.parametrize("rows", REC_ROWS)
@pytest.mark.parametrize("kern", list(REC_KERNELS))
def test_recurrence_matches_the_float64_cell(kern, rows, T):
    for recipe in C.REC_RECIPES:
        out, form, pre, wh = _run_rec(kern, recipe, rows, T)
        assert form == _form(kern, rows), (kern, rows, form)
        assert np.isfinite(out).all() and np.abs(out).max() <= 1.0
        err = float(np.abs(out - C.bilstm_ref(pre, wh)).max())
        print("TAIL bilstm   %-28s %-10s %-10s %.3e of %.1e" % (kern + "/" + form, "%dx%d" % (rows, T), recipe, err, C.REC_TOL[form]))
        assert err < C.REC_TOL[form], (kern, form, rows, T, recipe, err)


@pytest.mark.parametrize("recipe", ["normal", "saturated"])
@pytest.mark.parametrize("kern", ["split.f32", "split.f16"])
def test_split_forms_agree_at_the_row_switch(kern, recipe):
    """rows 0 .. 127 of a 129-row call (16 rows per workgroup) against the same rows as a 128-row call (4 rows per workgroup): bytes"""
    split, fast, f16 = REC_KERNELS[kern]
    pre, wh = C.rec_problem(recipe, 129, 57, f16)
    big, form_big = B.debug_bilstm(pre, wh, split=split, fast_gates=fast, pre_f16=f16)
    few, form_few = B.debug_bilstm(pre[:128], wh, split=split, fast_gates=fast, pre_f16=f16)
    assert (form_big, form_few) == ("split_16", "split_few")
    assert _same_bytes(big[:128], few), (kern, recipe, int((big[:128] != few).sum()))
    again, _ = B.debug_bilstm(pre, wh, split=split, fast_gates=fast, pre_f16=f16)
    assert _same_bytes(big, again)
    print("TAIL bilstm   %-28s 129x57     %-10s rows 0 .. 127: split_16 == split_few" % (kern + "/switch", recipe))


@pytest.mark.parametrize("rows", [17, 131])
@pytest.mark.parametrize("kern", list(REC_KERNELS))
def test_row_0_alone_equals_row_0_of_the_call(kern, rows):
    split, fast, f16 = REC_KERNELS[kern]
    pre, wh = C.rec_problem("normal", rows, 57, f16)
    full, form = B.debug_bilstm(pre, wh, split=split, fast_gates=fast, pre_f16=f16)
    alone, form1 = B.debug_bilstm(pre[:1], wh, split=split, fast_gates=fast, pre_f16=f16)
    assert _same_bytes(full[:1], alone), (kern, rows, form, form1)
    print("TAIL bilstm   %-28s %-10s row 0 of %s == alone (%s)" % (kern + "/row0", "%dx57" % rows, form, form1))


# ---------------------------------------------------------------------------------------------------------------
# the plain GEMM: lstm_o (256 -> 512), the folded heads (256 -> 60 in rows of 64), the heads (512 -> 60)
# ---------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = ((256, 60, 64), (256, 512, 512), (512, 60, 64))
GEMM_M = (1, 63, 64, 65, 255, 257, 4096, 4097)
FILL = np.frombuffer(bytes([0xC3] * 4), np.uint32)[0]


def _run_gemm(recipe, M, K, Co, ldc):
    a, w, bias, ref = C.gemm_problem(recipe, max(GEMM_M), K, Co)
    out = B.debug_gemm(a[:M], w, bias, ldc=ldc)
    assert out.shape == (M, ldc)
    assert (out[:, Co:].view(np.uint32) == FILL).all(), "pad columns %d .. %d were written" % (Co, ldc - 1)
    return out[:, :Co], ref[:M]


@pytest.mark.parametrize("M", GEMM_M)
@pytest.mark.parametrize("K,Co,ldc", GEMM_SHAPES, ids=["%dx%d" % s[:2] for s in GEMM_SHAPES])
def test_gemm_is_exact_and_within_the_bound(K, Co, ldc, M):
    got, ref = _run_gemm("exact", M, K, Co, ldc)
    wrong = got.astype(np.float64) != ref
    assert not wrong.any(), (M, K, Co, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    normal, nref = _run_gemm("normal", M, K, Co, ldc)
    e = _judge((M, K, Co), normal, nref, C.BOUND["fp32"])
    print("TAIL igemm    %-28s %-10s exact: 0 of %d differ  normal: %.3e of %.1e" % ("fp32/%dx%d/ldc%d" % (K, Co, ldc), "M%d" % M, got.size, e, C.BOUND["fp32"]))


@pytest.mark.parametrize("K,Co,ldc", [s for s in GEMM_SHAPES if s[1] <= 64], ids=["%dx%d" % s[:2] for s in GEMM_SHAPES if s[1] <= 64])
def test_both_gemm_tiles_give_one_rows_bits(K, Co, ldc):
    """M = 4096 runs the 64 x 64 tile, M = 4097 the 256 x 64 tile (csrc/igemm.hip launch_typed): rows 0 .. 4095 are the same K-ordered sums"""
    small, _ = _run_gemm("normal", 4096, K, Co, ldc)
    tall, _ = _run_gemm("normal", 4097, K, Co, ldc)
    assert _same_bytes(tall[:4096], small), (K, Co, int((tall[:4096] != small).sum()))
    print("TAIL igemm    %-28s M4096/4097 rows 0 .. 4095: 256 x 64 tile == 64 x 64 tile" % ("fp32/%dx%d/tiles" % (K, Co)))
