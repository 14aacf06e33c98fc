"""The conv3x3 kernel forms the network can reach, enumerated through the library's own plan function (ctpn_debug_conv3x3_plan: the struct
launch_conv3x3 computes and follows, csrc/conv3x3_plan.h) -- no device needed, the CU count is an argument.

A CELL is everything that selects another kernel instantiation or another index path inside one:
    precision / main form / pool, full map kept / strip kind + its columns / deep or forked / Ci (and so the edge kernel's K split) / dup_hi
written as one string, e.g. "split/p_16x16/pool+full/edge_pool2/deep/ci256ks6/dup0". The im2col strip is one kernel with one loop bound r, the
number of columns: its cells are the extremes r = 1 and r = 8; widths with r = 2 .. 7 are named "im2col2-7" and are not cells of their own.

census() walks the 13 conv3x3 layers of the network at their pooling levels over GRID and returns {cell: smallest shape that reaches it};
conv_form_cases.CASES is the committed table of those shapes (regenerate from the repository root: PYTHONPATH=. python tests/conv_forms.py > tests/conv_form_cases.py), plus
DEBUG_ONLY_CASES: the cells only ctpn_debug_conv3x3 reaches, over the channel pairs DEBUG_ONLY_CHANNELS (the non-persistent 128-channel forms
of Co = 192, the 64-channel forms behind Ci = 128, conv1_2's channels without its pool).
tests/test_conv_forms.py keeps the table complete and true; tests/test_gpu_conv_forms.py runs every case against the float64 oracle."""
import functools

import numpy as np

from ctpn_amd import _binding as B

CU = 256                                       # MI355X; the plan's only device-dependent input
PRECS = ("fp32", "split", "fp16", "bf16")
# name, ci, co, pooling level of its input, a 2x2 pool follows
LAYERS = (("conv1_2", 64, 64, 0, True), ("conv2_1", 64, 128, 1, False), ("conv2_2", 128, 128, 1, True), ("conv3_1", 128, 256, 2, False),
          ("conv3_2", 256, 256, 2, False), ("conv3_3", 256, 256, 2, True), ("conv4_1", 256, 512, 3, False), ("conv4_2", 512, 512, 3, False),
          ("conv4_3", 512, 512, 3, True), ("conv5_1", 512, 512, 4, False), ("conv5_2", 512, 512, 4, False), ("conv5_3", 512, 512, 4, False),
          ("rpn_conv/3x3", 512, 512, 4, False))
GRID_N = (1, 2, 3, 32)
GRID_H = (16, 32, 48, 96, 150, 600, 1280)
GRID_W = (16, 2000)                            # every image width in this closed range
# Reachable in the network, not through ctpn_debug_conv3x3_plan's defaults / ctpn_debug_conv3x3, and tested where they are built:
NOT_IN_THE_TABLE = {
    "conv1_1 computed inside conv1_2's launch (16-bit modes, uint8 feed, production path)": "tests/test_gpu_fuse.py",
    "option conv_p64 = 0: conv1_2 of split precision through the non-persistent 64-channel kernel": "tests/test_gpu_round6.py",
    "option split_edge = 0: split precision's ragged columns in the padded tile column": "tests/test_gpu_round6.py",
}


@functools.lru_cache(maxsize=None)
def form_names():
    return B.conv3x3_form_names()


def cell_name(prec, plan, pool, full, ci, dup):
    """plan: one row of B.conv3x3_plan_sweep"""
    mains, strips = form_names()
    main, strip, cols, _cover, deep, ks = (int(v) for v in plan)
    kind = strips[strip]
    if kind == "im2col" and 1 < cols < 8:
        cols = "2-7"
    where = "-" if kind == "none" else ("deep" if deep else "fork")
    return "%s/%s/%s/%s/%s/ci%d%s/dup%d" % (prec, mains[main], ("pool+full" if full else "pool") if pool else "full",
                                            kind if kind == "none" else "%s%s" % (kind, cols), where, ci, "ks%d" % ks if ks > 1 else "", int(dup))


def case_cell(prec, case, cu=CU):
    """the cell of one case (n, h, w, ci, co, pool, want_full, dup_hi) on a device of `cu` CUs (0: the current device)"""
    n, h, w, ci, co, pool, full, dup = case
    plan = B.conv3x3_plan_sweep(prec, n, h, w, 1, ci, co, pool, full or not pool, dup, cu_count=cu)[0]
    return cell_name(prec, plan, pool, bool(full or not pool), ci, dup)


def _sweep_cells(found, prec, n, h, ws, ci, co, pool, full, dup, cu):
    """every width of the sorted array ws (consecutive integers) -> found[cell] = the smallest (pixels, case) seen"""
    plans = B.conv3x3_plan_sweep(prec, n, h, int(ws[0]), len(ws), ci, co, pool, full, dup, cu_count=cu)
    key = plans[:, [0, 1, 2, 4, 5]]
    mid = (plans[:, 1] == 3) & (plans[:, 2] > 1) & (plans[:, 2] < 8)  # the im2col strip between its extremes: no cell
    _, first = np.unique(key, axis=0, return_index=True)              # the smallest width of every distinct plan
    for i in first:
        if mid[i]:
            continue
        cell = cell_name(prec, plans[i], pool, full, ci, dup)
        cand = (n * h * int(ws[i]), (n, h, int(ws[i]), ci, co, pool, full and pool, dup))
        if cell not in found or cand < found[cell]:
            found[cell] = cand


def census(cu=CU, precs=PRECS):
    """{cell: (n, h, w, ci, co, pool, want_full, dup_hi)} over the network's layers on GRID: the smallest map (n * h * w) that reaches each"""
    found = {}
    for prec in precs:
        for _name, ci, co, level, pool_after in LAYERS:
            dup = prec == "split" and _name == "rpn_conv/3x3"
            ws = np.arange(GRID_W[0] >> level, (GRID_W[1] >> level) + 1)
            for h in sorted({h >> level for h in GRID_H}):
                for n in GRID_N:
                    for full in ((False, True) if pool_after else (True,)):      # production / keep_acts
                        _sweep_cells(found, prec, n, h, ws, ci, co, pool_after, full, dup, cu)
    return {cell: case for cell, (_px, case) in found.items()}


# channel pairs no layer of the network has: Co = 192 (neither <= 64 nor a multiple of 128: the non-persistent 128-channel forms), Co = 64 behind
# Ci = 128 (the 64-channel forms outside conv1_2: t64 in the 16-bit modes), and conv1_2's own channels without its pool
DEBUG_ONLY_CHANNELS = ((128, 192), (128, 64), (64, 64))


def debug_only_census(network_cells, cu=CU):
    """the cells that only ctpn_debug_conv3x3 reaches -- every cell over DEBUG_ONLY_CHANNELS that the network's census does not hold: the
    smallest map per cell over a small grid of the shapes at which the forms split (flat / 16 x 16 / 8 x 32, strips, pool, deep / forked)"""
    found = {}
    ws = np.arange(16, 131)
    for prec in PRECS:
        for ci, co in DEBUG_ONLY_CHANNELS:
            if prec == "split" and co % 128 != 0 and co > 64:
                continue                                             # no kernel: split precision needs Co <= 64 or a multiple of 128
            for n in (1, 3):
                for h in (9, 16):
                    for pool, full in ((False, True), (True, False), (True, True)):
                        _sweep_cells(found, prec, n, h, ws, ci, co, pool, full, False, cu)
    return {cell: case for cell, (_px, case) in found.items() if cell not in network_cells}


def cu_dependent(prec, case, cus=(64, 104, 120, 228, 256, 304)):
    """does the case's cell change with the device's CU count (the flat 64-pixel items and the half-tile tail are chosen by it)"""
    return len({case_cell(prec, case, cu) for cu in cus}) > 1


# The layer walks of tests/test_gpu_conv_forms.py: (n, h, w) of the images and what each must cross, as
# (layer, production or kept, fragment of the cell's name) -- checked against the plan by tests/test_conv_forms.py
# The first four are given; none of them has a plain one-column edge strip at Ci = 256 (conv3_2 sees W % 16 = 4, 8, 8 and conv4_1 W % 16 = 2, 4, 4),
# so the census's width for it is added: at 3 x 16 x 904 conv4_1 is 2 x 113 (edge1, Ci = 256) and conv4_2 the same at Ci = 512
WALKS = ((1, 16, 1552), (3, 16, 1552), (1, 32, 1568), (3, 48, 1056), (3, 16, 904))


def walk_cells(prec, n, h, w, keep, cu=CU):
    """{layer: cell} of one forward of n images of h x w"""
    out = {}
    for name, ci, co, level, pool_after in LAYERS:
        dup = prec == "split" and name == "rpn_conv/3x3"
        out[name] = case_cell(prec, (n, h >> level, w >> level, ci, co, pool_after, keep and pool_after, dup), cu)
    return out


if __name__ == "__main__":
    cells = census()
    extra = debug_only_census(cells)
    print('"""Generated by `python tests/conv_forms.py`: cell -> (n, h, w, ci, co, pool, want_full, dup_hi), the smallest shape of the census\n'
          '(tests/conv_forms.py) that reaches the cell on a %d-CU device. %d cells of the network, %d of the debug entry alone."""' % (CU, len(cells), len(extra)))
    for name, table in (("CASES", cells), ("DEBUG_ONLY_CASES", extra)):
        print("%s = {" % name)
        for cell in sorted(table):
            print("    %r: %r," % (cell, tuple(int(v) for v in table[cell])))
        print("}")
