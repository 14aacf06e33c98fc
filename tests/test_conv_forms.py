"""CPU: the census of conv3x3 kernel forms (tests/conv_forms.py) through the library's plan function, against the committed case table
(tests/conv_form_cases.py) that tests/test_gpu_conv_forms.py runs on the device. 445 cells of the network + 125 of the debug entry alone."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import conv_forms as F
from conv_form_cases import CASES, DEBUG_ONLY_CASES


@pytest.fixture(scope="module")
def reachable():
    return F.census()


def test_plan_entry_point_names_and_argument_errors():
    mains, strips = B.conv3x3_form_names()
    assert mains == ["wr", "p64", "t64", "p_flat", "p_flat64", "p_16x16", "p_8x32", "p_8x32_half", "t_flat", "t_16x16", "t_8x32"]
    assert strips == ["none", "edge", "edge_pool", "im2col"]
    # the benchmark's layers at 600 x 900, batch 32, production path: what DESIGN.md describes
    assert B.conv3x3_plan("bf16", 32, 600, 900, 64, 64, True, False, cu_count=256) == ("wr", "none", 0, 0, 0, 0)
    assert B.conv3x3_plan("bf16", 32, 300, 450, 128, 128, True, False, cu_count=256) == ("p_8x32", "edge_pool", 2, 448, 0, 1)
    assert B.conv3x3_plan("split", 32, 150, 225, 256, 256, False, cu_count=256) == ("p_8x32", "edge", 1, 224, 1, 6)
    assert B.conv3x3_plan("split", 1, 150, 225, 128, 256, False, cu_count=256) == ("p_8x32_half", "edge", 1, 224, 1, 6)
    assert B.conv3x3_plan("split", 1, 150, 225, 64, 128, False, cu_count=256).ks == 3
    assert B.conv3x3_plan("fp32", 32, 150, 225, 256, 256, False, cu_count=256) == ("p_8x32", "im2col", 1, 224, 0, 0)
    assert B.conv3x3_plan("bf16", 1, 37, 56, 512, 512, False, cu_count=256).main == "p_flat64"
    assert B.conv3x3_plan("bf16", 32, 37, 56, 512, 512, False, cu_count=256).main == "p_flat"
    assert B.conv3x3_plan("split", 32, 600, 900, 64, 64, True, False, conv_p64=0, cu_count=256).main == "t64"
    assert B.conv3x3_plan("split", 32, 150, 225, 256, 256, False, split_edge=0, cu_count=256).strip == "none"
    for bad in (dict(precision="split", co=192), dict(precision="bf16", ci=96), dict(precision="bf16", dup_hi=True), dict(precision="fp32", n=0),
                dict(precision="fp32", cu_count=-1)):
        kw = dict(precision="fp32", n=1, h=16, w=40, ci=64, co=128, pool=False, cu_count=256)
        kw.update(bad)
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.conv3x3_plan(**kw)
        assert e.value.code == -1, bad
    if B.device_count() == 0:       # cu_count 0 asks a device
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.conv3x3_plan("fp32", 1, 16, 40, 64, 128, False)
        assert e.value.code == -5


def test_every_reachable_cell_has_a_case(reachable):
    """(a) the census over the 13 layers x 4 precisions x n {1, 2, 3, 32} x kept / production x 7 heights x every width 16 .. 2000"""
    missing = sorted(set(reachable) - set(CASES))
    assert not missing, "cells of the network without a case in tests/conv_form_cases.py: %s" % missing[:10]
    stale = sorted(set(CASES) - set(reachable))
    assert not stale, "cases whose cell the census no longer finds: %s" % stale[:10]
    assert len(CASES) == 445 and len(DEBUG_ONLY_CASES) == 125                # the counts DESIGN.md and the docstrings quote
    assert not set(CASES) & set(DEBUG_ONLY_CASES)
    # what the table cannot hold is named, with the file that tests it
    assert len(F.NOT_IN_THE_TABLE) == 3 and all(v.startswith("tests/test_gpu_") for v in F.NOT_IN_THE_TABLE.values())
    # every form and strip kind the library names is reached by some case
    mains, strips = F.form_names()
    cells = list(CASES) + list(DEBUG_ONLY_CASES)
    assert {c.split("/")[1] for c in cells} == set(mains)
    assert {c.split("/")[3].rstrip("0123456789") for c in cells} == set(strips)


def test_every_case_is_the_cell_it_claims_and_the_smallest(reachable):
    """(b) the plan of every committed shape, through the library, on 256 CUs; and the shape is the census's own (the smallest it finds)"""
    for table in (CASES, DEBUG_ONLY_CASES):
        for cell, case in table.items():
            assert F.case_cell(cell.split("/")[0], case) == cell, (cell, case)
            assert len(case) == 8 and case[6] <= case[5] and case[7] == (cell.endswith("dup1"))
    assert {c: tuple(int(v) for v in s) for c, s in reachable.items()} == CASES
    assert {c: tuple(int(v) for v in s) for c, s in F.debug_only_census(reachable).items()} == DEBUG_ONLY_CASES
    for cell, case in DEBUG_ONLY_CASES.items():      # channel pairs no layer has; the 128-channel non-persistent forms are all here, and only here
        assert case[3:5] in F.DEBUG_ONLY_CHANNELS and cell not in reachable
        assert (case[4] == 192) == (cell.split("/")[1] in ("t_flat", "t_16x16", "t_8x32"))
    assert {"t_flat", "t_16x16", "t_8x32"} <= {c.split("/")[1] for c in DEBUG_ONLY_CASES}
    assert not {"t_flat", "t_16x16", "t_8x32"} & {c.split("/")[1] for c in CASES}
    # ... and the 64-channel forms where the network never has them: t64 in the 16-bit modes, t64 / p64 without a pool or behind Ci = 128
    # (a cell's key holds Ci, not Co: the weights-in-registers kernel at Ci = Co = 64 without a pool is conv2_1's cell, in CASES)
    for frag in ("bf16/t64/", "fp16/t64/", "fp32/t64/full/", "split/p64/full/", "fp32/t64/pool/none/-/ci128/", "split/p64/pool/none/-/ci128/"):
        assert any(c.startswith(frag) and v[4] == 64 for c, v in DEBUG_ONLY_CASES.items()), frag
    # layer scale: the largest case is a 75 x 420 map of 128 channels; no 512-channel case is above 16 x 200 pixels
    assert max(c[0] * c[1] * c[2] for c in CASES.values()) <= 31500
    assert max(c[0] * c[1] * c[2] for c in CASES.values() if c[3] == 512) <= 6500


def test_cu_dependence_is_confined_to_the_forms_chosen_by_cu_count():
    for table in (CASES, DEBUG_ONLY_CASES):
        for cell, case in table.items():
            if F.cu_dependent(cell.split("/")[0], case):
                assert cell.split("/")[1] in ("p_flat", "p_flat64", "p_8x32", "p_8x32_half"), cell


# (c) what the walk geometries of tests/test_gpu_conv_forms.py are there to cross: (precision, n, h, w, keep) -> {layer: cell fragment}
WALK_CROSSES = [
    # one image, deep edge kernels: edge 2 at Ci = 256 / 512, edge 1 at Ci = 512 in the non-flat conv5_x / rpn_conv, pooled edges at Ci = 256 / 512
    ("bf16", 1, 16, 1552, False, {"conv3_3": "/pool/edge_pool4/deep/ci256/", "conv4_1": "/full/edge2/deep/ci256/", "conv4_2": "/full/edge2/deep/ci512/",
                                  "conv4_3": "/pool/edge_pool2/deep/ci512/", "conv5_1": "p_8x32_half/full/edge1/deep/ci512/",
                                  "rpn_conv/3x3": "p_8x32_half/full/edge1/deep/ci512/", "conv2_1": "wr/full/im2col8/fork/"}),
    ("fp16", 1, 16, 1552, True, {"conv3_3": "/pool+full/edge_pool4/deep/ci256/", "conv4_3": "/pool+full/edge_pool2/deep/ci512/"}),
    # three images: the same strips forked onto the helper stream, plain 8 x 32 patches
    ("bf16", 3, 16, 1552, False, {"conv3_3": "p_8x32/pool/edge_pool4/fork/ci256/", "conv4_1": "p_8x32/full/edge2/fork/ci256/",
                                  "conv4_3": "p_8x32/pool/edge_pool2/fork/ci512/", "conv5_3": "p_8x32/full/edge1/fork/ci512/",
                                  "rpn_conv/3x3": "p_8x32/full/edge1/fork/ci512/"}),
    ("fp16", 3, 16, 1552, True, {"conv4_3": "p_8x32/pool+full/edge_pool2/fork/ci512/", "conv4_2": "p_8x32/full/edge2/fork/ci512/"}),
    # split precision: the K split of six waves at Ci = 256 / 512, and rpn_conv's [hi | lo | hi] store from the edge kernel (feature column 96)
    ("split", 1, 16, 1552, False, {"conv3_3": "/pool/edge_pool4/deep/ci256ks6/", "conv4_3": "/pool/edge_pool2/deep/ci512ks6/",
                                   "conv5_2": "/full/edge1/deep/ci512ks6/dup0", "rpn_conv/3x3": "p_8x32_half/full/edge1/deep/ci512ks6/dup1"}),
    ("split", 3, 16, 1552, True, {"conv4_1": "p_8x32/full/edge2/deep/ci256ks6/", "rpn_conv/3x3": "p_8x32/full/edge1/deep/ci512ks6/dup1"}),
    # ... and from two edge columns (feature columns 96 and 97); 16 x 16 patches in conv2_x, the im2col strip in conv3_x
    ("split", 1, 32, 1568, False, {"conv4_3": "/pool/edge_pool4/deep/ci512ks6/", "rpn_conv/3x3": "p_8x32_half/full/edge2/deep/ci512ks6/dup1",
                                   "conv2_2": "p_16x16/pool/none/"}),
    ("bf16", 1, 32, 1568, False, {"conv3_1": "/full/im2col8/fork/ci128/", "conv3_2": "/full/im2col8/fork/ci256/", "conv5_1": "p_8x32_half/full/edge2/deep/ci512/",
                                  "conv4_3": "/pool/edge_pool4/deep/ci512/"}),
    ("fp32", 1, 16, 1552, False, {"conv2_1": "/full/im2col8/fork/ci64/", "conv5_1": "/full/im2col1/fork/ci512/"}),
    # the census's width for a one-column edge strip at Ci = 256 (none of the four given geometries has one): forked in the 16-bit modes, deep in split
    ("bf16", 3, 16, 904, False, {"conv4_1": "p_8x32/full/edge1/fork/ci256/", "conv4_2": "p_8x32/full/edge1/fork/ci512/"}),
    ("fp16", 3, 16, 904, True, {"conv4_1": "p_8x32/full/edge1/fork/ci256/"}),
    ("split", 3, 16, 904, False, {"conv4_1": "p_8x32/full/edge1/deep/ci256ks6/", "conv4_2": "p_8x32/full/edge1/deep/ci512ks6/"}),
    # three images of 48 x 1056: 16 x 16 patches in conv3_x, the forked im2col strip, the forked pooled edge at Ci = 512, flat 64-pixel items
    ("bf16", 3, 48, 1056, False, {"conv3_1": "p_8x32/full/im2col8/fork/ci128/", "conv3_3": "p_16x16/pool/none/", "conv4_3": "p_8x32/pool/edge_pool4/fork/ci512/",
                                  "conv5_1": "p_flat64/full/none/"}),
    ("split", 3, 48, 1056, True, {"conv3_2": "p_16x16/full/none/", "conv4_3": "p_8x32/pool+full/edge_pool4/deep/ci512ks6/", "rpn_conv/3x3": "p_flat64/full/none/-/ci512/dup1"}),
]


@pytest.mark.parametrize("prec,n,h,w,keep,crosses", WALK_CROSSES, ids=lambda v: None if isinstance(v, dict) else str(v))
def test_walk_geometries_cross_the_forms_they_are_chosen_for(prec, n, h, w, keep, crosses):
    assert (n, h, w) in F.WALKS
    cells = F.walk_cells(prec, n, h, w, keep)
    for layer, frag in crosses.items():
        assert frag in cells[layer], (layer, cells[layer], frag)


def test_walks_reach_forms_the_150x230_walk_does_not():
    """tests/test_gpu_precision.py's layer walk at 2 x 150 x 230 goes through no strip at all and four main forms; the new geometries add the rest"""
    old = set()
    for prec in ("split", "fp16"):
        old |= set(F.walk_cells(prec, 2, 150, 230, True).values())
    assert all("/none/" in c for c in old) and len({c.split("/")[1] for c in old}) <= 4
    new = set()
    for prec in F.PRECS:
        for n, h, w in F.WALKS:
            for keep in (False, True):
                new |= set(F.walk_cells(prec, n, h, w, keep).values())
    assert {c.split("/")[1] for c in new} >= {"wr", "p64", "t64", "p_16x16", "p_8x32", "p_8x32_half", "p_flat64"}
    assert {c.split("/")[3] for c in new} >= {"none", "edge1", "edge2", "edge_pool2", "edge_pool4", "im2col1", "im2col8"}
    assert any("/fork/" in c and "edge" in c for c in new) and any("/deep/" in c for c in new)
