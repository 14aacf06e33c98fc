"""CPU: the census of tile walks (tests/conv_walks.py) through the library's walk function, against the committed table (tests/conv_walk_cases.py)
that tests/test_gpu_conv_walks.py runs on the device; an independent Python restatement of the walk against the library's numbers; the hooks'
argument domain; the exact recipe's conditions; and numpy models of defective walks that the judges of the GPU file must fail."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
from oracle.rounding import bf16_round, fp16_round
import conv_walks as W
from conv_walk_cases import CASES, DEVICE_CASES
from test_gpu_conv_forms import BOUND, _judge, _problem


def _parts(cell):
    p = cell.split("/")
    return p[0], p[1], p[-1]


def test_the_generated_table_is_current_and_every_cell_is_reached_by_its_case():
    assert {c: tuple(int(v) for v in s) for c, s in W.census().items()} == CASES
    assert {c: tuple(int(v) for v in s) for c, s in W.device_census().items()} == DEVICE_CASES
    assert len(CASES) == 341 and len(DEVICE_CASES) == 19                     # the counts DESIGN.md and CHANGELOG.md quote
    assert {s for _, f, s in map(_parts, CASES) if not f.startswith("wr")} == set(W.P_SITUATIONS) | {"one_round"}
    for cell, case in CASES.items():
        prec, form, sit = _parts(cell)
        k = W.walk_of(prec, case)
        assert k.main == ("wr" if form == "wr_fused" else form) and sit in W.situations(k, case), (cell, case, k)
        assert len(case) == 9 and case[8] in W.GRID_CU and case[3] <= 128 and case[7] == 0
        assert B.conv3x3_plan(prec, *case[:6], bool(case[6]) or not case[5], cu_count=case[8]).strip == "none", cell      # the walk covers the width
    for cell, case in DEVICE_CASES.items():
        prec, form, _ = _parts(cell)
        k = W.walk_of(prec, case, W.CU)
        assert case[8] == 0 and k.main == form and not W.one_item_per_worker(k), (cell, k)
        assert case[3] <= (64 if form in ("wr", "p64") else 128) and case[0] * case[1] * case[2] <= 1 << 18
        if form == "wr":
            assert k.per_group > 80 and k.per_group > 5 * k.workers and case[4] == 128
    # every persistent form in every precision that reaches it, every situation it can be in (conv_walks.NO_CASE says which it cannot)
    for prec in W.PRECS:
        forms = {f for p, f, _ in map(_parts, CASES) if p == prec}
        assert forms >= set(W.P_FORMS) - ({"p64"} if prec != "split" else set()), (prec, forms)
        assert ("wr" in forms) == ("wr_fused" in forms) == (prec in ("bf16", "fp16"))
        for form in forms - {"wr", "wr_fused"}:
            have = {s for p, f, s in map(_parts, CASES) if (p, f) == (prec, form)}
            want = {"one_round", "slice2_keep", "slice4_keep"} if form == "p_flat64" else {"rounds", "partial", "deal_lt8", "deal_rem", "chunks_odd", "chunks_even"}
            if form in W.HT_FORMS:
                want |= {"tail", "halves"}
            if form in ("p_flat", "p_16x16", "p_8x32"):
                want |= {"slice2_keep", "slice2_change", "slice4_keep", "slice4_change"}
            if form == "p_8x32_half":
                want |= {"slice2_keep", "slice4_change"}
            want |= {"p_flat": {"seam_flat"}, "p_16x16": {"seam_stacked", "seam_half", "seam_per_image", "seam_pooled"}, "p_8x32": {"seam_stacked", "seam_per_image", "seam_pooled"},
                     "p64": {"seam_stacked", "seam_per_image", "seam_pooled"}}.get(form, set())
            assert have >= want, (prec, form, sorted(want - have))
        for mode, _pool, _keep in W.WR_MODES if "wr" in forms else ():
            for co in (64, 128):
                have = {c.split("/")[-1] for c in CASES if c.startswith("%s/wr/%s/co%d/" % (prec, mode, co))}
                assert have == set(W.WR_SITUATIONS), (prec, mode, co, have)
        if "wr_fused" in forms:
            assert {c.split("/")[-1] for c in CASES if c.startswith(prec + "/wr_fused/")} == set(W.WR_SITUATIONS)
    assert {f for _, f, _ in map(_parts, DEVICE_CASES)} == {"wr", "p64", "p_flat", "p_16x16", "p_8x32", "p_8x32_half"}      # p_flat64 is one round


def test_every_case_agrees_with_an_independent_restatement_of_the_walk():
    for table, cu_of in ((CASES, lambda c: c[8]), (DEVICE_CASES, lambda c: W.CU)):
        for cell, case in table.items():
            prec, form, sit = _parts(cell)
            form = "wr" if form == "wr_fused" else form
            case = case[:8] + (cu_of(case),)
            lib = W.walk_of(prec, case)._asdict()
            mine = W.restate(prec, form, case)
            assert mine == lib, (cell, case, {f: (mine[f], lib[f]) for f in mine if mine[f] != lib[f]})
            if table is CASES:
                assert sit in W.situations_from_schedule(prec, form, case), (cell, case)
            # the schedule hands out every item once
            if form == "wr":
                sched = W.schedule_wr(mine)
                tiles = sorted(t for v in sched.values() for t in v)
                assert tiles == list(range(mine["total"])), cell
                assert len([key for key in sched if key[1] != "claimed"]) * mine["tiles_n"] == mine["grid"]
            else:
                sched = W.schedule_p(mine)
                items = sorted(it for v in sched for it in v)
                want = [(t, -1) for t in range(mine["ht_full"])] + [(t, hf) for t in range(mine["ht_full"], mine["total"]) for hf in (0, 1)]
                assert items == sorted(want) and len(sched) == mine["grid"], cell
                assert sorted(v[0][0] if v[0][1] < 0 else -1 for v in sched if v and v[0][1] < 0) == list(range(min(mine["grid"], mine["ht_full"]))), cell
                assert mine["ht_full"] + mine["ht_r"] == mine["total"]


def test_the_hooks_argument_domain():
    kw = dict(precision="fp32", n=1, h=16, w=40, ci=64, co=128, pool=False, cu_count=256)
    k = B.conv3x3_walk_plan(**kw)
    assert k == ("p_flat64", 0, 0, 1, 0, 12, 12, 12, 0, 0, 0, 12, 2, 0)
    assert B.conv3x3_walk_plan("bf16", 32, 600, 900, 64, 64, True, False, cu_count=256)[:1] + B.conv3x3_walk_plan("bf16", 32, 600, 900, 64, 64, True, False, cu_count=256)[9:12] == ("wr", 8, 8700, 256)
    assert B.conv3x3_walk_plan("fp32", 1, 16, 40, 64, 64, False, cu_count=256).workers == 0                # t64: a form without a walk
    for bad in (dict(precision="split", co=192), dict(precision="bf16", ci=96), dict(precision="bf16", dup_hi=True), dict(n=0), dict(cu_count=-1), dict(w=0)):
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.conv3x3_walk_plan(**{**kw, **bad})
        assert e.value.code == -1, bad
    x, wt, b = np.zeros((1, 8, 16, 64), np.float32), np.zeros((3, 3, 64, 128), np.float32), np.zeros(128, np.float32)
    for bad in (dict(cu_count=-1), dict(want_full=False)):
        with pytest.raises(ctpn_amd.CtpnError) as e:
            B.debug_conv3x3_walk(x, wt, b, **bad)
        assert e.value.code == -1, bad
    with pytest.raises(ctpn_amd.CtpnError) as e:                                                            # more than 2^22 bordered pixels
        B.debug_conv3x3_walk(np.zeros((1, 2047, 2047, 1), np.float32), np.zeros((3, 3, 1, 8), np.float32), np.zeros(8, np.float32))
    assert e.value.code == -1
    u8 = np.zeros((1, 16, 16, 3), np.uint8)
    w1, b1, w2, b2 = np.zeros((3, 3, 3, 64), np.float32), np.zeros(64, np.float32), np.zeros((3, 3, 64, 64), np.float32), np.zeros(64, np.float32)
    with pytest.raises(ctpn_amd.CtpnError) as e:
        B.debug_conv1_fused(u8, w1, b1, w2, b2, "bf16", cu_count=-1)
    assert e.value.code == -1
    if B.device_count() == 0:       # the launches, and cu_count 0, need a device
        for fn in (lambda: B.conv3x3_walk_plan(**{**kw, "cu_count": 0}), lambda: B.debug_conv3x3_walk(x, wt, b, cu_count=4),
                   lambda: B.debug_conv1_fused(u8, w1, b1, w2, b2, "bf16", cu_count=4)):
            with pytest.raises(ctpn_amd.CtpnError) as e:
                fn()
            assert e.value.code == -5


@pytest.mark.parametrize("prec", W.PRECS)
def test_the_exact_recipe_is_exact_in_any_order(prec):
    x, wt, b, want, pooled = W.exact_problem(prec, 2, 9, 24, 128, 128)
    assert x.min() == 0 and x.max() == 3 and wt.min() == -2 and wt.max() == 2 and np.array_equal(b, np.rint(b))
    assert 9 * 128 * 3 * 2 + 8 < 2 ** 14 < 2 ** 24                           # every partial sum is an integer fp32 holds
    # fp32 accumulation in two orders: taps forwards over channels forwards, and both backwards
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    fwd, bwd = np.tile(b, (2, 9, 24, 1)).astype(np.float32), np.tile(b, (2, 9, 24, 1)).astype(np.float32)
    taps = [(ky, kx) for ky in range(3) for kx in range(3)]
    for ky, kx in taps:
        fwd += xp[:, ky:ky + 9, kx:kx + 24] @ wt[ky, kx]
    for ky, kx in taps[::-1]:
        bwd += xp[:, ky:ky + 9, kx:kx + 24, ::-1] @ wt[ky, kx, ::-1]
    assert np.array_equal(fwd, bwd) and fwd.dtype == np.float32
    exact = np.maximum(fwd, 0)
    if prec in ("fp32", "split"):
        assert np.array_equal(want, exact)
        hi = bf16_round(exact)
        assert np.array_equal(hi + bf16_round(exact - hi), exact)           # split precision stores the value itself
        assert (hi != exact).mean() > 0.2                                    # ... and the lo plane is in use
    else:
        rnd = bf16_round if prec == "bf16" else fp16_round
        assert np.array_equal(want, rnd(exact))
        assert (want != exact).mean() > (0.2 if prec == "bf16" else 0.05)   # the stored value is a rounding (fp16 holds integers below 2048)
    assert (want > 0).mean() > 0.3 and (want == 0).mean() > 0.02 and exact.max() < 2 ** 14 and np.array_equal(pooled, want[:, :8].reshape(2, 4, 2, 12, 2, 128).max(axis=(2, 4)))


# ---------------------------------------------------------------------------------------------------------------
# numpy models of defective walks: the judges of tests/test_gpu_conv_walks.py must fail every one of them
# ---------------------------------------------------------------------------------------------------------------
def _device_like(prec, ref64):
    """what a correct kernel stores for a float64 reference: its rounding to the mode's stored type"""
    r = ref64.astype(np.float32)
    return {"bf16": bf16_round, "fp16": fp16_round}.get(prec, lambda a: a)(r)


def _fill_value(prec):
    """the hook's fill, bytes 0xC3, read as a stored value"""
    if prec == "fp32":
        return np.array([0xC3C3C3C3], np.uint32).view(np.float32)[0]
    if prec == "fp16":
        return np.float32(np.array([0xC3C3], np.uint16).view(np.float16)[0])
    v = np.array([0xC3C30000], np.uint32).view(np.float32)[0]
    return v + v if prec == "split" else v                                    # hi + lo


def _region(k, case, tile, half):
    """the output block of one item of a 2D form that is not stacked, or of the weights-in-registers kernel: (image, rows, columns, channels)"""
    n, h, w = case[:3]
    tw = 16 if k["main"] == "p_16x16" else 32
    th = 256 // tw
    bn = 64 if k["main"] in ("wr", "p64") else 128
    pt, tn = (tile, 0) if k["main"] == "wr" else (tile // k["tiles_n"], tile % k["tiles_n"])
    img, rem = divmod(pt, k["tiles_x"] * k["tiles_y"])
    ty, tx = divmod(rem, k["tiles_x"])
    y0 = ty * th + (th // 2 if half > 0 else 0)
    y1 = min(y0 + (th if half < 0 else th // 2), h)
    return img, slice(y0, y1), slice(tx * tw, min(tx * tw + tw, w)), slice(tn * bn, tn * bn + bn)


def _judges_fail(cell, prec, case, mutate):
    """mutate(array, fill) changes a correct map in place; both value judges must then fail"""
    n, h, w, ci, co = case[:5]
    _x, _wt, _b, want, _ = _problem(prec, n, h, w, ci, co)
    good = _device_like(prec, want)
    _judge(cell, "full map", good, want, BOUND[prec], 0)                      # the model of a correct kernel passes ...
    bad = good.copy()
    mutate(bad, _fill_value(prec))
    with pytest.raises(AssertionError):
        _judge(cell, "full map", bad, want, BOUND[prec], 0)                   # ... the defect does not
    exact = W.exact_problem(prec, n, h, w, ci, co)[3]
    W.judge_bits(cell, exact.copy(), exact)
    bad = exact.copy()
    mutate(bad, _fill_value(prec))
    with pytest.raises(AssertionError):
        W.judge_bits(cell, bad, exact)


def _worker_with(sched, pred):
    return next(v for v in sched if pred(v))


@pytest.mark.parametrize("prec", ["bf16", "split", "fp32"])
def test_mutant_a_later_item_holds_its_workers_first_result(prec):
    cell = prec + "/p_8x32/partial"
    case = CASES[cell]
    assert case[0] == 1 or not W.restate(prec, "p_8x32", case)["stacked"]
    k = W.restate(prec, "p_8x32", case)
    v = _worker_with(W.schedule_p(k), lambda v: len(v) >= 2)

    def mutate(a, _fill):
        i0, r0, c0, ch0 = _region(k, case, *v[0])
        i1, r1, c1, ch1 = _region(k, case, *v[1])
        src = a[i0, r0, c0, ch0]
        dst = a[i1, r1, c1, ch1]
        hh, ww = min(src.shape[0], dst.shape[0]), min(src.shape[1], dst.shape[1])
        dst[:hh, :ww] = src[:hh, :ww]
    _judges_fail(cell, prec, case, mutate)


@pytest.mark.parametrize("prec", ["fp16", "split"])
def test_mutant_half_1_left_at_the_fill(prec):
    cell = prec + "/p_16x16/tail"
    case = CASES[cell]
    k = W.restate(prec, "p_16x16", case)
    assert not k["stacked"] and k["ht_r"] > 0
    tile = k["ht_full"]

    def mutate(a, fill):
        img, rows, cols, ch = _region(k, case, tile, 1)
        assert rows.stop > rows.start, "the tail tile's second half holds rows of the map"
        a[img, rows, cols, ch] = fill
    _judges_fail(cell, prec, case, mutate)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_mutant_a_tile_with_the_neighbouring_slices_weights(prec):
    cell = prec + "/p_8x32/slice2_change"
    case = CASES[cell]
    k = W.restate(prec, "p_8x32", case)
    assert k["tiles_n"] == 2 and not k["stacked"]
    v = _worker_with(W.schedule_p(k), lambda v: len(v) >= 2)

    def mutate(a, _fill):
        img, rows, cols, ch = _region(k, case, *v[1])
        other = slice(128 - ch.start, 256 - ch.start)
        a[img, rows, cols, ch] = a[img, rows, cols, other].copy()
    _judges_fail(cell, prec, case, mutate)


def test_mutant_a_stored_border_row_at_a_seam():
    """what ctpn_debug_conv3x3_walk checks after the launch, restated: a stacked tile that stores the border rows between two images is found, and named"""
    case = CASES["bf16/p_8x32/seam_stacked"]
    n, h, w, _ci, co = case[:5]
    buf = W.guarded_map(n, h, w, co * 2)
    for img in range(n):
        buf[img * (h + 2) + 1:img * (h + 2) + 1 + h, 1:w + 1] = 0x11           # what a correct launch writes: the interior
    assert W.guarded_map_violation(buf, n, h) is None
    k = W.restate("bf16", "p_8x32", case)
    seam_tiles = [t for t in range(k["total"]) if W._tile_spans_images(k, case, t)]
    assert seam_tiles
    bad = buf.copy()
    bad[h + 1, 1:33] = 0x11                                                    # image 0's bottom border row, one tile wide
    assert W.guarded_map_violation(bad, n, h) == (0, h + 1)
    bad = buf.copy()
    bad[h + 2, 5] = 0                                                          # image 1's top border row: a zero is a store too
    assert W.guarded_map_violation(bad, n, h) == (1, 0)
    bad = buf.copy()
    bad[n * (h + 2) + 3, 0, 0] = 0
    assert W.guarded_map_violation(bad, n, h) == ("guard", 3)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_mutants_of_the_claimed_tiles(prec):
    cell = prec + "/wr/full/co64/claims"
    case = CASES[cell]
    k = W.restate(prec, "wr", case)
    sched = W.schedule_wr(k)
    tiles = sched[(7, 0)]
    assert k["workers"] == 1 and len(tiles) >= 8 and tiles[-1] == k["total"] - 1

    def last_missing(a, fill):                                                 # the last claimed tile of the last group never ran
        img, rows, cols, ch = _region(k, case, tiles[-1], -1)
        a[img, rows, cols, ch] = fill

    def twice(a, _fill):                                                       # claimed tile 6 computed twice, the second time into tile 7's place
        i0, r0, c0, ch0 = _region(k, case, tiles[5], -1)
        i1, r1, c1, ch1 = _region(k, case, tiles[6], -1)
        src, dst = a[i0, r0, c0, ch0], a[i1, r1, c1, ch1]
        hh, ww = min(src.shape[0], dst.shape[0]), min(src.shape[1], dst.shape[1])
        dst[:hh, :ww] = src[:hh, :ww]
    _judges_fail(cell, prec, case, last_missing)
    _judges_fail(cell, prec, case, twice)
