"""GPU (-m gpu): the tile walks of the persistent conv3x3 kernels -- rounds, tails, halves, channel slices, image seams, static and claimed items --
one case per WALK CELL of tests/conv_walk_cases.py (tests/conv_walks.py says what a cell is and how the table is made; tests/test_conv_walks.py keeps
it true). A case runs ctpn_debug_conv3x3_walk: the product kernels with the main launch laid out for the cell's CU count (3 .. 24 workgroups on a
map of a few thousand pixels, so that workgroups run second and later items), outputs and 64 guard rows behind them pre-filled, every border pixel
and guard row checked by the hook (CTPN_ERR_STATE, which fails the case).

Per cell:
  float64 bound   the reference and the bounds of tests/test_gpu_conv_forms.py (_problem, _judge, BOUND), on the full and the pooled map
  byte equality   the same shape launched with every item on a worker of its own -- the walk tests/conv_form_cases.py pins: cu_count 0, or, where the
                  device's count would take another main form (p_flat / p_flat64, p_8x32 / p_8x32_half), the nearest count that keeps it
                  (28 anchors -- p_flat64's one round, one-tile launches of all halves, wr launches of one tile -- are the same launch at every
                  count that keeps their form: there the comparison is a second run, and the bound and the exact recipe carry the cell)
  exact recipe    integer data whose fp32 sums are exact in any order (conv_walks.exact_problem): the stored bits are oracle/rounding.py of the
                  exact value, whatever the launch
  run to run      a second run stores the same bytes
  pool            the fused pool is the max of the stored full map
  dup_hi          split precision without a pool: the [hi | lo | hi] layout under the same walk stores the same hi + lo, its third plane the first
The fused conv1_1 form (wr_fused) is compared, byte for byte, with ctpn_debug_conv1_fused at the device's own count (tests/test_gpu_first_kernels.py
bounds that against the oracle) and with its own second run.
DEVICE_CASES run at cu_count 0 with two or more rounds on the device itself; a case whose walk differs on a device of another CU count skips.
One line per cell: profiles/conv_walk_cells.txt."""
import functools

import numpy as np
import pytest

from ctpn_amd import _binding as B
from oracle import network as N
import conv_walks as W
import first_cells as C1
from conv_walk_cases import CASES, DEVICE_CASES
from test_gpu_conv_forms import BOUND, _judge, _problem

pytestmark = pytest.mark.gpu


def _key(kv):
    return (kv[0].split("/")[0], kv[1][:5], kv[0])      # neighbours share a problem (the reference cache of test_gpu_conv_forms._problem)


OVERRIDE = sorted(((c, v) for c, v in CASES.items() if "/wr_fused/" not in c), key=_key)
FUSED = sorted(((c, v) for c, v in CASES.items() if "/wr_fused/" in c), key=_key)
DEVICE = sorted(DEVICE_CASES.items(), key=_key)
_ids = lambda cases: [c.replace("/", ".") for c, _ in cases]


@functools.lru_cache(maxsize=None)
def device_cu():
    """the device's CU count: the grid of a launch with more tiles than any device has CUs"""
    return B.conv3x3_walk_plan("fp32", 8, 64, 256, 32, 128, False, cu_count=0).workers


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _run(prec, case, data, cu):
    """one launch of the case's form -> (full or None, pooled or None)"""
    _n, _h, _w, _ci, _co, pool, keep, dup, _cu = case
    x, wt, b = data
    return B.debug_conv3x3_walk(x, wt, b, precision=prec, fuse_pool=bool(pool), want_full=bool(keep or not pool), cu_count=cu, dup_hi=bool(dup))


def _check_cell(cell, case, cu, ref_cu):
    prec = cell.split("/")[0]
    n, h, w, ci, co, pool, keep, dup, _ = case
    tol = BOUND[prec]
    x, wt, b, want, want_pool = _problem(prec, n, h, w, ci, co)
    plan = B.conv3x3_plan(prec, n, h, w, ci, co, pool, keep or not pool, dup, cu_count=cu)
    pcols = plan.cols // 2 if plan.strip == "edge_pool" else 0
    full, pooled = _run(prec, case, (x, wt, b), cu)
    errs = []
    if full is not None:
        errs.append(_judge(cell, "full map", full, want, tol, plan.cols)[0])
    if pooled is not None:
        errs.append(_judge(cell, "pooled map", pooled, want_pool, tol, pcols)[0])
        if full is not None:
            assert np.array_equal(pooled, N.maxpool2x2(full)), cell            # the fused pool is the max of what the full-resolution store holds
    # every item on a worker of its own: the same bytes
    rfull, rpooled = _run(prec, case, (x, wt, b), ref_cu)
    for what, a, r in (("full map", full, rfull), ("pooled map", pooled, rpooled)):
        assert (a is None) == (r is None) and (a is None or _bits_equal(a, r)), (cell, what, "differs from the launch at cu_count %d" % ref_cu)
    # run to run
    afull, apooled = _run(prec, case, (x, wt, b), cu)
    assert (full is None or _bits_equal(full, afull)) and (pooled is None or _bits_equal(pooled, apooled)), (cell, "a second run differs")
    # split precision's [hi | lo | hi] pixel (the layer that feeds the LSTM projection): the same walk storing a third plane, which the hook compares
    # with the first; hi + lo are the bytes of the two-plane launch
    if prec == "split" and not pool:
        dfull = B.debug_conv3x3_walk(x, wt, b, precision=prec, cu_count=cu, dup_hi=True)[0]
        assert _bits_equal(dfull, full), (cell, "the dup_hi layout stores other values")
    # the exact recipe
    xe, we, be, efull, epool = W.exact_problem(prec, n, h, w, ci, co)
    gfull, gpooled = _run(prec, case, (xe, we, be), cu)
    cnt = 0
    if gfull is not None:
        cnt += W.judge_bits((cell, "exact recipe, full map"), gfull, efull)
    if gpooled is not None:
        cnt += W.judge_bits((cell, "exact recipe, pooled map"), gpooled, epool)
    k = W.walk_of(prec, case, cu)
    print("WALK %-40s %-22s cu %3d  G %3d items %4d (%d halves)  ref cu %3d  err %.3e of %.1e  exact %d values" % (
        cell, "x".join(str(v) for v in case[:5]), cu, k.grid, k.ht_full + 2 * k.ht_r if k.main != "wr" else k.total, 2 * k.ht_r, ref_cu, max(errs), tol, cnt))


@pytest.mark.parametrize("cell,case", OVERRIDE, ids=_ids(OVERRIDE))
def test_walk_cell(cell, case):
    prec, form = cell.split("/")[:2]
    cu = case[8]
    assert 0 < cu <= device_cu(), "the override list runs on any device with %d CUs or more" % cu
    k = W.walk_of(prec, case)
    assert k.main == form and cell.split("/")[-1] in W.situations(k, case), (cell, k)
    # a second item somewhere, except in the anchors and in p_flat64 (one round by its plan)
    assert not W.one_item_per_worker(k) or cell.split("/")[-1] in ("halves", "empty") or form == "p_flat64", (cell, k)
    ref_cu = W.reference_cu(prec, case, device_cu())
    assert ref_cu is not None, cell
    rk = W.walk_of(prec, case, ref_cu)
    assert rk.main == form and W.one_item_per_worker(rk), (cell, ref_cu, rk)      # the nearest count that keeps the form: asserted in the cell
    _check_cell(cell, case, cu, ref_cu)


@pytest.mark.parametrize("cell,case", DEVICE, ids=_ids(DEVICE))
def test_walk_cell_on_the_devices_own_cu_count(cell, case):
    prec, form = cell.split("/")[:2]
    here, table = W.walk_of(prec, case, 0), W.walk_of(prec, case, W.CU)
    if here != table:
        # same shape, same options: only the CU count differs (a device of 256 CUs must give the table's walk), and between the walks of one form
        # or of the two pairs of forms the count chooses between
        assert device_cu() != W.CU and {here.main, table.main} in ({form}, {"p_flat", "p_flat64"}, {"p_8x32", "p_8x32_half"}), \
            "the walk of %r is %s on this device of %d CUs, the table says %s" % (case, here, device_cu(), table)
        pytest.skip("%s: its main form is chosen by the CU count (256 in the table); this device takes %s" % (cell, here.main))
    assert here.main == form and not W.one_item_per_worker(here)
    # the reference: the nearest override that keeps the form is the device's count itself here, so compare with the largest override that
    # changes the walk and keeps the form (half the CUs)
    ref_cu = next(cu for cu in range(device_cu() // 2, 0, -1) if W.walk_of(prec, case, cu).main == form)
    _check_cell(cell, case, 0, ref_cu)


@pytest.mark.parametrize("cell,case", FUSED, ids=_ids(FUSED))
def test_fused_conv1_walk_cell(cell, case):
    prec = cell.split("/")[0]
    n, h, w, _ci, _co, _pool, _keep, _dup, cu = case
    k = W.walk_of(prec, case)
    assert k.main == "wr" and cell.split("/")[-1] in W.situations(k, case) and cu <= device_cu()
    assert W.one_item_per_worker(W.walk_of(prec, case, 0))
    wts = C1.normal_weights()
    images = C1.normal_images(n, h, w)
    pool, bits = B.debug_conv1_fused(images, *wts, precision=prec, cu_count=cu)
    ref_pool, ref_bits = B.debug_conv1_fused(images, *wts, precision=prec)
    cnt = C1.judge_same_bytes((cell, "the device's own count"), bits, ref_bits)
    assert np.array_equal(pool, ref_pool)
    again = B.debug_conv1_fused(images, *wts, precision=prec, cu_count=cu)
    C1.judge_same_bytes((cell, "again"), again[1], bits)
    print("WALK %-40s %-22s cu %3d  G %3d items %4d  0 of %d stored values differ from the launch at cu_count 0" % (
        cell, "%dx%dx%d" % (n, h, w), cu, k.grid, k.total, cnt))


def test_a_cu_count_outside_1_to_the_devices_own_is_refused():
    x, wt, b = np.zeros((1, 8, 16, 64), np.float32), np.zeros((3, 3, 64, 128), np.float32), np.zeros(128, np.float32)
    for cu in (device_cu() + 1, 1 << 20, -1):
        with pytest.raises(B.CtpnError) as e:
            B.debug_conv3x3_walk(x, wt, b, "bf16", cu_count=cu)
        assert e.value.code == -1, cu
    for cu in (1, device_cu()):
        assert B.debug_conv3x3_walk(x, wt, b, "bf16", cu_count=cu)[0].shape == (1, 8, 16, 128)
    u8 = np.zeros((1, 16, 16, 3), np.uint8)
    with pytest.raises(B.CtpnError) as e:
        B.debug_conv1_fused(u8, *C1.normal_weights(), precision="bf16", cu_count=device_cu() + 1)
    assert e.value.code == -1


@pytest.mark.parametrize("shape,tiles", [((1, 24, 96), 9), ((1, 64, 256), 64)], ids=["9_tiles_static", "64_tiles_claims"])
def test_130_wr_launches_lap_the_64_counter_slots_twice(shape, tiles):
    """every launch of the weights-in-registers kernel takes the next of 64 slots of claim counters and its last workgroup re-arms them: 130
    consecutive launches are two laps and two launches, so every slot has been used after a re-arm. 9 tiles at cu_count 8: two static items per
    worker at the most and one group without a tile (the early exit counts as finished); 64 tiles: three claimed tiles per worker."""
    n, h, w = shape
    case = (n, h, w, 64, 64, 0, 0, 0, 8)
    k = W.walk_of("bf16", case)
    assert k.main == "wr" and k.total == tiles and k.workers == 1
    x, wt, b, want, _ = _problem("bf16", n, h, w, 64, 64)
    first = _run("bf16", case, (x, wt, b), 8)[0]
    _judge("130 launches", "full map", first, want, BOUND["bf16"], 0)
    for i in range(2, 131):
        got = _run("bf16", case, (x, wt, b), 8)[0]
        if i in (65, 130):                                                       # the two checkpoints: one lap and one launch, two laps and two
            assert _bits_equal(got, first), "launch %d stores other bytes than the first" % i
