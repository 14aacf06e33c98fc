"""GPU: a ctx has no memory -- a call's result depends on its arguments and on the ctx's options and parameters, not on what the ctx did
before (the hand-kept state of csrc/ctx.h and the api_*.hip units: the geometry a forward set's borders are zero for, act_valid / fc_valid /
fwd_ragged / tail_pending / ev_decoded, last / set1_state / img_flip and the staging buffers, the ragged sets, nms_mw_dirty, last_post / last_plan,
the setters that switch kernel forms on a live ctx). Every comparison is an equality of bytes (tests/ctx_walks.py, same) with fresh(): the op on
a new ctx of the SAME capacity (5, 304, 1040) that has done nothing else, computed once per (precision, op, options) and shared.

  a  test_every_ordered_pair        one live ctx at default options walks an Eulerian circuit over all 17 data-ops: 290 calls, every ordered
                                    pair of ops (an op after itself included) once as neighbours
  b  test_option_excursion          uA | set | uA uB rW uA | set back | uA uB rW for every non-default value of conv1_kernel, conv1_fuse, lstm_split,
                                    conv_p64, split_edge, keep_acts (defaults read from the ctx): the geometry stays, so nothing is re-zeroed
  c  test_seeded_walk               120 data-ops with nms_columns / nms_prefix / nms_check / connect_device / tail_overlap / tail_confine and
                                    ctpn_reserve_proposals 1000 / 2048 / 4096 between them: every result is the default ctx's
  d  test_capacity_changes_nothing  uA, uB, uC, rW on a ctx of exactly their own size

Wall time of each parametrised test on one MI355X (pytest --durations, the fresh results a test is first to ask for included; the 56 tests of
the file together: 15 s, creating and loading 156 fresh and 52 live ctxs among it):

  test                              fp32      split     fp16      bf16
  test_fresh_results_are_not_empty  0.83 s    0.36 s    0.45 s    0.92 s
  test_every_ordered_pair           0.80 s    0.46 s    0.28 s    0.49 s      (290 calls: 1 .. 3 ms a call, comparison included)
  test_option_excursion, keep_acts  0.56 s    0.49 s    0.51 s    0.31 s      (22 named maps of uA read back twice)
  test_option_excursion, the others 0.13 .. 0.15 s  0.13 .. 0.17 s  0.09 .. 0.13 s  0.12 .. 0.14 s
  test_seeded_walk, per seed        0.37 .. 0.43 s  0.25 .. 0.28 s  0.17 .. 0.20 s  0.15 .. 0.17 s
  test_capacity_changes_nothing     --        0.03 s    --        0.02 .. 0.03 s

None comes near the ten seconds at which a walk would be split into halves.

Teeth, beside tests/test_ctx_walks.py: run once against a scratch build of the library whose forward_impl skips the three border re-zero memsets
(the geometry test of csrc/api_forward.hip, "borders must be zero for this geometry"; data values only, no address depends on them),
test_every_ordered_pair[bf16] failed at 254 of its 290 steps; the first failing pair was (uA, uB), step 2 ("uB differs from the fresh
ctx's in element 0, after uA uA"). The product library passes all 56: no pair, excursion or walk found a leak."""
import time

import numpy as np
import pytest

import ctpn_amd
import ctx_walks as W

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3)          # tests/test_ctx_walks.py holds their coverage
# (option, index into its non-default values in ascending order); the ranges are ctpn_set_option's (include/ctpn_hip.h)
RANGES = {"conv1_kernel": (0, 2), "conv1_fuse": (0, 1), "lstm_split": (0, 1), "conv_p64": (0, 1), "split_edge": (0, 1), "keep_acts": (0, 1)}
EXCURSIONS = [(name, k) for name, (lo, hi) in RANGES.items() for k in range(hi - lo)]
MAPS = ("conv1_1", "conv1_2", "pool1", "conv2_1", "conv2_2", "pool2", "conv3_1", "conv3_2", "conv3_3", "pool3", "conv4_1", "conv4_2", "conv4_3",
        "pool4", "conv5_1", "conv5_2", "conv5_3", "rpn_conv/3x3", "lstm_pre", "lstm_out", "lstm_o", "heads")
POOL_FUSED = ("conv1_2", "conv2_2", "conv3_3", "conv4_3")          # stored only with keep_acts = 1
CTPN_ERR_STATE = -3

_fresh = {}


def _rows(result, cols, dtype):
    return sum(x.shape[0] for x in result if isinstance(x, np.ndarray) and x.ndim == 2 and x.shape[1] == cols and x.dtype == dtype)


def fresh(prec, name, options=None, want_maps=False):
    """the op's result on a new ctx of capacity CAP that has done nothing else (with want_maps: and every named map behind it)"""
    key = (prec, name, tuple(sorted((options or {}).items())), want_maps)
    if key not in _fresh:
        with ctpn_amd.Context(0, *W.CAP, prec, options=options or {}) as ctx:
            ctx.load_weights(W.weights())
            res = W.OP[name].run(ctx)
            maps = {nm: ctx.get_tensor(nm) for nm in MAPS} if want_maps else None
        if W.OP[name].kind == "error":
            assert res == W.ERROR_CODES[name], (prec, name, res)
        else:
            assert _rows(res, 5, np.float32) > 0, "%s %s: the fresh result holds no roi, an equality with it would be empty" % (prec, name)
        _fresh[key] = (res, maps) if want_maps else res
    return _fresh[key]


def live_ctx(prec, cap=W.CAP):
    ctx = ctpn_amd.Context(0, *cap, prec)
    ctx.load_weights(W.weights())
    return ctx


@pytest.mark.parametrize("prec", W.PRECS)
def test_fresh_results_are_not_empty(prec):
    """every op yields rois (asserted in fresh), both DETECT_MODEs yield lines, the device-pointer call is the host call, errors are their codes"""
    res = {o.name: fresh(prec, o.name) for o in W.OPS}
    lines = {"H": 0, "O": 0}
    for name, (k, mode) in W.LINES.items():
        assert all(x.ndim == 2 and x.shape[1] == 9 and x.dtype == np.float64 for x in res[name][:k])
        lines[mode] += sum(x.shape[0] for x in res[name][:k])
    print(prec, "rois per op:", {n: _rows(r, 5, np.float32) for n, r in res.items()}, "lines per mode:", lines)
    assert lines["H"] > 0 and lines["O"] > 0
    assert W.same(res["dC"], res["uC"]) is None
    assert W.same(res["uC"], res["uC2"]) is not None and W.same(res["rW"], res["uW"]) is not None      # the neighbours that share a geometry differ


def run_walk(prec, names, first_step=0):
    """the ops in order on one live ctx; -> the failed steps as messages naming the step, the op and the three ops before it"""
    failed = []
    with live_ctx(prec) as ctx:
        for i, name in enumerate(names):
            at = W.same(W.OP[name].run(ctx), fresh(prec, name))
            if at is not None:
                failed.append("step %d: %s differs from the fresh ctx's in element %d, after %s" % (first_step + i, name, at, " ".join(names[max(0, i - 3):i]) or "nothing"))
    return failed


@pytest.mark.parametrize("prec", W.PRECS)
def test_every_ordered_pair(prec):
    names = [W.OPS[i].name for i in W.pair_walk(len(W.OPS))]
    t0 = time.perf_counter()
    failed = run_walk(prec, names)
    print("%s: %d calls in %.2f s, %d failed" % (prec, len(names), time.perf_counter() - t0, len(failed)))
    assert not failed, "%d of %d steps: %s" % (len(failed), len(names), "; ".join(failed[:8]))


@pytest.mark.parametrize("opt,k", EXCURSIONS, ids=["%s-%d" % e for e in EXCURSIONS])
@pytest.mark.parametrize("prec", W.PRECS)
def test_option_excursion(prec, opt, k):
    failed = []
    with live_ctx(prec) as ctx:
        dflt = ctx.get_option(opt)
        value = [v for v in range(RANGES[opt][0], RANGES[opt][1] + 1) if v != dflt][k]
        there = {opt: value}

        def step(name, options, what):
            at = W.same(W.OP[name].run(ctx), fresh(prec, name, options))
            if at is not None:
                failed.append("%s %s: element %d differs from the fresh ctx's with %r" % (name, what, at, options))

        step("uA", {}, "at first")
        ctx.set_option(opt, value)
        step("uA", there, "behind the set")
        if opt == "keep_acts":          # 0 -> 1: every named map is the fresh keep_acts ctx's
            want = fresh(prec, "uA", there, want_maps=True)[1]
            for nm in MAPS:
                got = ctx.get_tensor(nm)
                if W.same((got,), (want[nm],)) is not None:
                    failed.append("keep_acts 0 -> 1: %s differs from the fresh keep_acts ctx's" % nm)
        for name in ("uB", "rW", "uA"):
            step(name, there, "with %s = %d" % (opt, value))
        ctx.set_option(opt, dflt)
        step("uA", {}, "behind the set back")
        if opt == "keep_acts":          # 1 -> 0: what the production path does not store is refused, not handed out from the earlier forward
            for nm in POOL_FUSED + (("lstm_o",) if prec in ("fp16", "bf16") else ()):
                with pytest.raises(ctpn_amd.CtpnError) as e:
                    ctx.get_tensor(nm)
                assert e.value.code == CTPN_ERR_STATE and "keep_acts" in str(e.value), nm
        for name in ("uB", "rW"):
            step(name, {}, "after the excursion")
    assert not failed, "%s = %d (default %d): %s" % (opt, value, dflt, "; ".join(failed))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("prec", W.PRECS)
def test_seeded_walk(prec, seed):
    walk = W.random_walk(seed, 120)
    failed, done = [], []
    with live_ctx(prec) as ctx:
        for item in walk:
            if item[0] != "op":
                W.apply_action(ctx, item)
                done.append("%s=%d" % (item[-2], item[-1]))
                continue
            at = W.same(W.OP[item[1]].run(ctx), fresh(prec, item[1]))
            if at is not None:
                failed.append("item %d: %s differs from the fresh ctx's in element %d, after %s" % (len(done), item[1], at, " ".join(done[-6:]) or "nothing"))
            done.append(item[1])
    assert not failed, "seed %d, %d of 120 ops: %s" % (seed, len(failed), "; ".join(failed[:8]))


@pytest.mark.parametrize("name,cap", [("uA", W.A), ("uB", W.B), ("uC", W.C), ("rW", (5, 96, 82))])
@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_capacity_changes_nothing(prec, name, cap):
    """the conv plan (ctpn_debug_conv3x3_plan) takes n, h, w and no capacity: a ctx of exactly the batch's size gives the bytes of the large one"""
    with live_ctx(prec, cap) as ctx:
        at = W.same(W.OP[name].run(ctx), fresh(prec, name))
    assert at is None, "%s on a ctx of %r: element %d differs from the ctx of %r" % (name, cap, at, W.CAP)
