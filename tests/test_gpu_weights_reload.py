"""GPU: a ctx's weights are the LAST arena loaded -- every copy pack_weights (csrc/api_weights.hip) derives from the arena follows a second and a
third load into a live ctx, through every kernel that reads it (tests/inflight_cases.py, COPIES: copy -> reader -> case). Every comparison is an
equality of bytes (tests/ctx_walks.py, same) with fresh(): the op on a new ctx that has loaded that arena and done nothing else; the one
tolerance is A5's anchor to the oracle. W1 = util.stress_arena("biased", 3), W2 = ("biased", 4); mixed(k) = W1 with manifest entry k from W2.

  A1 test_reload_whole_arena         load W1, W2, W1 into one live ctx of ctx_walks' capacity; after each load the case's ops (and with keep_acts = 1
                                     every named map of test_gpu_ctx_forgets.MAPS) equal the fresh ctx's for that arena. Cases: RELOAD_CASES
  A2 test_reload_one_entry           for each of the 38 entries, on a ctx of exactly C's size: W1, then mixed(k); uC and `heads` equal the fresh
                                     ctx's for mixed(k), whose heads differ from W1's (else the entry is named as inert)
  A3 test_every_way_in               load_weights_device from a torch tensor (synchronised first: the call reads it on the ctx's stream) on a fresh
                                     ctx and over W1; ctpn_broadcast_weights_rank with world 1 behind a load of W2 over W1. (With world 1 the
                                     root sends to nobody and keeps its own arena, so on a ctx without weights the call is CTPN_ERR_STATE, which
                                     is asserted; the binding cannot name a second ctx's arena, so that way in is not run.)
  A4 test_a_load_changes_nothing_else after forward(A): load W2 -- every stored map, the proposals, every option and parameter, the proposal
                                     capacity and forward_sets() are what they were
  A5 test_reloaded_weights_are_w2    fp32: `heads` of uC after the reload within test_gpu_bias_and_saturation.TOL["fp32"] (max |diff| over the
                                     map's max) of oracle.network.forward with W2

Teeth: run once against a scratch build of the library whose pack_weights, on a second and later load, skips one derived copy (data values
only; no address depends on them), all 52 tests of this file each time. Every failure is at "load 2 (W2)", the first reload:
  wt_xf (launch_lstm_pre_pack)   18 failed: test_reload_whole_arena in fp16 and bf16, all seven cases each (keep_acts too: lstm_pre reads wt_xf
                                 there as well), first "fp16 default: load 2 (W2): uA differs from the fresh ctx's in element 0", and the same for
                                 uC, bD, pAB; resident_lstm_pre (uBig, lstm_pre_kernel) among them; test_reload_one_entry[fp16 / bf16-entries28-38]
                                 names the entries 28 and 30, the two LSTM kernels, and no other; test_every_way_in[fp16 / bf16]. fp32 and
                                 split precision, which have no wt_xf, pass
  wt_fold / b_fold               16 failed: the same tests without the two keep_acts cases, which run the two GEMMs; test_reload_one_entry names
                                 exactly the six folded entries 32 .. 37
  the pack_conv1_frags call      21 failed: test_reload_whole_arena in split precision (default, exact_recurrence, keep_acts) and in the 16-bit
                                 modes in every case but conv1_valu, which reads w_first; test_reload_one_entry[split / fp16 / bf16-entries0-10]
                                 names conv1_1/weights and conv1_1/biases; test_every_way_in in the three. fp32 passes
  the two wh copies              28 failed: every case of test_reload_whole_arena in all four precisions (19), test_reload_one_entry
                                 [*-entries28-38] naming the entries 28 and 30, test_every_way_in in all four, and test_reloaded_weights_are_w2
No mutant went unnoticed, so no case had to be added to the table. The product library passes all 52.

Wall time of each parametrised test on one MI355X (pytest --durations, the fresh results a test is first to ask for included; the 52 tests of
the file together: 23 s): test_fresh_results_are_not_empty 0.16 .. 0.92 s; test_reload_whole_arena 0.11 .. 0.96 s (keep_acts, 22 maps read back
three times, the longest); test_reload_one_entry 0.35 .. 0.51 s per group of eight to ten entries (ten fresh ctxs and twenty loads: no group
comes near the ten seconds at which it would be split further); test_every_way_in 0.63 s (4.7 s for the first of the process, which loads
librccl and starts torch's device context); test_a_load_changes_nothing_else 0.18 .. 0.53 s; test_reloaded_weights_are_w2 under a second."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import ctx_walks as W
import inflight_cases as K
import test_gpu_bias_and_saturation as BS
import test_gpu_ctx_forgets as F

pytestmark = pytest.mark.gpu

CASES = [(prec, name) for name, case in K.RELOAD_CASES.items() for prec in case.precs]


@pytest.fixture(autouse=True)
def _options_come_from_the_tests_only(monkeypatch):
    for var in B.OPTION_ENV.values():                      # the binding maps these onto every Context; other modules set some of them
        monkeypatch.delenv(var, raising=False)


@pytest.mark.parametrize("prec", W.PRECS)
def test_fresh_results_are_not_empty(prec):
    """both arenas yield rois on every op (asserted in fresh) and lines on A and C; the two arenas' results differ; the 16-bit modes reach both
    lstm_pre forms on this device (ctpn_debug_lstm_pre_plan with the device's own CU count)"""
    ops = ("uA", "uC", "bD", "pAB") + (("uBig",) if prec in K.HALF else ())
    for name in ops:
        r1, r2 = K.fresh(prec, "W1", name), K.fresh(prec, "W2", name)
        assert W.same(r1, r2) is not None, name
    for akey in ("W1", "W2"):
        for name in ("uA", "uC"):
            k = W.LINES[name][0]
            lines = sum(x.shape[0] for x in K.fresh(prec, akey, name)[:k])
            print(prec, akey, name, "lines:", lines, "rois:", K.rows(K.fresh(prec, akey, name), 5, np.float32))
            assert lines > 0, "%s %s %s: no text line; take the next seed for W2 (tests/inflight_cases.py, SEEDS)" % (prec, akey, name)
    if prec in K.HALF:
        forms = {op: B.lstm_pre_plan(cells, cu_count=0).form for op, cells in K.LSTM_PRE_CELLS.items()}
        assert forms["uBig"] == "lds" and forms["uA"] == "small", forms


@pytest.mark.parametrize("prec,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_reload_whole_arena(prec, name):
    case = K.RELOAD_CASES[name]
    maps = F.MAPS if case.maps else ()
    failed = []
    with ctpn_amd.Context(0, *W.CAP, prec, options=case.options) as ctx:
        for step, akey in enumerate(("W1", "W2", "W1")):
            ctx.load_weights(K.arena(akey))
            for op in case.ops:
                want = K.fresh(prec, akey, op, case.options, maps=maps)
                at = W.same(K.FRESH_RUN[op](ctx), want[0] if maps else want)
                if at is not None:
                    failed.append("load %d (%s): %s differs from the fresh ctx's in element %d" % (step + 1, akey, op, at))
                for nm in maps:          # a stale copy is named by its layer
                    if W.same((ctx.get_tensor(nm),), (want[1][nm],)) is not None:
                        failed.append("load %d (%s): %s behind %s differs from the fresh ctx's" % (step + 1, akey, nm, op))
    assert not failed, "%s %s %r: %s" % (prec, name, case.options, "; ".join(failed[:12]))


@pytest.mark.parametrize("lo,hi", K.A2_GROUPS, ids=["entries%d-%d" % g for g in K.A2_GROUPS])
@pytest.mark.parametrize("prec", W.PRECS)
def test_reload_one_entry(prec, lo, hi):
    names = [n for n, _, _ in K.manifest()]
    base = K.fresh(prec, "W1", "uC+heads", cap=W.C)
    failed, inert = [], []
    with ctpn_amd.Context(0, *W.C, prec) as ctx:
        for k in range(lo, hi):
            ctx.load_weights(K.arena("W1"))
            if W.same(K.FRESH_RUN["uC+heads"](ctx), base) is not None:
                failed.append("entry %d: W1 again differs from the fresh ctx's" % k)
            want = K.fresh(prec, ("M", k), "uC+heads", cap=W.C)
            if W.same((want[-1],), (base[-1],)) is None:
                inert.append("%d %s" % (k, names[k]))
            ctx.load_weights(K.mixed(k))
            at = W.same(K.FRESH_RUN["uC+heads"](ctx), want)
            if at is not None:
                failed.append("entry %d (%s): element %d differs from the fresh ctx's for W1 with that entry from W2" % (k, names[k], at))
    assert not inert, "entries that do not reach `heads` (the equality proves nothing for them): %s" % ", ".join(inert)
    assert not failed, "%s: %s" % (prec, "; ".join(failed))


@pytest.mark.parametrize("prec", W.PRECS)
def test_every_way_in(prec):
    import torch
    w2_dev = torch.from_numpy(np.array(K.arena("W2"))).cuda()
    torch.cuda.synchronize()                               # ctpn_load_weights_device reads the tensor on the ctx's stream (include/ctpn_hip.h)
    ops = ("uA", "pAB")
    failed = []

    def check(ctx, akey, what):
        for op in ops:
            at = W.same(K.FRESH_RUN[op](ctx), K.fresh(prec, akey, op))
            if at is not None:
                failed.append("%s: %s differs from load_weights(%s) on a fresh ctx in element %d" % (what, op, akey, at))

    with ctpn_amd.Context(0, *W.CAP, prec) as ctx:
        with pytest.raises(ctpn_amd.CtpnError) as e:       # world 1: the root keeps its arena, and a root without one is refused
            ctx.broadcast_weights_rank(B.comm_unique_id(), 0, 1, root=0)
        assert e.value.code == K.CTPN_ERR_STATE
        ctx.load_weights_device(w2_dev.data_ptr())
        check(ctx, "W2", "load_weights_device on a fresh ctx")
    with ctpn_amd.Context(0, *W.CAP, prec) as ctx:
        ctx.load_weights(K.arena("W1"))
        check(ctx, "W1", "load_weights")
        ctx.load_weights_device(w2_dev.data_ptr())
        check(ctx, "W2", "load_weights_device over W1")
        ctx.load_weights(K.arena("W1"))
        ctx.load_weights(K.arena("W2"))
        ctx.broadcast_weights_rank(B.comm_unique_id(), 0, 1, root=0)
        B.broadcast_weights([ctx])
        check(ctx, "W2", "broadcast_weights_rank, world 1, behind W2 over W1")
    del w2_dev
    assert not failed, "%s: %s" % (prec, "; ".join(failed))


@pytest.mark.parametrize("keep_acts", [0, 1])
@pytest.mark.parametrize("prec", W.PRECS)
def test_a_load_changes_nothing_else(prec, keep_acts):
    x = W.inputs()
    info = W._info([W.A[1]] * W.A[0], W.A[2])

    def stored(ctx):
        out = {}
        for nm in F.MAPS:
            try:
                out[nm] = ctx.get_tensor(nm)
            except ctpn_amd.CtpnError as e:                # what the production path does not store is refused, before the load and after it
                out[nm] = int(e.code)
        return out

    with ctpn_amd.Context(0, *W.CAP, prec, options={"keep_acts": keep_acts}) as ctx:
        ctx.load_weights(K.arena("W1"))
        ctx.forward(x["A"])
        maps = stored(ctx)
        rois, anchors = ctx.proposals(info, want_anchors=True)
        state = K.FRESH_RUN["introspect"](ctx) + (ctx.forward_sets(),)
        ctx.load_weights(K.arena("W2"))
        after = stored(ctx)
        arrays = [nm for nm in F.MAPS if isinstance(maps[nm], np.ndarray)]
        assert "heads" in arrays and len(arrays) >= (22 if keep_acts else 16), arrays
        for nm in F.MAPS:
            a, b = maps[nm], after[nm]
            assert (W.same((a,), (b,)) is None) if isinstance(a, np.ndarray) else a == b, "%s changed with the load" % nm
        rois2, anchors2 = ctx.proposals(info, want_anchors=True)
        assert W.same(tuple(rois) + tuple(anchors), tuple(rois2) + tuple(anchors2)) is None and sum(r.shape[0] for r in rois) > 0
        assert K.FRESH_RUN["introspect"](ctx) + (ctx.forward_sets(),) == state
        ctx.forward(x["A"])                                # and the weights did change
        assert W.same((ctx.get_tensor("heads"),), (maps["heads"],)) is not None


def test_reloaded_weights_are_w2():
    """A5. Measured on one MI355X: 1.11e-6 against the bound of 5e-6; the oracle's own heads with W1 lie 1.32 (relative) from those with W2."""
    from oracle import network as N
    with ctpn_amd.Context(0, *W.CAP, "fp32") as ctx:
        ctx.load_weights(K.arena("W1"))
        K.FRESH_RUN["uC"](ctx)
        ctx.load_weights(K.arena("W2"))
        got = K.FRESH_RUN["uC+heads"](ctx)
    assert W.same(got, K.fresh("fp32", "W2", "uC+heads")) is None
    ref = N.forward(W.inputs()["C"], ctpn_amd.arena_views(K.arena("W2")), keep={"rpn_cls_score"})
    want = np.concatenate([ref["rpn_bbox_pred"], ref["rpn_cls_score"]], axis=-1)
    heads = got[-1][..., :60]
    err = BS.fig("heads of uC behind a reload, against the oracle with W2", "fp32", "biased seed 4", W.C, BS.rel(heads, want), BS.TOL["fp32"])
    stale = N.forward(W.inputs()["C"], ctpn_amd.arena_views(K.arena("W1")), keep={"rpn_cls_score"})
    far = BS.rel(np.concatenate([stale["rpn_bbox_pred"], stale["rpn_cls_score"]], axis=-1), want)
    print("the oracle's heads with W1 against those with W2: %.3g" % far)
    assert far > 1e3 * BS.TOL["fp32"]                      # the anchor can tell the arenas apart
    assert err < BS.TOL["fp32"], err
