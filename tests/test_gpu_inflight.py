"""GPU: what is called between a ctpn_detect_submit and its ctpn_detect_collect. A forward set, the proposal stream, the copy stream, the staging
buffers and one set of tail buffers are shared by everything a ctx does (csrc/ctx.h), and the header lets a caller do far more in between than
another submit. tests/inflight_cases.py puts every ctx-taking function of the ABI into one class (CLASSES; tests/test_inflight_cases.py holds
that none is missing); here each class is held to what it says, in both placements

  1   submit A slot 0 . X . collect 0                               2   submit A slot 0 . submit B slot 1 . X . collect 0 . collect 1

(A = 3 x 32 x 1040, B = 3 x 304 x 264 of tests/ctx_walks.py; in 2, forward_sets() shows B on set 1), with tail_overlap 0 and 1, by equality of bytes
(ctx_walks.same) with fresh(): the same call on a new ctx that has done nothing else.

  B2 test_between_calls_change_neither_batch   every X of inflight_cases.XS on one live ctx: the collects equal fresh uA / pAB, X's own result equals X
                                               on a fresh ctx or is its documented code (ctpn_detect* with both slots busy: CTPN_ERR_STATE), and uA run
                                               once more equals the fresh ctx's. The forward, proposal and detect families in four precisions, the
                                               image I/O units (JPEG decode with host and device entropy, the canvas packer, the crops, the JPEG and PNG
                                               encoders) in bf16
  B3 test_refused_calls_are_refused_and_harmless   every R of inflight_cases.REFUSED: CTPN_ERR_STATE and a text that names the function; the collects
                                               still equal the fresh results; once collected the same call succeeds. The weight loads one GPU can make
                                               are among them (W2, W1 itself -- the rule goes by state --, load_weights_device, ctpn_broadcast_weights_rank
                                               with world 1, ctpn_broadcast_weights of one handle). Then load W2: pAB is fresh W2's; load W1: fresh W1's
  B4 test_load_between_collect_and_submit      submit A 0 . submit B 1 . collect 0 . [load refused: slot 1 busy] . collect 1 . load W2 . submit A 0 .
                                               submit B 1 . collect both: fresh W2's

The load-in-flight cases of B3 and B4 pass because ctpn_load_weights_* / ctpn_broadcast_weights* drain and refuse (csrc/api_weights.hip,
weights_quiesce). Before that change they copied and packed on set 0's stream alone while set 1's stream and the proposal stream read the
packed weights, and answered CTPN_OK. Run once against a library built with the parent's api_weights.hip: all 16 of
test_refused_calls_are_refused_and_harmless fail with "load_weights_W2: not refused with a batch in flight" (and the same for load_weights_W1,
load_weights_device, broadcast_weights_rank, broadcast_weights), all 8 of test_load_between_collect_and_submit with DID NOT RAISE. At these
small shapes the batches had finished before the pack started, so the collected bytes were right there: the tests hold the refusal, they do
not try to win the race.

Outcome of B2: every between call passed in every precision, placement and tail_overlap value on the library as it is: none had to be
fixed or moved to the refused class.

Wall time of each parametrised test on one MI355X (pytest --durations; the 41 tests of the file together: 19 s):
test_between_calls_change_neither_batch 0.12 .. 0.31 s (1.4 s for the one that is first to ask for a precision's fresh results);
test_refused_calls_are_refused_and_harmless 0.64 .. 0.79 s (nine refusals, a 72 MB device copy of W2, seven loads; 1.9 s for the first of
the process); test_load_between_collect_and_submit below 0.3 s."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import ctx_walks as W
import inflight_cases as K

pytestmark = pytest.mark.gpu

OVERLAPS = (0, 1)


@pytest.fixture(autouse=True)
def _options_come_from_the_tests_only(monkeypatch):
    for var in B.OPTION_ENV.values():
        monkeypatch.delenv(var, raising=False)


def live(prec, overlap):
    ctx = ctpn_amd.Context(0, *W.CAP, prec, options={"tail_overlap": overlap})
    ctx.load_weights(K.arena("W1"))
    return ctx


def submit(ctx, placement):
    last = K.submit(ctx, placement)
    if placement == 2:
        sets = ctx.forward_sets()
        assert sets[0] == 2 and sets[3] == (0, 1), "the second batch does not run on forward set 1: %r" % (sets,)
    return last


def collected(ctx, prec, placement, akey="W1"):
    """-> None, or what differs between the placement's collects and the fresh results"""
    at = W.same(K.collect(ctx, placement), K.fresh(prec, akey, K.COLLECTED[placement]))
    return None if at is None else "the collected %s differs from the fresh ctx's (%s) in element %d" % (K.COLLECTED[placement], akey, at)


@pytest.mark.parametrize("placement", K.PLACEMENTS)
@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("prec", W.PRECS)
def test_between_calls_change_neither_batch(prec, overlap, placement):
    failed = []
    with live(prec, overlap) as ctx:
        for x in K.xs_for(prec):
            last = submit(ctx, placement)
            try:
                got = x.run(ctx, last, placement)
            except ctpn_amd.CtpnError as e:
                got = "raised %s" % e
            bad = collected(ctx, prec, placement)
            if bad:
                failed.append("%s: %s" % (x.name, bad))
            kind, what = x.expect(last, placement)
            if kind == "code":
                if got != (what,):
                    failed.append("%s: gave %r, not the code %d" % (x.name, got, what))
            else:
                opts = {"tail_overlap": overlap} if what == "introspect" else None          # the one X whose result names the option
                at = "raised" if isinstance(got, str) else W.same(got, K.fresh(prec, "W1", what, opts))
                if at is not None:
                    failed.append("%s: its own result differs from %s on a fresh ctx (%s)" % (x.name, what, got if isinstance(got, str) else "element %d" % at))
            at = W.same(W.OP["uA"].run(ctx), K.fresh(prec, "W1", "uA"))
            if at is not None:
                failed.append("%s: uA afterwards differs from the fresh ctx's in element %d" % (x.name, at))
    assert not failed, "%s, tail_overlap = %d, placement %d: %s" % (prec, overlap, placement, "; ".join(failed))


@pytest.mark.parametrize("placement", K.PLACEMENTS)
@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("prec", W.PRECS)
def test_refused_calls_are_refused_and_harmless(prec, overlap, placement):
    env = K.refused_env()
    env["rois"] = list(K.fresh(prec, "W1", "uC")[2:4])
    failed = []
    with live(prec, overlap) as ctx:
        for r in K.REFUSED:
            submit(ctx, placement)
            try:
                r.call(ctx, env)
                failed.append("%s: not refused with a batch in flight" % r.name)
            except ctpn_amd.CtpnError as e:
                if e.code != K.CTPN_ERR_STATE or r.fn not in str(e) or "has not been collected" not in str(e):
                    failed.append("%s: refused with %r" % (r.name, str(e)))
            bad = collected(ctx, prec, placement)
            if bad:
                failed.append("%s: %s" % (r.name, bad))
            if placement == 2 and r.name.startswith(("load_", "broadcast_")):          # slot 0 collected, slot 1 alone busy: still refused
                ctx.detect_submit(images=W.inputs()["B"], slot=1)
                with pytest.raises(ctpn_amd.CtpnError) as e:
                    r.call(ctx, env)
                assert e.value.code == K.CTPN_ERR_STATE, r.name
                ctx.detect_collect(1)
            try:
                r.call(ctx, env)                           # once collected, the same call succeeds
            except ctpn_amd.CtpnError as e:
                failed.append("%s: fails on the idle ctx: %s" % (r.name, e))
            r.undo(ctx, env)
            at = W.same(W.OP["uA"].run(ctx), K.fresh(prec, "W1", "uA"))
            if at is not None:
                failed.append("%s: uA afterwards differs from the fresh ctx's in element %d" % (r.name, at))
        for akey in ("W2", "W1"):
            ctx.load_weights(K.arena(akey))
            at = W.same(W.OP["pAB"].run(ctx), K.fresh(prec, akey, "pAB"))
            if at is not None:
                failed.append("after load_weights(%s): pAB differs from the fresh ctx's in element %d" % (akey, at))
    assert not failed, "%s, tail_overlap = %d, placement %d: %s" % (prec, overlap, placement, "; ".join(failed))


def test_the_text_line_tail_on_an_idle_ctx_is_the_fresh_one():
    """what ctpn_debug_text_lines gives once it is no longer refused: uC's own lines from uC's rois"""
    res = K.fresh("bf16", "W1", "uC")
    with live("bf16", 1) as ctx:
        submit(ctx, 2)
        K.collect(ctx, 2)
        got = K._text_lines(ctx, list(res[2:4]))
    assert W.same(got[:2], res[:2]) is None and sum(x.shape[0] for x in got[:2]) > 0


@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("prec", W.PRECS)
def test_load_between_collect_and_submit(prec, overlap):
    x = W.inputs()
    with live(prec, overlap) as ctx:
        submit(ctx, 2)
        a = ctx.detect_collect(0, want_rois=True)
        with pytest.raises(ctpn_amd.CtpnError) as e:       # slot 1 is still busy
            ctx.load_weights(K.arena("W2"))
        assert e.value.code == K.CTPN_ERR_STATE and "ctpn_load_weights_host" in str(e.value)
        b = ctx.detect_collect(1, want_rois=True)
        assert W.same(W._flat(a, b), K.fresh(prec, "W1", "pAB")) is None
        ctx.load_weights(K.arena("W2"))
        ctx.detect_submit(images=x["A"], slot=0)
        ctx.detect_submit(images=x["B"], slot=1)
        assert ctx.forward_sets()[3] == (0, 1)
        at = W.same(K.collect(ctx, 2), K.fresh(prec, "W2", "pAB"))
    assert at is None, "%s, tail_overlap = %d: pAB behind the load differs from the fresh W2 ctx's in element %d" % (prec, overlap, at)
